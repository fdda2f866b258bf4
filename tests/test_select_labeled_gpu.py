"""ss_reads_select_labeled (ss_label.hip): the records with at least N hits of one label, as a new resident set.  Read back, it is --
as a multiset of records -- what tests/label_model.py selects: the records with at least N hits against the sub-table "k-mers
with label j".  n_records and n_bases are exact."""
from collections import Counter

import numpy as np
import pytest

from tests import label_model, rs_model
from tests.test_support_labeled_gpu import _all_kmers, _distinct, _kfa, _labels, _one_length_block, _ragged_block, _rand

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def material():
    rs = np.random.RandomState(2025)
    g = _rand(rs, 70000)
    return dict(g=g, rep=b"", src=g)


@pytest.fixture(scope="module")
def table(L, material):
    kmers = _distinct(_all_kmers(material["g"][:40000], 31, 2))
    db = L.KmerDB.from_text(_kfa(kmers), 31, True)
    yield db, kmers, rs_model.encode_kmers(kmers, 31), _labels(len(kmers), 3, 77)
    db.close()


@pytest.fixture(scope="module")
def read_sets(L, material):
    import torch
    keep, out = [], {}
    for name, block, order in (("packed", _one_length_block(material), True), ("ragged", _ragged_block(material, 1), False)):
        d = torch.frombuffer(bytearray(block), dtype=torch.uint8).cuda()
        keep.append(d)
        out[name] = L.ReadSet.from_flat_dev(d.data_ptr(), d.numel(), order=order)
    L.check(L.lib().ss_device_sync(), "sync")
    assert out["packed"].packed_slabs() >= 1 and out["ragged"].packed_slabs() == 0
    yield {name: (r, r.read_back()) for name, r in out.items()}
    for r in out.values():
        r.close()


@pytest.mark.parametrize("min_hits", [1, 16, 100000])
@pytest.mark.parametrize("sname", ["packed", "ragged"])
def test_select_labeled_equals_model(L, table, read_sets, sname, min_hits):
    db, kmers, keys, lab = table
    rset, text = read_sets[sname]
    recs = [p for p in text.split(b"\n") if p]
    per = label_model.labeled_hits_per_record(text, keys, lab, 3, 31)
    before = db.counts_rows().copy()
    for j in (1, 3):                           # (label 2 has no row: covered below)
        want = [r for r, h in zip(recs, per[j].tolist()) if h >= min_hits]
        calls = L.labeled_calls()
        sub = rset.select_labeled(db, lab, 3, j, min_hits)
        try:
            assert L.labeled_calls() == calls + 1
            info = sub.info()
            got = [p for p in sub.read_back().split(b"\n") if p]
            print(sname, "label", j, "N", min_hits, "selected", info["n_records"], "model", len(want), "of", len(recs))
            assert info["n_records"] == len(want)
            assert info["n_bases"] == sum(len(r) for r in want)
            assert Counter(got) == Counter(want)
            if min_hits == 1:
                assert 0 < len(want) < len(recs)
            if min_hits == 100000:
                assert not want
            if want:
                # the selected records against the label's own table: every one has its N hits there
                own = L.KmerDB.from_text(_kfa([km for km, l in zip(kmers, lab.tolist()) if l == j]), 31, True)
                try:
                    hist, _ = sub.support(own, n_bins=min_hits + 1)
                    assert int(hist[min_hits]) == len(want)
                finally:
                    own.close()
        finally:
            sub.close()
    sub = rset.select_labeled(db, lab, 3, 2, 1)
    try:
        assert sub.info()["n_records"] == 0 and sub.info()["n_bases"] == 0
    finally:
        sub.close()
    assert (db.counts_rows() == before).all()
