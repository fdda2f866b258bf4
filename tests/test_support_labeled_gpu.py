"""ss_reads_support_labeled (ss_label.hip, scan_minik_kernel's LabelSink): read support per label of a table's rows, held bit for
bit to tests/label_model.py -- rs_model on each label's sub-table -- and to ss_reads_support against a table built from that
label's k-mers alone, for every (table, read set, label count) below.  The labels' hits and label 0's add up to the unlabelled
total; the table's counters are the same before and after.

Not covered here: the SS_ERANGE of a cut record at k != 31 (a cut record needs a record longer than a 32 MB block)."""
import gzip
import os

import numpy as np
import pytest

from tests import label_model, rs_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _rand(rs, n):
    return np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, size=n)].tobytes()


def _distinct(kmers):
    return list(dict.fromkeys(kmers))


def _kfa(kmers):
    return b"".join(b">1\n" + km + b"\n" for km in kmers)


def _all_kmers(g, k, step=1):
    return [g[i:i + k] for i in range(0, len(g) - k + 1, step)]


@pytest.fixture(scope="module")
def material():
    rs = np.random.RandomState(2025)
    g = _rand(rs, 70000)
    stretch = _rand(rs, 60)
    rep = b"".join(_rand(rs, 1128) + stretch for _ in range(5))
    rep += _rand(rs, 6000 - len(rep))
    return dict(g=g, rep=rep, src=g + rep)


TABLES = ["k31_dense", "k31_sampled", "k31_repeat", "k25", "k17"]


@pytest.fixture(scope="module")
def tables(L, material):
    """name -> (KmerDB, k, kmers, model keys); every table's k-mers are distinct: row i is k-mer i"""
    g = material["g"]
    spec = {
        "k31_dense": (31, _all_kmers(g[:20000], 31), True),               # solid buckets; expects hits
        "k31_sampled": (31, _all_kmers(g, 31, 7), False),                 # inline slots, a Bloom filter
        "k31_repeat": (31, _all_kmers(material["rep"], 31), False),       # several k-mers per minimizer offset
        "k25": (25, _all_kmers(g, 25, 3), False),
        "k17": (17, _all_kmers(g[:30000], 17), False),
    }
    out = {}
    for name, (k, kmers, expect) in spec.items():
        kmers = _distinct(kmers)
        assert len(kmers) <= 70000
        db = L.KmerDB.from_text(_kfa(kmers), k, True)
        if expect:
            db.expect_hits(True)
        out[name] = (db, k, kmers, rs_model.encode_kmers(kmers, k))
    yield out
    for db, _, _, _ in out.values():
        db.close()


def _one_length_block(material):
    rs = np.random.RandomState(7)
    src = np.frombuffer(material["src"], np.uint8)
    starts = rs.randint(0, src.size - 150, size=3000)
    arr = src[starts[:, None] + np.arange(150)[None, :]].copy()
    arr[::53, :][np.arange(len(arr[::53])), rs.randint(0, 150, size=len(arr[::53]))] = ord("N")
    arr[5::211, 0] = ord("N")
    arr[9::223, 149] = ord("N")
    return b"".join(a.tobytes() + b"\n" for a in arr)


def _ragged_block(material, tail_mod):
    """Lengths 1, 30, 31, 32 and 150, a record that spans three tiles, lower case, N inside and at the ends, an empty record; the
    block's length is tail_mod modulo 1024."""
    rs = np.random.RandomState(11)
    g, src = material["g"], material["src"]
    recs = []
    for i in range(2400):
        ln = (1, 30, 31, 32, 150, 150, 150, 150)[i % 8]
        s = rs.randint(0, len(src) - ln)
        r = bytearray(src[s:s + ln])
        if i % 17 == 0 and ln > 40:
            a = rs.randint(0, ln - 35)
            r[a:a + 35] = bytes(r[a:a + 35]).lower()
        if i % 19 == 0:
            r[rs.randint(0, ln)] = ord("N")
        if i % 41 == 0:
            r[0] = ord("N")
        if i % 43 == 0:
            r[-1] = ord("n")
        recs.append(bytes(r))
    recs.insert(700, g[1000:3500])             # spans three tiles
    block = b"\n".join(recs[:1000]) + b"\n\n" + b"\n".join(recs[1000:]) + b"\n"      # (two '\n' in a row: an empty record)
    last = (tail_mod - len(block) - 1) % 1024
    if last < 40:
        last += 1024
    block += src[300:300 + last] + b"\n"
    assert len(block) % 1024 == tail_mod
    return block


def _fastq_gz(path, reads, seed):
    rs = np.random.RandomState(seed)
    qa = np.frombuffer(b"0123456789BCDEFGHIJ", np.uint8)
    out = [b"@r%d\n%s\n+\n%s\n" % (i, r, qa[rs.randint(0, qa.size, size=len(r))].tobytes()) for i, r in enumerate(reads)]
    with open(path, "wb") as f:
        f.write(gzip.compress(b"".join(out), 1))
    assert os.path.getsize(path) >= 1 << 20
    return path


SETS = ["packed", "ragged_1024", "ragged_1025", "two_slabs"]


@pytest.fixture(scope="module")
def read_sets(L, material, tmp_path_factory):
    """name -> (ReadSet, its bytes read back)"""
    import torch
    keep, out = [], {}

    def flat(block, order):
        d = torch.frombuffer(bytearray(block), dtype=torch.uint8).cuda()
        keep.append(d)
        rset = L.ReadSet.from_flat_dev(d.data_ptr(), d.numel(), order=order)
        L.check(L.lib().ss_device_sync(), "sync")
        return rset

    out["packed"] = flat(_one_length_block(material), True)
    assert out["packed"].packed_slabs() >= 1
    out["ragged_1024"] = flat(_ragged_block(material, 0), False)
    out["ragged_1025"] = flat(_ragged_block(material, 1), False)
    # two .fastq.gz files of 1 MB and more (2 x 1 250 reads of 1 000 bases): the device path gives each a slab of its own, and record
    # indices run on across slabs
    rs = np.random.RandomState(13)
    src = material["src"]
    root = str(tmp_path_factory.mktemp("lab_gz"))
    paths = []
    for m in range(2):
        reads = [src[s:s + 1000] for s in rs.randint(0, len(src) - 1000, size=1250)]
        paths.append(_fastq_gz(os.path.join(root, "r%d.fastq.gz" % (m + 1)), reads, 100 + m))
    out["two_slabs"] = L.ReadSet(paths)
    assert out["two_slabs"].info()["n_blocks"] >= 2
    sets = {name: (r, r.read_back()) for name, r in out.items()}
    yield sets
    for r in out.values():
        r.close()


def _labels(n_rows, n_labels, seed):
    """random labels over the rows: label 0 among them, and -- from three labels on -- one label that no row has"""
    rs = np.random.RandomState(seed)
    pool = [j for j in range(n_labels + 1) if not (n_labels >= 3 and j == (n_labels + 1) // 2)]
    lab = np.array(pool, np.uint8)[rs.randint(0, len(pool), size=n_rows)]
    assert (lab == 0).any()
    return lab


_UNLABELLED = {}


@pytest.mark.parametrize("n_labels", [1, 3, 15])
@pytest.mark.parametrize("tname", TABLES)
def test_labeled_support_equals_model_and_sub_tables(L, tables, read_sets, tname, n_labels):
    assert L.LABELS_MAX == 15
    db, k, kmers, keys = tables[tname]
    lab = _labels(len(kmers), n_labels, 1000 + n_labels)
    empty = [j for j in range(1, n_labels + 1) if not (lab == j).any()]
    assert bool(empty) == (n_labels >= 3)
    # a table per label, from that label's k-mers alone
    subs = {}
    for j in range(1, n_labels + 1):
        own = [km for km, l in zip(kmers, lab.tolist()) if l == j]
        if own:
            subs[j] = L.KmerDB.from_text(_kfa(own), k, True)
    try:
        for sname in SETS:
            rset, text = read_sets[sname]
            n_rec = sum(1 for p in text.split(b"\n") if p)
            if (tname, sname) not in _UNLABELLED:
                db.reset()
                rset.scan_into(db)                 # (counters that are not zero: what the labelled call must leave alone)
                L.check(L.lib().ss_device_sync(), "sync")
                _UNLABELLED[tname, sname] = rset.support(db)[1]
            hits0 = _UNLABELLED[tname, sname]
            before = db.counts_rows().copy()
            calls = L.labeled_calls()
            hist, hits, nk = rset.support_labeled(db, lab, n_labels)
            assert L.labeled_calls() == calls + 1
            assert (db.counts_rows() == before).all()
            per = label_model.labeled_hits_per_record(text, keys, lab, n_labels, k)
            want_hist, want_hits, want_k = label_model.labeled_support_model(text, keys, lab, n_labels, k)
            print(tname, sname, "labels", n_labels, "records", n_rec, "hits", hits.tolist(), "model", want_hits, "label 0", int(per[0].sum()),
                  "unlabelled", hits0)
            assert hist.shape == (n_labels, 65) and hist.dtype == np.uint64
            assert hits.tolist() == want_hits
            assert nk.tolist() == want_k
            assert (hist == want_hist).all()
            assert (hist.sum(axis=1) == n_rec).all()
            assert int(hits.sum()) + int(per[0].sum()) == hits0
            for j in range(1, n_labels + 1):
                if j in subs:
                    h1, t1 = rset.support(subs[j])
                    assert t1 == int(hits[j - 1]) and (h1 == hist[j - 1]).all(), (sname, j)
                    assert subs[j].info()["n_distinct"] == int(nk[j - 1])
                else:
                    assert int(hits[j - 1]) == 0 and int(nk[j - 1]) == 0 and int(hist[j - 1, 0]) == n_rec
            if sname == "packed":
                h2, t2, _ = rset.support_labeled(db, lab, n_labels, n_bins=2)
                assert t2.tolist() == want_hits and (h2.sum(axis=1) == n_rec).all()
                assert (h2[:, 0] == hist[:, 0]).all()
    finally:
        for s in subs.values():
            s.close()


def test_a_kmer_listed_twice_under_different_labels_counts_for_nobody(L, material, read_sets):
    """rows 0..999 once, then rows 0..99 again under another label (their slots: no label) and rows 100..199 again under the same
    label (their slots: that label)"""
    g = material["g"]
    base = _distinct(_all_kmers(g[:1500], 31))[:1000]
    kmers = base + base[:200]
    lab = np.concatenate([np.full(500, 1), np.full(500, 2), np.full(100, 2), np.full(100, 1)]).astype(np.uint8)
    keys = rs_model.encode_kmers(kmers, 31)
    uk, ul = label_model.kmer_labels(keys, lab)
    assert uk.size == 1000 and int((ul == 0).sum()) == 100 and int((ul == 1).sum()) == 400 and int((ul == 2).sum()) == 500
    db = L.KmerDB.from_text(_kfa(kmers), 31, True)
    try:
        assert db.info()["n_distinct"] == 1000
        block = b"".join(g[s:s + 150] + b"\n" for s in range(0, 1400, 7))
        import torch
        d = torch.frombuffer(bytearray(block), dtype=torch.uint8).cuda()
        rset = L.ReadSet.from_flat_dev(d.data_ptr(), d.numel(), order=False)
        try:
            text = rset.read_back()
            hist, hits, nk = rset.support_labeled(db, lab, 2)
            want_hist, want_hits, want_k = label_model.labeled_support_model(text, keys, lab, 2, 31)
            per = label_model.labeled_hits_per_record(text, keys, lab, 2, 31)
            print("hits", hits.tolist(), "model", want_hits, "conflicting", int(per[0].sum()))
            assert int(per[0].sum()) > 0 and min(want_hits) > 0
            assert nk.tolist() == want_k == [400, 500]
            assert hits.tolist() == want_hits
            assert (hist == want_hist).all()
            _, total = rset.support(db)
            assert int(hits.sum()) + int(per[0].sum()) == total
        finally:
            rset.close()
    finally:
        db.close()


def test_argument_errors(L, material, tables, read_sets):
    rset = read_sets["packed"][0]
    db, _, kmers, _ = tables["k25"]
    lab = np.zeros(len(kmers), np.uint8)
    lab[::3] = 2

    def code(fn):
        with pytest.raises(L.SSError) as e:
            fn()
        return e.value.code

    calls = L.labeled_calls()
    assert code(lambda: rset.support_labeled(db, lab, 1)) == L.SS_EINVAL              # a label above n_labels
    assert code(lambda: rset.select_labeled(db, lab, 1, 1, 1)) == L.SS_EINVAL
    assert code(lambda: rset.support_labeled(db, lab, 0)) == L.SS_EINVAL              # n_labels outside 1 .. max
    assert code(lambda: rset.support_labeled(db, lab, L.LABELS_MAX + 1)) == L.SS_EINVAL
    assert code(lambda: rset.select_labeled(db, lab, 0, 1, 1)) == L.SS_EINVAL
    assert code(lambda: rset.select_labeled(db, lab, L.LABELS_MAX + 1, 1, 1)) == L.SS_EINVAL
    assert code(lambda: rset.select_labeled(db, lab, 2, 0, 1)) == L.SS_EINVAL         # label outside 1 .. n_labels
    assert code(lambda: rset.select_labeled(db, lab, 2, 3, 1)) == L.SS_EINVAL
    assert code(lambda: rset.select_labeled(db, lab, 2, 2, 0)) == L.SS_EINVAL         # min_hits 0, as ss_reads_select
    assert code(lambda: rset.support_labeled(db, lab, 2, n_bins=1)) == L.SS_EINVAL    # as ss_reads_support
    with pytest.raises(ValueError):
        rset.support_labeled(db, lab[:-1], 2)
    k15m = _distinct(_all_kmers(material["g"][:5000], 15, 5))
    k15 = L.KmerDB.from_text(_kfa(k15m), 15, True)
    try:
        assert code(lambda: rset.support_labeled(k15, np.ones(len(k15m), np.uint8), 1)) == L.SS_ERANGE      # a flat table
        assert code(lambda: rset.select_labeled(k15, np.ones(len(k15m), np.uint8), 1, 1, 1)) == L.SS_ERANGE
    finally:
        k15.close()
    assert L.labeled_calls() == calls
    rset.support_labeled(db, lab, 2)
    assert L.labeled_calls() == calls + 1
