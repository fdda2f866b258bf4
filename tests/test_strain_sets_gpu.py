"""ss_reads_classify_strains and ss_reads_select_strains (ss_strain_sets.hip; scan_minik_kernel's ClassSink with masks): every record
of a resident set assigned to the set of called strains with the most hits, held bit for bit to tests/strain_set_model.py for every
(table, read set, M) below; the inputs are those of tests/strain_set_cases.py, whose conditions against a vacuous pass
tests/test_strain_sets_host.py checks on the model.

Not covered here: the SS_ERANGE of a cut record (a cut record needs a record longer than a 32 MB block) and of more records than
an int holds; the SS_EINVAL of a table and a set on different devices (one device)."""
import gzip
import os

import numpy as np
import pytest

from tests import class_cases as cc, strain_set_cases as sc, strain_set_model as sm

pytestmark = pytest.mark.gpu

SETS = ["packed", "file_order", "binned_ascii", "ragged_0", "ragged_1", "ragged_1023", "two_slabs", "half_a", "half_b", "empty", "long"]
PAIRS = [(t, s) for t, v in sc.TABLES.items() for s in (SETS if not v[4] else ["long", "packed"])]


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def g():
    return cc.source()


@pytest.fixture(scope="module")
def tables(L, g):
    """name -> (KmerDB, k, n, row_sets of every row, keys and sets of the rows with a slot)"""
    out = {}
    for name, (_, _, expect, _, _) in sc.TABLES.items():
        k, n, kmers, row_sets, keys, vsets = sc.table(name, g)
        db = L.KmerDB.from_text(cc.kfa(kmers), k, True)
        assert db.n_rows == len(kmers)
        if expect:
            db.expect_hits(True)
        out[name] = (db, k, n, row_sets, keys, vsets)
    yield out
    for t in out.values():
        t[0].close()


def _fastq_gz(path, reads, seed):
    rs = np.random.RandomState(seed)
    qa = np.frombuffer(b"0123456789BCDEFGHIJ", np.uint8)
    out = [b"@r%d\n%s\n+\n%s\n" % (i, r, qa[rs.randint(0, qa.size, size=len(r))].tobytes()) for i, r in enumerate(reads)]
    with open(path, "wb") as f:
        f.write(gzip.compress(b"".join(out), 1))
    assert os.path.getsize(path) >= 1 << 20
    return path


@pytest.fixture(scope="module")
def read_sets(L, g, tmp_path_factory):
    """name -> (ReadSet, its bytes read back)"""
    import torch
    keep, out = [], {}

    def flat(block, order):
        d = torch.frombuffer(bytearray(block or b"\n"), dtype=torch.uint8).cuda()
        keep.append(d)
        rset = L.ReadSet.from_flat_dev(d.data_ptr(), len(block), order=order)
        L.check(L.lib().ss_device_sync(), "sync")
        return rset

    one = cc.one_length_block(g)
    out["packed"] = flat(one, True)
    assert out["packed"].packed_slabs() == 1
    out["file_order"] = flat(one, False)
    out["binned_ascii"] = flat(cc.one_length_block(g, lower=True), True)
    assert out["binned_ascii"].packed_slabs() == 0 and out["file_order"].packed_slabs() == 0
    for tail in (0, 1, 1023):
        out["ragged_%d" % tail] = flat(cc.ragged_block(g, tail), False)
    lines = one.split(b"\n")[:-1]
    out["half_a"] = flat(b"".join(r + b"\n" for r in lines[:1500]), False)
    out["half_b"] = flat(b"".join(r + b"\n" for r in lines[1500:]), True)
    out["empty"] = flat(b"", False)
    out["long"] = flat(sc.long_record_block(g), False)
    # two .fastq.gz files of 1 MB and more: the device path gives each a slab of its own, and record indices run on across slabs
    root = str(tmp_path_factory.mktemp("sets_gz"))
    paths = [_fastq_gz(os.path.join(root, "r%d.fastq.gz" % (m + 1)), reads, 100 + m) for m, reads in enumerate(sc.two_slab_reads(g))]
    out["two_slabs"] = L.ReadSet(paths)
    assert out["two_slabs"].info()["n_blocks"] >= 2
    sets = {name: (r, r.read_back()) for name, r in out.items()}
    yield sets
    for r in out.values():
        r.close()


_DONE = {}


def _classified(L, tables, read_sets, tname, sname):
    """the device's and the model's results of one (table, set) at every M, computed once: {m: (device dict, model dict, records)}"""
    if (tname, sname) in _DONE:
        return _DONE[tname, sname]
    db, k, n, row_sets, keys, vsets = tables[tname]
    rset, text = read_sets[sname]
    per, n_rec = sm.record_votes(text, keys, vsets, k)
    res = {}
    for m in sc.MS:
        calls = L.classify_strains_calls()
        got = rset.classify_strains(db, row_sets, n, m, want_sets=True, want_records=True)
        assert L.classify_strains_calls() == calls + 1
        res[m] = (got, sm.classify_strains_model(text, keys, vsets, n, k, m, per), n_rec)
    _DONE[tname, sname] = res
    return res


@pytest.mark.parametrize("tname,sname", PAIRS)
def test_sets_equal_the_model(L, tables, read_sets, tname, sname):
    n = sc.TABLES[tname][3]
    for m, (got, want, n_rec) in _classified(L, tables, read_sets, tname, sname).items():
        print(tname, sname, "M", m, "records", n_rec, "unique", int(got["unique"][1:].sum()), "tied", int(got["tied"][0]), "unassigned",
              int(got["unique"][0]), "distinct sets", int((got["set_reads"] > 0).sum()), "largest score", int(got["scores"].max()) if n_rec else 0)
        for key in ("unique", "tied", "strain_hits", "kmers"):
            assert got[key].dtype == np.uint64 and got[key].shape == (n + 1,)
            assert (got[key] == want[key]).all(), (key, got[key], want[key])
        assert got["set_reads"].shape == (1 << n,) and (got["set_reads"] == want["set_reads"]).all()
        assert got["sets"].dtype == np.uint16 and got["sets"].tolist() == want["sets"].tolist()
        assert got["scores"].dtype == np.uint32 and got["scores"].tolist() == want["scores"].tolist()
        assert got["ties"] == want["ties"] == int(got["tied"][0])
        # the invariants
        assert int(got["set_reads"].sum()) == n_rec == int(got["unique"].sum() + got["tied"][0])
        assert all(int(got["unique"][j]) == int(got["set_reads"][1 << (j - 1)]) for j in range(1, n + 1))
        assert int(got["kmers"][0]) == 0
    if sname == "long":
        assert n_rec == 1 and int(got["scores"][0]) > 4095           # (more than the per-thread pass counts)


def test_the_long_record_outgrows_sixteen_bits(L, tables, read_sets):
    got = _classified(L, tables, read_sets, "k31_whole_n2", "long")[1][0]
    assert int(got["scores"][0]) > 65535 and got["sets"].tolist() == [1] and int(got["strain_hits"][1]) == int(got["scores"][0])


@pytest.mark.parametrize("tname", [t for t, v in sc.TABLES.items() if not v[4]])
def test_layouts_agree_and_halves_add_up(L, tables, read_sets, tname):
    r = {s: _classified(L, tables, read_sets, tname, s) for s in ("packed", "file_order", "binned_ascii", "half_a", "half_b")}
    db, _, n, row_sets, _, _ = tables[tname]
    for m in sc.MS:
        a, b, c = (r[s][m][0] for s in ("packed", "file_order", "binned_ascii"))
        ha, hb = r["half_a"][m][0], r["half_b"][m][0]
        for key in ("unique", "tied", "strain_hits", "set_reads"):
            assert (a[key] == b[key]).all() and (a[key] == c[key]).all(), key
            assert (ha[key] + hb[key] == a[key]).all(), key
        assert (ha["kmers"] == a["kmers"]).all()
    # without the sets and the records: the same numbers
    plain = read_sets["packed"][0].classify_strains(db, row_sets, n, 1, want_sets=False)
    assert plain["set_reads"] is None and plain["sets"] is None and (plain["unique"] == r["packed"][1][0]["unique"]).all()
    assert (plain["tied"] == r["packed"][1][0]["tied"]).all() and (plain["strain_hits"] == r["packed"][1][0]["strain_hits"]).all()


@pytest.mark.parametrize("sname", ["packed", "ragged_1", "two_slabs"])
@pytest.mark.parametrize("tname", ["k25_n15", "k31_sampled_n2", "k31_n1"])
def test_one_bit_masks_give_the_hits_of_support_labeled(L, tables, read_sets, tname, sname):
    db, _, n, row_sets, _, _ = tables[tname]
    rset = read_sets[sname][0]
    low, lab = sc.one_bit_rows(row_sets)
    got = rset.classify_strains(db, low, n, 1)
    _, hits, kmers = rset.support_labeled(db, lab, n)
    assert got["strain_hits"][1:].tolist() == hits.tolist() and int(hits.sum()) > 0
    assert got["kmers"][1:].tolist() == kmers.tolist()
    assert int(got["tied"][0]) == 0 or n > 1                        # (one-bit masks still tie where two strains have as many hits)
    _, total = rset.support(db)
    assert int(got["strain_hits"].sum()) == total
    # the call leaves the table's counters alone
    db.reset()
    rset.scan_into(db)
    L.check(L.lib().ss_device_sync(), "sync")
    before = db.counts_rows().copy()
    rset.classify_strains(db, row_sets, n, 2)
    assert (db.counts_rows() == before).all() and int(before.sum()) > 0
    db.reset()


def _records(text):
    return [r for r in text.split(b"\n") if r]


def _wanted(want_model, n):
    """entries (want, how): the unassigned, a single strain, a set of several, and a set that nobody has -- each both ways"""
    sr = want_model["set_reads"]
    single = next((m for m in range(1, 1 << n) if sm.popcount(m) == 1 and sr[m]), 1)
    multi = next((m for m in range(1, 1 << n) if sm.popcount(m) > 1 and sr[m]), single)
    nobody = next((m for m in range((1 << n) - 1, 0, -1) if not sr[m]), 0)
    masks = [0, single, multi] + ([nobody] if nobody else [])
    return [(m, how) for m in masks for how in (0, 1)]


@pytest.mark.parametrize("sname", ["packed", "ragged_1", "two_slabs", "long", "empty"])
@pytest.mark.parametrize("tname", ["k31_dense_n16", "k25_n15", "k31_sampled_n2"])
def test_selection_equals_the_model(L, tables, read_sets, tname, sname):
    db, _, n, row_sets, _, _ = tables[tname]
    rset, text = read_sets[sname]
    recs = _records(text)
    for m in (1, 8):
        got, want, n_rec = _classified(L, tables, read_sets, tname, sname)[m]
        entries = _wanted(want, n) if n_rec else [(0, 0), (1, 1)]
        calls, ccalls = L.select_strains_calls(), L.classify_strains_calls()
        subs, counts = rset.select_strains(db, row_sets, n, m, [e[0] for e in entries], [e[1] for e in entries], want_counts=True)
        assert L.select_strains_calls() == calls + 1 and L.classify_strains_calls() == ccalls
        try:
            for key in ("unique", "tied", "strain_hits", "kmers"):
                assert (counts[key] == got[key]).all(), key
            assert counts["ties"] == got["ties"]
            for (mask, how), sub in zip(entries, subs):
                idx = sm.selected(want["sets"], mask, how)
                back = _records(sub.read_back())
                print(tname, sname, "M", m, "want", bin(mask), "how", how, "records", len(back))
                assert sorted(back) == sorted(recs[i] for i in idx), (mask, how)
                info = sub.info()
                assert info["n_records"] == len(idx) and info["n_bases"] == sum(len(recs[i]) for i in idx)
                if mask == 0:
                    assert len(idx) == (int(got["unique"][0]) if how == 0 else 0)
        finally:
            for sub in subs:
                sub.close()


def test_thirty_two_entries_in_one_call(L, tables, read_sets):
    db, _, n, row_sets, _, _ = tables["k31_dense_n16"]
    rset, text = read_sets["ragged_1023"]
    recs = _records(text)
    _, want, _ = _classified(L, tables, read_sets, "k31_dense_n16", "ragged_1023")[1]
    masks = [1 << (i % n) for i in range(16)] + [int(m) for m in np.argsort(-want["set_reads"].astype(np.int64), kind="stable")[:16]]
    hows = [1] * 16 + [0] * 16
    assert len(masks) == L.SELECT_STRAINS_MAX
    subs = rset.select_strains(db, row_sets, n, 1, masks, hows)
    try:
        total = 0
        for mask, how, sub in zip(masks, hows, subs):
            idx = sm.selected(want["sets"], mask, how)
            total += len(idx)
            assert sorted(_records(sub.read_back())) == sorted(recs[i] for i in idx), (mask, how)
        assert total > 0
    finally:
        for sub in subs:
            sub.close()


def test_argument_errors(L, g, tables, read_sets):
    rset = read_sets["packed"][0]
    db, _, n, row_sets, _, _ = tables["k25_n15"]

    def raw(row=row_sets, n_strains=n, m=1, skip=None):
        """the C call itself; skip: the argument passed as NULL"""
        bufs = [np.zeros(17, np.uint64) for _ in range(4)]
        args = dict(db=db.handle, r=rset._h, row=L.ptr(row), unique=L.ptr(bufs[0]), tied=L.ptr(bufs[1]), hits=L.ptr(bufs[2]), kmers=L.ptr(bufs[3]))
        if skip:
            args[skip] = None
        return L.lib().ss_reads_classify_strains(args["db"], args["r"], args["row"], n_strains, m, args["unique"], args["tied"], args["hits"],
                                                 args["kmers"], None, None, None)

    def raw_select(want, how, n_want, n_strains=n, m=1, no_out=False):
        w, h = np.array(want, np.uint16), np.array(how, np.uint8)
        hs = (L.C.c_void_p * 40)()
        rc = L.lib().ss_reads_select_strains(db.handle, rset._h, L.ptr(row_sets), n_strains, m, L.ptr(w), L.ptr(h), n_want, None if no_out else hs,
                                             None, None, None, None)
        made = [x for x in hs[:max(min(n_want, 40), 0)] if x]
        if rc:
            assert not made                                           # on an error every out[i] is NULL
        for x in made:
            L.lib().ss_reads_destroy(L.C.c_void_p(x))
        return rc

    calls = L.classify_strains_calls()
    assert raw() == 0
    assert L.classify_strains_calls() == calls + 1
    for skip in ("db", "r", "row", "unique", "tied", "hits", "kmers"):
        assert raw(skip=skip) == L.SS_EINVAL, skip
    assert raw(m=0) == L.SS_EINVAL
    assert raw(n_strains=0) == L.SS_EINVAL
    assert raw(n_strains=17) == L.SS_EINVAL
    assert raw(n_strains=16) == 0                                     # the cap itself is served
    assert raw(n_strains=n - 1) == L.SS_EINVAL                        # a mask bit at or above n_strains
    with pytest.raises(ValueError):
        rset.classify_strains(db, row_sets[:-1], n, 1)
    assert L.classify_strains_calls() == calls + 2

    scalls = L.select_strains_calls()
    assert raw_select([1, 3], [0, 1], 2) == 0
    assert L.select_strains_calls() == scalls + 1
    assert raw_select([1], [0], 0) == L.SS_EINVAL
    assert raw_select([1] * 33, [0] * 33, 33) == L.SS_EINVAL
    assert raw_select([1] * 32, [0] * 32, 32) == 0
    assert raw_select([1], [2], 1) == L.SS_EINVAL                     # neither equals nor intersects
    assert raw_select([1 << n], [0], 1) == L.SS_EINVAL                # a strain that is not there
    assert raw_select([1], [0], 1, m=0) == L.SS_EINVAL
    assert raw_select([1], [0], 1, n_strains=17) == L.SS_EINVAL
    assert raw_select([1], [0], 1, no_out=True) == L.SS_EINVAL
    assert L.select_strains_calls() == scalls + 2

    k15m = list(dict.fromkeys(g[i:i + 15] for i in range(0, 5000, 5)))
    k15 = L.KmerDB.from_text(cc.kfa(k15m), 15, True)
    try:
        with pytest.raises(L.SSError) as e:
            rset.classify_strains(k15, np.ones(len(k15m), np.uint16), 2, 1)      # a flat table
        assert e.value.code == L.SS_ERANGE
        with pytest.raises(L.SSError) as e:
            rset.select_strains(k15, np.ones(len(k15m), np.uint16), 2, 1, [1], [0])
        assert e.value.code == L.SS_ERANGE
    finally:
        k15.close()
    assert L.classify_strains_calls() == calls + 2 and L.select_strains_calls() == scalls + 2
