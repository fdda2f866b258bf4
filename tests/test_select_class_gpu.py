"""ss_reads_select_class (ss_classify.hip): the records of chosen clades of a resident set's classification as new resident sets,
held record for record to tests/select_class_model.py for every (table, read set, M) below and the clade list of
tests/test_select_class_host.py, which checks on the model that no listed clade passes vacuously.  The inputs are those of
tests/class_cases.py, the read sets are built as tests/test_classify_gpu.py builds them.

Not covered here, as in tests/test_classify_gpu.py: the SS_ERANGE of a cut record (a cut record needs a record longer than a
32 MB block; the test the call shares with ss_reads_classify is the one line `R->has_cut_record`) and of more records than an int
holds; the SS_EINVAL of a table and a set on different devices (one device)."""
import ctypes as C

import numpy as np
import pytest

from tests import class_cases as cc, class_model as cm, select_class_model as scm
from tests.test_select_class_host import CLADES

pytestmark = pytest.mark.gpu

MS = (1, 3)
SETS = ["packed", "file_order", "binned_ascii", "ragged_1", "ragged_1023", "ragged_binned_1", "ragged_binned_1023", "half_a", "half_b", "empty"]


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
    """name -> (KmerDB, k, keys, row_node)"""
    out = {}
    for name, (k, _, expect) in cc.TABLES.items():
        _, kmers, keys, row_node = cc.table(name, g)
        db = L.KmerDB.from_text(cc.kfa(kmers), k, True)
        if expect:
            db.expect_hits(True)
        out[name] = (db, k, keys, row_node)
    yield out
    for db, _, _, _ in out.values():
        db.close()


@pytest.fixture(scope="module")
def read_sets(L, g):
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
    for tail in (1, 1023):
        out["ragged_%d" % tail] = flat(cc.ragged_block(g, tail), False)
        out["ragged_binned_%d" % tail] = flat(cc.ragged_block(g, tail), True)
    lines = one.split(b"\n")[:-1]
    out["half_a"] = flat(b"".join(r + b"\n" for r in lines[:1500]), False)
    out["half_b"] = flat(b"".join(r + b"\n" for r in lines[1500:]), True)
    out["empty"] = flat(b"", False)
    sets = {name: (r, r.read_back()) for name, r in out.items()}
    yield sets
    for r in out.values():
        r.close()


_HITS = {}


@pytest.fixture(scope="module")
def record_hits(tables, read_sets):
    """(table, set) -> the model's hits per record of the set's text (class_model.record_hits), computed once"""
    def get(tname, sname):
        if (tname, sname) not in _HITS:
            _, k, keys, row_node = tables[tname]
            _HITS[tname, sname] = cm.record_hits(read_sets[sname][1], keys, row_node, k)
        return _HITS[tname, sname]
    yield get
    _HITS.clear()


def _records(rset):
    """the non-empty records of a set, sorted"""
    return sorted(r for r in rset.read_back().split(b"\n") if r)


_DONE = {}


def _selected(L, tables, read_sets, record_hits, tname, sname):
    """{m: (device lists per clade, infos per clade, counts, model lists per clade)} of one (table, set), computed once; the sets
    themselves are checked and closed here"""
    if (tname, sname) in _DONE:
        return _DONE[tname, sname]
    db, k, keys, row_node = tables[tname]
    rset, text = read_sets[sname]
    par = cc.parents()
    per, n_rec = record_hits(tname, sname)
    res = {}
    for m in MS:
        calls, ccalls = L.select_class_calls(), L.classify_calls()
        sets, counts = rset.select_class(db, row_node, par, m, CLADES, want_counts=True)
        assert L.select_class_calls() == calls + 1 and L.classify_calls() == ccalls
        assert len(sets) == len(CLADES)
        lists, infos = [], []
        for sub in sets:
            lists.append(_records(sub))
            infos.append(sub.info())
            hist, _ = sub.support(db, 2)
            assert int(hist.sum()) == infos[-1]["n_records"]                 # support() on the set sums to its records
            sub.close()
        classes = cm.classes_per_record(text, keys, row_node, par, k, m, per)
        res[m] = (lists, infos, counts, [scm.selected(text, classes, par, c) for c in CLADES], n_rec)
    _DONE[tname, sname] = res
    return res


@pytest.mark.parametrize("sname", SETS)
@pytest.mark.parametrize("tname", list(cc.TABLES))
def test_sets_equal_the_model(L, tables, read_sets, record_hits, tname, sname):
    db, _, _, row_node = tables[tname]
    rset = read_sets[sname][0]
    for m, (lists, infos, counts, want, n_rec) in _selected(L, tables, read_sets, record_hits, tname, sname).items():
        print(tname, sname, "M", m, "records", n_rec, "per clade", [len(x) for x in lists], "model", [len(x) for x in want])
        for i, c in enumerate(CLADES):
            assert lists[i] == want[i], (c, len(lists[i]), len(want[i]))
            assert infos[i]["n_records"] == len(want[i]) and infos[i]["n_bases"] == sum(len(r) for r in want[i]), c
        # the numbers of the same call are classify()'s for the same arguments
        ref = rset.classify(db, row_node, cc.parents(), m)
        for key in ("direct", "node_hits", "kmers"):
            assert counts[key].dtype == np.uint64 and (counts[key] == ref[key]).all(), key
        assert counts["ties"] == ref["ties"]
        assert int(counts["direct"].sum()) == n_rec
        clade = cm.clade_sums(counts["direct"], cc.parents(), cc.N_NODES)
        assert [len(x) for x in lists] == [clade[c] for c in CLADES]         # reads_clade of read_classes.tsv
        assert lists[1] == lists[9]                                          # the clade listed twice: two equal sets
        assert lists[7] == [] and lists[8] == []
    if sname not in ("empty", "half_a", "half_b"):                           # (the whole blocks: test_select_class_host.py's conditions)
        lists1, lists3 = (_DONE[tname, sname][m][0] for m in MS)
        assert len(lists3[0]) > len(lists1[0]) > 0 and len(lists1[1]) > len(lists1[2]) > 0


@pytest.mark.parametrize("tname", list(cc.TABLES))
def test_layouts_agree_and_halves_add_up(L, tables, read_sets, record_hits, tname):
    r = {s: _selected(L, tables, read_sets, record_hits, tname, s) for s in
         ("packed", "file_order", "binned_ascii", "half_a", "half_b", "ragged_1", "ragged_binned_1", "ragged_1023", "ragged_binned_1023")}
    for m in MS:
        a, b, c = (r[s][m][0] for s in ("packed", "file_order", "binned_ascii"))
        assert a == b
        assert [sorted(x.upper() for x in lst) for lst in c] == a            # (the ASCII slab keeps its one lower-case base)
        assert any(x != x.upper() for lst in c for x in lst)
        for tail in (1, 1023):
            assert r["ragged_%d" % tail][m][0] == r["ragged_binned_%d" % tail][m][0]
        ha, hb = r["half_a"][m][0], r["half_b"][m][0]
        assert [sorted(x + y) for x, y in zip(ha, hb)] == a
        for key in ("direct", "node_hits"):
            assert (r["half_a"][m][2][key] + r["half_b"][m][2][key] == r["packed"][m][2][key]).all()


def test_a_set_is_a_read_set(L, tables, read_sets):
    """an empty clade's set can be scanned; a set scans to the counts of its own text, and order() keeps its records"""
    db, k, keys, row_node = tables["k31_dense"]
    rset = read_sets["ragged_1"][0]
    sets = rset.select_class(db, row_node, cc.parents(), 1, [121, 41, 0])
    try:
        empty, sub, unc = sets
        assert empty.info()["n_records"] == 0 and empty.info()["n_bases"] == 0 and _records(empty) == []
        db.reset()
        empty.scan_into(db)
        L.check(L.lib().ss_device_sync(), "sync")
        assert not db.counts_rows().any()
        sub.scan_into(db)
        L.check(L.lib().ss_device_sync(), "sync")
        got = db.counts_rows().copy()
        db.reset()
        db.scan_flat(b"".join(r + b"\n" for r in _records(sub)))
        assert got.any() and (db.counts_rows() == got).all()
        before = _records(unc)
        n = unc.info()["n_records"]
        unc.order()
        assert _records(unc) == before and unc.info()["n_records"] == n == len(before) > 0
        assert int(unc.support(db, 2)[0].sum()) == n
    finally:
        db.reset()
        for s in sets:
            s.close()


def test_argument_errors(L, g, tables, read_sets):
    rset = read_sets["packed"][0]
    db, _, _, row_node = tables["k25"]
    par = cc.parents()
    n = cc.N_NODES
    junk = 0xDEAD0

    def raw(row=row_node, parent=par, n_nodes=n, m=1, clades=(0, 41), n_clades=None, skip=None, counts=False, dbh=None):
        """the C call itself -> (status, out[]); skip: the argument passed as NULL.  out[] comes in filled with a value that is no set."""
        cl = np.array(clades, np.uint32)
        nc = len(cl) if n_clades is None else n_clades
        out = (C.c_void_p * max(nc, len(cl), 1))(*([junk] * max(nc, len(cl), 1)))
        bufs = [np.zeros(n_nodes + 1, np.uint64) for _ in range(3)]
        args = dict(db=dbh or db.handle, r=rset._h, row=L.ptr(row), parent=L.ptr(parent), clades=L.ptr(cl), out=out)
        if skip:
            args[skip] = None
        rc = L.lib().ss_reads_select_class(args["db"], args["r"], args["row"], n_nodes, args["parent"], m, args["clades"], nc, args["out"],
                                           *([L.ptr(b) for b in bufs] if counts else [None] * 3))
        return rc, list(out), bufs

    def close(handles):
        for h in handles:
            L.check(L.lib().ss_reads_destroy(C.c_void_p(h)), "ss_reads_destroy")

    calls, ccalls = L.select_class_calls(), L.classify_calls()
    rc, out, _ = raw()
    assert rc == 0 and all(h and h != junk for h in out)
    close(out)
    assert L.select_class_calls() == calls + 1
    rc, out, bufs = raw(counts=True)                                       # with the counts: classify()'s
    assert rc == 0
    close(out)
    ref = rset.classify(db, row_node, par, 1)
    assert (bufs[0] == ref["direct"]).all() and (bufs[1] == ref["node_hits"]).all() and (bufs[2] == ref["kmers"]).all()
    ccalls += 1

    def refused(want, **kw):
        rc, out, _ = raw(**kw)
        assert rc == want, (kw, rc)
        return out

    for skip in ("db", "r", "row", "parent", "clades"):
        assert refused(L.SS_EINVAL, skip=skip) == [None, None], skip       # after an error every out[i] is NULL
    refused(L.SS_EINVAL, skip="out")
    assert refused(L.SS_EINVAL, m=0) == [None, None]
    assert refused(L.SS_EINVAL, n_nodes=0, clades=(0, 0)) == [None, None]
    assert refused(L.SS_EINVAL, n_nodes=100, clades=(0, 41)) == [None, None]                # a row node above n_nodes
    assert refused(L.SS_EINVAL, clades=(0, n + 1)) == [None, None]                         # a clade above n_nodes
    assert refused(L.SS_EINVAL, clades=(n + 1, 0)) == [None, None]
    refused(L.SS_EINVAL, n_clades=0)
    refused(L.SS_EINVAL, clades=[0] * (L.CLASS_CLADES_MAX + 1))
    rc, out, _ = raw(clades=[41] * L.CLASS_CLADES_MAX)                                      # the cap itself is served
    assert rc == 0 and len(set(out)) == L.CLASS_CLADES_MAX and all(out)
    close(out)
    for at, to in ((7, n + 1), (300, 300), (40, 1)):                                        # a parent above n_nodes, a self loop, a ring
        bad = par.copy()
        bad[at] = to
        assert refused(L.SS_EINVAL, parent=bad) == [None, None], (at, to)
    with pytest.raises(L.SSError) as e:
        rset.select_class(db, row_node, par, 1, [])
    assert e.value.code == L.SS_EINVAL
    with pytest.raises(ValueError):
        rset.select_class(db, row_node[:-1], par, 1, [0])
    k15m = list(dict.fromkeys(g[i:i + 15] for i in range(0, 5000, 5)))
    k15 = L.KmerDB.from_text(cc.kfa(k15m), 15, True)
    try:
        assert refused(L.SS_ERANGE, dbh=k15.handle, row=np.ones(len(k15m), np.uint32), parent=np.zeros(2, np.uint32), n_nodes=1,
                       clades=(0, 1)) == [None, None]                                         # a flat table
    finally:
        k15.close()
    assert L.classify_calls() == ccalls                                                       # none of this was an ss_reads_classify
