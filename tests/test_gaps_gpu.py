"""ss_reads_gaps (ss_gaps.hip; scan_minik_kernel's ClassSink with C / T slot values, then gap_walk_kernel): the runs of missing k-mers
inside every record, held integer for integer to tests/gap_model.py -- the totals and the per-record rows -- for every (table,
called rows, read set) below.  The inputs are those of tests/gap_cases.py, whose conditions against a vacuous pass
tests/test_gaps_host.py checks on the model.

Not covered here: the SS_ERANGE of a cut record (a cut record needs a record longer than a 32 MB block); the SS_EINVAL of a table
and a set on different devices (one device)."""
import numpy as np
import pytest

from tests import gap_cases as gc, gap_model as gm

pytestmark = pytest.mark.gpu

TABLES = ("k31", "k21")
HOWS = ("all", "half")
SETS = ("mixed_file", "mixed_binned", "one_file", "one_packed", "hand", "tile_edges", "long", "empty", "n1", "n63", "n64", "n65", "n257", "shard_a",
        "shard_b")


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def g():
    return gc.genome()


@pytest.fixture(scope="module")
def tables(L, g):
    """name -> (KmerDB, k, kmers, keys of the rows with a slot, their starts)"""
    out = {}
    for name in TABLES:
        k, kmers, keys, starts = gc.table(name, g)
        db = L.KmerDB.from_text(gc.kfa(kmers), k, True)
        assert db.n_rows == len(kmers)
        out[name] = (db, k, kmers, keys, starts)
    yield out
    for t in out.values():
        t[0].close()


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

    mixed, one = gc.mixed_reads(g), gc.one_length_reads(g)
    out["mixed_file"] = flat(gc.block(mixed), False)
    out["mixed_binned"] = flat(gc.block(mixed), True)
    out["one_file"] = flat(gc.block(one), False)
    out["one_packed"] = flat(gc.block(one), True)
    assert out["one_packed"].packed_slabs() >= 1
    assert out["mixed_binned"].packed_slabs() == 0 and out["mixed_file"].packed_slabs() == 0 and out["one_file"].packed_slabs() == 0
    recs = [r for r, _ in gc.hand_records(g).values()] + [gc.in_cluster_case(g)[0]]
    out["hand"] = flat(gc.block(recs), False)
    out["tile_edges"] = flat(gc.tile_edge_block(g), False)
    out["long"] = flat(gc.block(gc.long_records(g)), False)
    out["empty"] = flat(b"", False)
    for n in (1, 63, 64, 65, 257):
        out["n%d" % n] = flat(gc.block(one[:n]), False)
    out["shard_a"] = flat(gc.block(mixed[:140]), False)
    out["shard_b"] = flat(gc.block(mixed[140:]), True)
    sets = {name: (r, r.read_back()) for name, r in out.items()}
    assert sets["tile_edges"][1].rstrip(b"\n") == gc.tile_edge_block(g).rstrip(b"\n")      # (positions are the block's byte offsets)
    yield sets
    for r in out.values():
        r.close()


_DONE = {}


def _gaps(L, tables, read_sets, tname, how, sname, m):
    """(the device's totals, its rows, the model's totals, its rows) of one case, computed once"""
    key = (tname, how, sname, m)
    if key not in _DONE:
        db, k, kmers, keys, starts = tables[tname]
        full, called = gc.called_rows(tname, kmers, starts, how)
        rset, text = read_sets[sname]
        calls = L.gaps_calls()
        got, rec = rset.gaps(db, full, m, want_records=True)
        assert L.gaps_calls() == calls + 1
        want, wrec = gm.gaps_model(text, keys, called, k, m)
        _DONE[key] = (got, rec, want, wrec)
    return _DONE[key]


@pytest.mark.parametrize("sname", SETS)
@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("tname", TABLES)
def test_gaps_equal_the_model(L, tables, read_sets, tname, how, sname):
    for m in (1, 12):
        got, rec, want, wrec = _gaps(L, tables, read_sets, tname, how, sname, m)
        print(tname, how, sname, "M", m, got)
        assert got == want
        assert rec.dtype == np.uint32 and rec.shape == wrec.shape and (rec == wrec).all(), np.nonzero((rec != wrec).any(axis=1))[0][:10]
        assert got["windows"] == got["hits_called"] + got["hits_cluster"] + got["misses"]
        assert got["sites"] <= got["gap_km1"] + got["gap_k"] + got["gap_k_2k"] and got["reads_with_sites"] <= got["sites"]
    if sname == "long":
        assert got["long_records"] == 2 and got["records"] == 2 and int(rec[1, 0]) > 4 * 4095      # (far more than the per-lane pass takes)
    if sname == "tile_edges" and tname == "k31" and how == "all":
        assert got["gap_k"] == got["sites"] == 3
    if sname == "hand" and tname == "k31" and how == "all":
        names = list(gc.hand_records(g=gc.genome()))
        assert rec[names.index("clean")].tolist() == [120, 0, 0, 88] and rec[names.index("sub_75")].tolist() == [89, 1, 1, 88]
        assert rec[names.index("short")].tolist() == [0, 0, 0, 0] and rec[names.index("exactly_k")].tolist() == [1, 0, 0, 0]


def test_a_run_of_uncalled_kmers_on_the_device(L, g, tables, read_sets):
    db, k, kmers, keys, starts = tables["k31"]
    _, uncalled = gc.in_cluster_case(g)
    called = np.array([s not in uncalled for s in starts], np.uint8)
    rset, text = read_sets["hand"]
    got, rec = rset.gaps(db, called, 1, want_records=True)
    want, wrec = gm.gaps_model(text, keys, called, k, 1)
    assert got == want and (rec == wrec).all()
    assert rec[-1].tolist() == [79, 1, 0, 88] and got["gaps_in_cluster"] >= 1 and got["kmers_called"] == len(kmers) - 82


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("tname", TABLES)
def test_layouts_agree_and_shards_add_up(L, tables, read_sets, tname, how):
    for m in (1, 12):
        a, b = (_gaps(L, tables, read_sets, tname, how, s, m)[0] for s in ("mixed_file", "mixed_binned"))
        assert a == b and a["sites"] > 0
        c, d = (_gaps(L, tables, read_sets, tname, how, s, m)[0] for s in ("one_file", "one_packed"))
        assert c == d and c["sites"] > 0
        sa, sb = (_gaps(L, tables, read_sets, tname, how, s, m)[0] for s in ("shard_a", "shard_b"))
        assert gm.add(sa, sb) == a
    # without the records: the same totals
    db, _, kmers, _, starts = tables[tname]
    full, _ = gc.called_rows(tname, kmers, starts, how)
    assert read_sets["one_packed"][0].gaps(db, full, 12) == d


@pytest.mark.parametrize("sname", ["n257", "one_packed", "mixed_binned"])
@pytest.mark.parametrize("tname", TABLES)
def test_hits_are_those_of_read_support(L, g, tables, read_sets, tname, sname):
    db = tables[tname][0]
    rset = read_sets[sname][0]
    got = _gaps(L, tables, read_sets, tname, "all", sname, 1)[0]
    _, hits = rset.support(db)
    db.reset()
    rset.scan_into(db)
    L.check(L.lib().ss_device_sync(), "sync")
    before = db.counts_rows().copy()
    again = rset.gaps(db, None, 1)
    assert (db.counts_rows() == before).all() and int(before.sum()) > 0      # the call leaves the table's counters alone
    db.reset()
    # every record with a hit is assessed at M = 1 when every row is called: the hits are all the set's hits
    assert again == got and got["hits_cluster"] == 0 and got["hits_called"] == int(hits) > 0
    db2, k, kmers, keys, starts = tables[tname]
    full, _ = gc.called_rows(tname, kmers, starts, "half")
    half, rec = rset.gaps(db2, full, 1, want_records=True)
    assert half["hits_cluster"] > 0
    if (rec[:, 0] > 0).all():
        assert half["hits_called"] + half["hits_cluster"] == int(hits)
    else:                                                                      # the records without a called hit keep theirs
        assert half["hits_called"] + half["hits_cluster"] < int(hits)


def test_argument_errors(L, g, tables, read_sets):
    rset = read_sets["one_packed"][0]
    db = tables["k21"][0]
    called = np.ones(db.n_rows, np.uint8)

    def raw(m=1, skip=None, rec=False):
        """the C call itself; skip: the argument passed as NULL"""
        out = np.zeros(L.GAPS_OUT, np.uint64)
        recs = np.zeros((600, 4), np.uint32)
        args = dict(db=db.handle, r=rset._h, row=L.ptr(called), out=L.ptr(out))
        if skip:
            args[skip] = None
        return L.lib().ss_reads_gaps(args["db"], args["r"], args["row"], m, args["out"], L.ptr(recs) if rec else None)

    calls = L.gaps_calls()
    assert raw() == 0 and raw(skip="row") == 0 and raw(rec=True) == 0
    assert L.gaps_calls() == calls + 3
    for skip in ("db", "r", "out"):
        assert raw(skip=skip) == L.SS_EINVAL, skip
    assert raw(m=0) == L.SS_EINVAL
    with pytest.raises(ValueError):
        rset.gaps(db, called[:-1], 1)
    assert L.gaps_calls() == calls + 3
    k15m = list(dict.fromkeys(g[i:i + 15] for i in range(0, 3000, 5)))
    k15 = L.KmerDB.from_text(gc.kfa(k15m), 15, True)
    try:
        with pytest.raises(L.SSError) as e:
            rset.gaps(k15, None, 1)                                             # a flat table
        assert e.value.code == L.SS_ERANGE
    finally:
        k15.close()
    assert L.gaps_calls() == calls + 3
