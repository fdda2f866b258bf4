"""ss_reads_calls (ss_calls.hip) and ss_reads_load_ordered (ss_pairs.hip): the class, the best score and the hit list of every
record of a resident set, held entry for entry to tests/read_calls_model.py for every (table, block, M) below.  The inputs are
class_cases' and read_calls_cases'; tests/test_read_calls_host.py checks on the model that the cases this is about are among
them (lists of 0, 7, 8, 9 and 16 and more nodes, an entry above 65535, a long record with a short list, ties, lists without a
class).

Not covered here: the SS_ERANGE of a cut record and of more records than an int holds (as tests/test_classify_gpu.py says)."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from tests import class_cases as cc, class_model as cm, read_calls_cases as rcc, read_calls_model as rcm

pytestmark = pytest.mark.gpu

MS = (1, 3)
KEYS = ("classes", "scores", "first", "list_node", "list_hits")


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


def _fastq_gz(path, reads, seed):
    rs = np.random.RandomState(seed)
    qa = np.frombuffer(b"0123456789BCDEFGHIJ", np.uint8)
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, qa[rs.randint(0, qa.size, size=len(r))].tobytes()) for i, r in enumerate(reads))
    with open(path, "wb") as f:
        f.write(gzip.compress(text, 1))
    assert os.path.getsize(path) >= 1 << 20
    return text


FILE_ORDER = ["ragged_0", "ragged_1", "ragged_1023", "one_length", "repeat"]
LAYOUTS = ["packed", "binned_ascii", "two_slabs"]


@pytest.fixture(scope="module")
def read_sets(L, g, tmp_path_factory):
    """name -> (ReadSet, its bytes read back); gz_texts: the texts of the two .fastq.gz files of two_slabs, and their paths"""
    import torch
    keep, out = [], {}

    def flat(block, order):
        d = torch.frombuffer(bytearray(block or b"\n"), dtype=torch.uint8).cuda()
        keep.append(d)
        rset = L.ReadSet.from_flat_dev(d.data_ptr(), len(block), order=order)
        L.check(L.lib().ss_device_sync(), "sync")
        return rset

    blocks = rcc.blocks(g)
    for name in FILE_ORDER:
        out[name] = flat(blocks[name], False)
        assert out[name].packed_slabs() == 0
    out["packed"] = flat(blocks["one_length"], True)
    assert out["packed"].packed_slabs() == 1
    out["binned_ascii"] = flat(cc.one_length_block(g, lower=True), True)
    assert out["binned_ascii"].packed_slabs() == 0
    out["empty"] = flat(b"", False)
    out["one_base"] = flat(b"A\n", False)
    out["many_nodes_alone"] = flat(b"".join(g[j * cc.STRETCH + 20:j * cc.STRETCH + 65] for j in range(3, 19)) + b"\n", False)
    rs = np.random.RandomState(13)
    root = str(tmp_path_factory.mktemp("calls_gz"))
    paths, texts = [], []
    for m in range(2):
        reads = [g[s:s + 1000] for s in rs.randint(0, len(g) - 1000, size=1250)]
        paths.append(os.path.join(root, "r%d.fastq.gz" % (m + 1)))
        texts.append(_fastq_gz(paths[-1], reads, 100 + m))
    out["two_slabs"] = L.ReadSet(paths)
    assert out["two_slabs"].info()["n_blocks"] >= 2
    sets = {name: (r, r.read_back()) for name, r in out.items()}
    sets["gz_texts"] = (paths, texts)
    yield sets
    for r in out.values():
        r.close()


_DONE = {}


def _called(L, tables, read_sets, tname, sname):
    """{m: (device dict, model dict)} of one (table, set), computed once"""
    if (tname, sname) not in _DONE:
        db, k, keys, row_node = tables[tname]
        rset, text = read_sets[sname]
        par = cc.parents()
        per, _ = cm.record_hits(text, keys, row_node, k)
        res = {}
        for m in MS:
            before = L.read_calls_calls()
            got = rset.calls(db, row_node, par, m)
            assert L.read_calls_calls() > before
            res[m] = (got, rcm.calls_model(text, keys, row_node, par, k, m, per))
        _DONE[tname, sname] = res
    return _DONE[tname, sname]


def _by_record(text, calls):
    """sorted [(record bytes, class, score, list)]: what a set says of its records, whatever their order"""
    recs = [r for r in text.split(b"\n") if r]
    assert len(recs) == len(calls["classes"])
    first = [int(x) for x in calls["first"]]
    return sorted((r, int(calls["classes"][i]), int(calls["scores"][i]),
                   tuple(zip(calls["list_node"][first[i]:first[i + 1]].tolist(), calls["list_hits"][first[i]:first[i + 1]].tolist())))
                  for i, r in enumerate(recs))


@pytest.mark.parametrize("sname", FILE_ORDER + LAYOUTS + ["empty", "one_base", "many_nodes_alone"])
@pytest.mark.parametrize("tname", list(cc.TABLES))
def test_calls_equal_the_model(L, tables, read_sets, tname, sname):
    for m, (got, want) in _called(L, tables, read_sets, tname, sname).items():
        print(tname, sname, "M", m, "records", got["classes"].size, "entries", got["list_node"].size, "classified", int((got["classes"] != 0).sum()),
              "largest entry", int(got["list_hits"].max()) if got["list_hits"].size else 0)
        assert got["classes"].dtype == got["scores"].dtype == got["list_node"].dtype == got["list_hits"].dtype == np.uint32
        assert got["first"].dtype == np.uint64
        for key in KEYS:
            assert got[key].shape == want[key].shape and (got[key] == want[key]).all(), (m, key)
        assert got["ties"] == want["ties"]
    if sname == "many_nodes_alone":
        assert got["classes"].size == 1 and got["list_node"].size == 16
    if sname == "one_base":
        assert got["classes"].tolist() == [0] and got["first"].tolist() == [0, 0]
    if sname == "empty":
        assert got["classes"].size == 0 and got["first"].tolist() == [0]


@pytest.mark.parametrize("tname", list(cc.TABLES))
def test_layouts_agree(L, tables, read_sets, tname):
    """packed, file order and (but for its one lower-case base) binned ASCII hold the same reads: the same calls per read"""
    for m in MS:
        a = _by_record(read_sets["one_length"][1], _called(L, tables, read_sets, tname, "one_length")[m][0])
        b = _by_record(read_sets["packed"][1], _called(L, tables, read_sets, tname, "packed")[m][0])
        assert a == b
        c = _by_record(read_sets["binned_ascii"][1].upper(), _called(L, tables, read_sets, tname, "binned_ascii")[m][0])
        assert a == c
        # two slabs: record numbers run on across the slabs
        got, want = _called(L, tables, read_sets, tname, "two_slabs")[m]
        assert _by_record(read_sets["two_slabs"][1], got) == _by_record(read_sets["two_slabs"][1], want) and got["classes"].size == 2500


@pytest.mark.parametrize("sname", ["ragged_1", "repeat", "packed", "two_slabs"])
@pytest.mark.parametrize("tname", list(cc.TABLES))
def test_invariants_and_the_counts_of_classify(L, tables, read_sets, tname, sname):
    db, _, _, row_node = tables[tname]
    rset, _ = read_sets[sname]
    par = cc.parents()
    for m in MS:
        got = _called(L, tables, read_sets, tname, sname)[m][0]
        assert int(got["first"][-1]) == got["list_node"].size == got["list_hits"].size and int(got["first"][0]) == 0
        assert (np.diff(got["first"].astype(np.int64)) >= 0).all()
        assert (np.bincount(got["classes"], minlength=cc.N_NODES + 1).astype(np.uint64) == got["direct"]).all()
        by_node = np.bincount(got["list_node"], weights=got["list_hits"].astype(np.float64), minlength=cc.N_NODES + 1).astype(np.uint64)
        assert (by_node[1:] == got["node_hits"][1:]).all() and by_node[0] == 0
        calls_before, classify_before = L.read_calls_calls(), L.classify_calls()
        ref = rset.classify(db, row_node, par, m, want_classes=True)
        assert L.read_calls_calls() == calls_before and L.classify_calls() == classify_before + 1      # (each call counts its own)
        for key in ("direct", "node_hits", "kmers"):
            assert (got[key] == ref[key]).all(), key
        assert got["ties"] == ref["ties"] and (got["classes"] == ref["classes"]).all()
        assert (got["scores"][got["classes"] != 0] >= m).all()
        empty = np.diff(got["first"].astype(np.int64)) == 0
        assert (got["scores"][empty] == 0).all() and (got["scores"][~empty] > 0).all()


def _raw(L, db, rset, row_node, par, m, n_rec, cap, skip=None, n_nodes=cc.N_NODES):
    """the C call itself -> (rc, n_list, arrays); skip: the argument passed as NULL"""
    a = dict(classes=np.zeros(n_rec + 1, np.uint32), scores=np.zeros(n_rec + 1, np.uint32), first=np.zeros(n_rec + 2, np.uint64),
             list_node=np.zeros(max(cap, 1), np.uint32), list_hits=np.zeros(max(cap, 1), np.uint32))
    n_list = C.c_uint64(12345)
    args = dict(db=db.handle, r=rset._h, row=L.ptr(row_node), parent=L.ptr(par), classes=L.ptr(a["classes"]), scores=L.ptr(a["scores"]),
                first=L.ptr(a["first"]), list_node=L.ptr(a["list_node"]) if cap else None, list_hits=L.ptr(a["list_hits"]) if cap else None,
                n_list=C.byref(n_list))
    if skip:
        args[skip] = None
    rc = L.lib().ss_reads_calls(args["db"], args["r"], args["row"], n_nodes, args["parent"], m, args["classes"], args["scores"], args["first"],
                                args["list_node"], args["list_hits"], cap, args["n_list"], None, None, None)
    return rc, int(n_list.value), a


def test_capacity(L, tables, read_sets):
    db, _, _, row_node = tables["k31_dense"]
    par = cc.parents()
    for sname in ("ragged_1", "two_slabs"):
        rset, _ = read_sets[sname]
        want = _called(L, tables, read_sets, "k31_dense", sname)[1][0]
        n_rec, n_list = want["classes"].size, want["list_node"].size
        assert n_list > n_rec
        rc, n, _ = _raw(L, db, rset, row_node, par, 1, n_rec, 0)                      # no lists: how many entries there are
        assert rc == L.SS_ERANGE and n == n_list
        rc, n, a = _raw(L, db, rset, row_node, par, 1, n_rec, n_list)                 # ... and the call that brings room for them
        assert rc == 0 and n == n_list
        for key in KEYS:
            assert (a[key][:want[key].size] == want[key]).all(), key
        rc, n, _ = _raw(L, db, rset, row_node, par, 1, n_rec, n_list - 1)             # one entry short
        assert rc == L.SS_ERANGE and n == n_list
        rc, n, a = _raw(L, db, rset, row_node, par, 1, n_rec, n_list + 1000)          # more room than needed
        assert rc == 0 and n == n_list and (a["list_hits"][:n_list] == want["list_hits"]).all()
        with pytest.raises(L.SSError) as e:
            rset.calls(db, row_node, par, 1, cap=5)
        assert e.value.code == L.SS_ERANGE and e.value.n_list == n_list
    # a set without a listed node needs no room
    rset, _ = read_sets["one_base"]
    rc, n, a = _raw(L, db, rset, row_node, par, 1, 1, 0)
    assert rc == 0 and n == 0 and a["first"][:2].tolist() == [0, 0]
    rset, _ = read_sets["empty"]
    rc, n, a = _raw(L, db, rset, row_node, par, 1, 0, 0)
    assert rc == 0 and n == 0 and a["first"][0] == 0


def test_argument_errors(L, tables, read_sets):
    db, _, _, row_node = tables["k25"]
    rset, _ = read_sets["ragged_1"]
    par = cc.parents()
    n_rec = _called(L, tables, read_sets, "k25", "ragged_1")[1][0]["classes"].size
    before = L.read_calls_calls()
    for skip in ("db", "r", "row", "parent", "classes", "scores", "first", "n_list"):
        assert _raw(L, db, rset, row_node, par, 1, n_rec, 100000, skip=skip)[0] == L.SS_EINVAL, skip
    assert _raw(L, db, rset, row_node, par, 1, n_rec, 100000, skip="list_node")[0] == L.SS_EINVAL      # room without a list
    assert _raw(L, db, rset, row_node, par, 1, n_rec, 100000, skip="list_hits")[0] == L.SS_EINVAL
    assert _raw(L, db, rset, row_node, par, 0, n_rec, 100000)[0] == L.SS_EINVAL                        # min_score == 0
    assert _raw(L, db, rset, row_node, par, 1, n_rec, 100000, n_nodes=0)[0] == L.SS_EINVAL
    assert _raw(L, db, rset, row_node, par, 1, n_rec, 100000, n_nodes=100)[0] == L.SS_EINVAL           # a row node above n_nodes
    bad = par.copy()
    bad[40] = 1
    assert _raw(L, db, rset, row_node, bad, 1, n_rec, 100000)[0] == L.SS_EINVAL                        # the chain closed to a ring
    assert L.read_calls_calls() == before                                                              # (none of them ran)
    with pytest.raises(ValueError):
        rset.calls(db, row_node[:-1], par, 1)


# ---------------------------------------------------------------------------------------------- ss_reads_load_ordered


def _is_flat(rb, flat):
    return rb[:len(flat)] == flat and set(rb[len(flat):]) <= {10}


def test_load_ordered(L, g, read_sets, tmp_path):
    rs = np.random.RandomState(41)
    qa = np.frombuffer(b"#+5678ABCDEFGHIJ", np.uint8)

    def wrap(s, w, eol):
        return b"".join(s[i:i + w] + eol for i in range(0, len(s), w))

    reads = [g[s:s + int(n)] for s, n in zip(rs.randint(0, len(g) - 400, size=300), rs.randint(1, 400, size=300))]
    quals = [qa[rs.randint(0, qa.size, size=len(r))].tobytes() for r in reads]
    texts = {
        "four_line.fq": b"@e0\n\n+\n\n" + b"".join(b"@r%d x\n%s\n+\n%s\n" % (i, r, q) for i, (r, q) in enumerate(zip(reads, quals))),
        "wrapped.fq": b"".join(b"@r%d\n" % i + wrap(r, 60, b"\n") + b"+\n" + wrap(q, 60, b"\n") for i, (r, q) in enumerate(zip(reads, quals))),
        "wrapped.fa": b"".join(b">r%d\n" % i + wrap(r, 70, b"\n") for i, r in enumerate(reads)),
        "crlf.fq": b"".join(b"@r%d\r\n%s\r\n+\r\n%s\r\n" % (i, r, q) for i, (r, q) in enumerate(zip(reads, quals))),
    }
    for q in (0, 20):
        L.set_min_base_qual(q)
        try:
            for name, text in texts.items():
                flat, _ = L.fastx_to_flat(text)
                for gz in (False, True):
                    p = tmp_path / (name + (".gz" if gz else ""))
                    p.write_bytes(gzip.compress(text, 6) if gz else text)
                    rset = L.ReadSet.load_ordered(str(p))
                    try:
                        assert _is_flat(rset.read_back(), flat), (name, gz, q)
                        assert rset.packed_slabs() == 0 and rset.info()["n_blocks"] <= 1
                    finally:
                        rset.close()
            if q:
                assert b"N" in L.fastx_to_flat(texts["four_line.fq"])[0].replace(b"\n", b"")[:2000]      # (the mask did something)
        finally:
            L.set_min_base_qual(0)
    # files of 1 MB and more of .gz, which the device may inflate: the same block
    for path, text in zip(*read_sets["gz_texts"]):
        rset = L.ReadSet.load_ordered(path)
        try:
            assert _is_flat(rset.read_back(), L.fastx_to_flat(text)[0])
        finally:
            rset.close()
    from tests import bamio
    bam = tmp_path / "x.bam"
    bam.write_bytes(bamio.bgzf(bamio.header(), [bamio.record("q", "ACGTACGT")], level=6))
    for bad, code in ((str(bam), L.SS_EINVAL), ("", L.SS_EINVAL), (str(tmp_path / "missing.fq"), L.SS_EIO)):
        with pytest.raises(L.SSError) as e:
            L.ReadSet.load_ordered(bad)
        assert e.value.code == code, bad
    h = C.c_void_p()
    assert L.lib().ss_reads_load_ordered(None, C.byref(h)) == L.SS_EINVAL and L.lib().ss_reads_load_ordered(b"x", None) == L.SS_EINVAL


def test_a_file_classified_in_file_order_and_written(L, g, tables, tmp_path):
    """the three calls together, as the command uses them: load_ordered, calls, read_calls_write -> the model's table"""
    db, k, keys, row_node = tables["k31_dense"]
    par = cc.parents()
    lines = rcc.blocks(g)["ragged_1"].split(b"\n")[:400]
    text = b"".join(b"@read%d/1 extra\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(lines))
    p = tmp_path / "in.fq"
    p.write_bytes(text)
    node_value = np.array([-1] + [1000 + v for v in range(1, cc.N_NODES + 1)], np.int64)
    with_seq = sum(1 for r in lines if r)
    rset = L.ReadSet.load_ordered(str(p))
    try:
        got = rset.calls(db, row_node, par, 3)
    finally:
        rset.close()
    want = rcm.calls_model(L.fastx_to_flat(text)[0], keys, row_node, par, k, 3)
    for key in KEYS:
        assert (got[key] == want[key]).all(), key
    c = L.read_calls_write([str(p)], [str(tmp_path / "calls.tsv")], got, node_value)
    assert (tmp_path / "calls.tsv").read_bytes() == rcm.table_text([text], want, node_value)[0]
    assert c["read"] == 400 and c["empty"] == 400 - with_seq and c["classified"] == int((want["classes"] != 0).sum()) > 100
