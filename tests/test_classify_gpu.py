"""ss_reads_classify (ss_classify.hip, scan_minik_kernel's ClassSink): every record of a resident set assigned to a node of a
forest over the table's k-mers, held bit for bit to tests/class_model.py for every (table, read set, M) below; the inputs are
those of tests/class_cases.py, whose conditions against a vacuous pass tests/test_classify_host.py checks on the model.

Not covered here: the SS_ERANGE of a cut record (a cut record needs a record longer than a 32 MB block) and of more records than
an int holds; the SS_EINVAL of a table and a set on different devices (one device)."""
import gzip
import os

import numpy as np
import pytest

from tests import class_cases as cc, class_model as cm, label_model

pytestmark = pytest.mark.gpu

MS = (1, 2, 8)


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
        assert db.n_rows == len(kmers) and db.info()["n_distinct"] == len(kmers) - 1
        if expect:
            db.expect_hits(True)
        out[name] = (db, k, keys, row_node)
    yield out
    for db, _, _, _ in out.values():
        db.close()


def _fastq_gz(path, reads, seed):
    rs = np.random.RandomState(seed)
    qa = np.frombuffer(b"0123456789BCDEFGHIJ", np.uint8)
    out = [b"@r%d\n%s\n+\n%s\n" % (i, r, qa[rs.randint(0, qa.size, size=len(r))].tobytes()) for i, r in enumerate(reads)]
    with open(path, "wb") as f:
        f.write(gzip.compress(b"".join(out), 1))
    assert os.path.getsize(path) >= 1 << 20
    return path


SETS = ["packed", "file_order", "binned_ascii", "ragged_0", "ragged_1", "ragged_1023", "two_slabs", "half_a", "half_b", "empty"]


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
    # two .fastq.gz files of 1 MB and more: the device path gives each a slab of its own, and record indices run on across slabs
    rs = np.random.RandomState(13)
    root = str(tmp_path_factory.mktemp("cls_gz"))
    paths = []
    for m in range(2):
        reads = [g[s:s + 1000] for s in rs.randint(0, len(g) - 1000, size=1250)]
        paths.append(_fastq_gz(os.path.join(root, "r%d.fastq.gz" % (m + 1)), reads, 100 + m))
    out["two_slabs"] = L.ReadSet(paths)
    assert out["two_slabs"].info()["n_blocks"] >= 2
    sets = {name: (r, r.read_back()) for name, r in out.items()}
    yield sets
    for r in out.values():
        r.close()


_DONE = {}


def _classified(L, tables, read_sets, tname, sname):
    """the device's and the model's results of one (table, set) at every M, computed once: {m: (device dict, model triple, model classes)}"""
    if (tname, sname) in _DONE:
        return _DONE[tname, sname]
    db, k, keys, row_node = tables[tname]
    rset, text = read_sets[sname]
    par = cc.parents()
    per, n_rec = cm.record_hits(text, keys, row_node, k)
    res = {}
    for m in MS:
        calls = L.classify_calls()
        got = rset.classify(db, row_node, par, m, want_classes=True)
        assert L.classify_calls() == calls + 1
        want = cm.classify_model(text, keys, row_node, par, cc.N_NODES, k, m, per)
        det = cm.classes_detail(text, keys, row_node, par, k, m, per)
        res[m] = (got, want, det, n_rec)
    _DONE[tname, sname] = res
    return res


@pytest.mark.parametrize("sname", SETS)
@pytest.mark.parametrize("tname", list(cc.TABLES))
def test_classes_equal_the_model(L, tables, read_sets, tname, sname):
    for m, (got, want, det, n_rec) in _classified(L, tables, read_sets, tname, sname).items():
        ties = sum(1 for d in det if d[2])
        print(tname, sname, "M", m, "records", n_rec, "classified", n_rec - int(got["direct"][0]), "ties", got["ties"], "model ties", ties,
              "hits", int(got["node_hits"].sum()), "nodes with reads", int((got["direct"][1:] > 0).sum()))
        assert got["direct"].dtype == np.uint64 and got["direct"].shape == (cc.N_NODES + 1,)
        assert (got["kmers"] == want[2]).all()
        assert (got["node_hits"] == want[1]).all()
        assert (got["direct"] == want[0]).all()
        assert int(got["direct"].sum()) == n_rec
        assert got["classes"].dtype == np.uint32 and got["classes"].tolist() == [d[0] for d in det]
        assert got["ties"] == ties
    if sname != "empty":
        assert int(got["kmers"][121]) == 0 and int(got["kmers"][300]) == 0


@pytest.mark.parametrize("tname", list(cc.TABLES))
def test_layouts_agree_and_halves_add_up(L, tables, read_sets, tname):
    r = {s: _classified(L, tables, read_sets, tname, s) for s in ("packed", "file_order", "binned_ascii", "half_a", "half_b")}
    for m in MS:
        a, b, c = (r[s][m][0] for s in ("packed", "file_order", "binned_ascii"))
        assert (a["direct"] == b["direct"]).all() and (a["direct"] == c["direct"]).all()
        assert (a["node_hits"] == b["node_hits"]).all() and (a["node_hits"] == c["node_hits"]).all()
        assert a["ties"] == b["ties"] == c["ties"]
        ha, hb = r["half_a"][m][0], r["half_b"][m][0]
        assert (ha["direct"] + hb["direct"] == a["direct"]).all()
        assert (ha["node_hits"] + hb["node_hits"] == a["node_hits"]).all()
        assert (ha["kmers"] == a["kmers"]).all()
    # more nodes than a workgroup adds up in LDS (the further ones roots without rows): the same numbers, from global atomics
    wide_par = np.zeros(5001, np.uint32)
    wide_par[:cc.N_NODES + 1] = cc.parents()
    db, _, _, row_node = tables[tname]
    for s in ("packed", "binned_ascii"):
        wide = read_sets[s][0].classify(db, row_node, wide_par, 2, want_classes=True)
        for key in ("direct", "node_hits", "kmers"):
            assert (wide[key][:cc.N_NODES + 1] == r[s][2][0][key]).all() and not wide[key][cc.N_NODES + 1:].any(), (s, key)
        assert (wide["classes"] == r[s][2][0]["classes"]).all() and wide["ties"] == r[s][2][0]["ties"]
    # without the classes: the same numbers
    plain = read_sets["packed"][0].classify(db, row_node, cc.parents(), 1)
    assert plain["classes"] is None and (plain["direct"] == r["packed"][1][0]["direct"]).all()


@pytest.mark.parametrize("sname", ["packed", "ragged_1", "two_slabs"])
@pytest.mark.parametrize("tname", list(cc.TABLES))
def test_node_hits_against_support_labels_and_a_scan(L, tables, read_sets, tname, sname):
    db, k, keys, row_node = tables[tname]
    rset, text = read_sets[sname]
    got = _classified(L, tables, read_sets, tname, sname)[1][0]
    # the hits of all nodes and of no node: ss_reads_support's hits
    _, total = rset.support(db)
    assert int(got["node_hits"].sum()) == total
    # folded onto 15 labels: ss_reads_support_labeled's hits, and the model's
    lab = cc.relabel15(row_node)
    folded = rset.classify(db, lab.astype(np.uint32), np.zeros(16, np.uint32), 1)
    _, hits15, kmers15 = rset.support_labeled(db, lab, 15)
    per15 = label_model.labeled_hits_per_record(text, keys, lab, 15, k)
    assert folded["node_hits"][1:].tolist() == hits15.tolist() == per15[1:].sum(axis=1).tolist()
    assert int(folded["node_hits"][0]) == int(per15[0].sum())
    assert folded["kmers"][1:].tolist() == kmers15.tolist()
    # a real scan of the set: the counters of v's slots, one row per slot; and the call leaves them as they are
    db.reset()
    rset.scan_into(db)
    L.check(L.lib().ss_device_sync(), "sync")
    before = db.counts_rows().copy()
    again = rset.classify(db, row_node, cc.parents(), 2)
    assert (db.counts_rows() == before).all()
    assert (again["node_hits"] == got["node_hits"]).all()
    # (of the rows that list one k-mer, counts_rows shows the slot's count at the one that match_results keeps: the largest)
    order = np.argsort(keys, kind="stable")
    starts = np.nonzero(np.concatenate(([True], keys[order][1:] != keys[order][:-1])))[0]
    per_slot = np.maximum.reduceat(before[order], starts)
    uk, un = cm.kmer_nodes(keys, row_node)
    assert (uk == keys[order][starts]).all()
    by_node = np.bincount(un, weights=per_slot.astype(np.float64), minlength=cc.N_NODES + 1).astype(np.uint64)
    print(tname, sname, "scan counts", int(per_slot.sum()), "node hits", int(got["node_hits"].sum()), "without a node", int(got["node_hits"][0]))
    assert int(per_slot.sum()) > 0 and int(got["node_hits"][0]) > 0
    assert (by_node == got["node_hits"]).all()
    db.reset()


def test_argument_errors(L, g, tables, read_sets):
    rset = read_sets["packed"][0]
    db, _, _, row_node = tables["k25"]
    par = cc.parents()
    n = cc.N_NODES

    def code(fn):
        with pytest.raises(L.SSError) as e:
            fn()
        return e.value.code

    def raw(row=row_node, parent=par, n_nodes=n, m=1, skip=None):
        """the C call itself; skip: the argument passed as NULL"""
        bufs = [np.zeros(n_nodes + 1, np.uint64) for _ in range(3)]
        args = dict(db=db.handle, r=rset._h, row=L.ptr(row), parent=L.ptr(parent), direct=L.ptr(bufs[0]), hits=L.ptr(bufs[1]), kmers=L.ptr(bufs[2]))
        if skip:
            args[skip] = None
        return L.lib().ss_reads_classify(args["db"], args["r"], args["row"], n_nodes, args["parent"], m, args["direct"], args["hits"],
                                         args["kmers"], None)

    calls = L.classify_calls()
    assert raw() == 0
    assert L.classify_calls() == calls + 1
    for skip in ("db", "r", "row", "parent", "direct", "hits", "kmers"):
        assert raw(skip=skip) == L.SS_EINVAL, skip
    assert raw(m=0) == L.SS_EINVAL
    assert code(lambda: rset.classify(db, row_node, par, 0)) == L.SS_EINVAL
    assert raw(n_nodes=0) == L.SS_EINVAL
    big = np.zeros(L.CLASS_NODES_MAX + 2, np.uint32)
    assert raw(parent=big, n_nodes=L.CLASS_NODES_MAX + 1) == L.SS_EINVAL
    assert raw(parent=big, n_nodes=L.CLASS_NODES_MAX) == 0                                # the cap itself is served
    assert raw(n_nodes=100) == L.SS_EINVAL                                                # a row node above n_nodes
    bad = par.copy()
    bad[7] = n + 1
    assert code(lambda: rset.classify(db, row_node, bad, 1)) == L.SS_EINVAL               # a parent above n_nodes
    bad = par.copy()
    bad[300] = 300
    assert code(lambda: rset.classify(db, row_node, bad, 1)) == L.SS_EINVAL               # a node that is its own parent
    bad = par.copy()
    bad[40] = 1
    assert code(lambda: rset.classify(db, row_node, bad, 1)) == L.SS_EINVAL               # the chain closed to a ring
    bad = par.copy()
    bad[282], bad[283], bad[284] = 283, 284, 282
    assert code(lambda: rset.classify(db, row_node, bad, 1)) == L.SS_EINVAL               # a ring that no root reaches
    with pytest.raises(ValueError):
        rset.classify(db, row_node[:-1], par, 1)
    k15m = list(dict.fromkeys(g[i:i + 15] for i in range(0, 5000, 5)))
    k15 = L.KmerDB.from_text(cc.kfa(k15m), 15, True)
    try:
        assert code(lambda: rset.classify(k15, np.ones(len(k15m), np.uint32), np.zeros(2, np.uint32), 1)) == L.SS_ERANGE      # a flat table
    finally:
        k15.close()
    assert L.classify_calls() == calls + 2
