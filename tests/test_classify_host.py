"""--classify_reads on the host: the model (tests/class_model.py) on hand-worked cases, its invariants, the conditions that keep
tests/test_classify_gpu.py from passing vacuously (checked on the model for that test's inputs, tests/class_cases.py), the text of
read_classes.tsv, the flag and the idle hook.  What the device computes is tests/test_classify_gpu.py's."""
import argparse
import os
import types

import numpy as np
import pytest

from tests import class_cases as cc, class_model as cm, label_model, rs_model

# thirteen nodes in the shape of a built database's tree (leaves 1..7, inner nodes above them, root 13), and a second tree
#   13 -- 11 -- 9 -- 1, 2          14 -- 15
#      |     `- 10 -- 3, 4
#      `- 12 -- 5, 6, 7      (8 hangs under 12 as an inner node without leaves of its own)
PARENT = [0, 9, 9, 10, 10, 12, 12, 12, 12, 11, 11, 13, 13, 0, 0, 14]


def test_hand_worked_classes():
    c = lambda h, m=1: cm.classify_hits(h, PARENT, m)      # noqa: E731
    assert c({1: 5}) == (1, 5, False)                                   # hits on one leaf only
    assert c({1: 3, 9: 2, 11: 1}) == (1, 6, False)                      # a leaf and two of its ancestors: the path adds up
    assert c({9: 4, 1: 1}) == (1, 5, False)                             # (a node always beats its ancestors)
    assert c({1: 1, 2: 1}) == (9, 1, True)                              # sibling leaves: their parent, which has no hits
    assert c({1: 2, 3: 2}) == (11, 2, True)
    assert c({1: 2, 5: 2}) == (13, 2, True)                             # leaves whose lowest common ancestor is the root
    assert c({1: 2, 3: 2, 5: 2}) == (13, 2, True)
    assert c({1: 1, 15: 1}) == (0, 1, True)                             # tied nodes in two trees: nobody
    assert c({1: 2, 15: 1}) == (1, 2, False)
    assert c({1: 3}, 4) == (0, 3, False)                                # score M - 1
    assert c({1: 3}, 3) == (1, 3, False)
    assert c({1: 1, 2: 1}, 2) == (0, 1, False)                          # (a tie below M is no tie: unclassified)
    assert c({}) == (0, 0, False)
    assert cm.lca(PARENT, 1, 1) == 1 and cm.lca(PARENT, 1, 9) == 9 and cm.lca(PARENT, 4, 7) == 13 and cm.lca(PARENT, 7, 14) == 0
    assert cm.check_forest(PARENT, 15)
    assert not cm.check_forest(PARENT[:13] + [1, 0, 14], 15)            # 13 -> 1 -> 9 -> 11 -> 13
    assert not cm.check_forest(PARENT[:15] + [16], 15)                  # a parent above n_nodes
    assert not cm.check_forest([0, 1], 1)                               # its own parent


def test_classes_of_a_small_text():
    """k = 8 over a 300-base source, a node per stretch of 50 (1..6), 1 and 2 under 7, 3 and 4 under 8, 7 and 8 under 9; 5, 6 roots"""
    g = cc.rand_bases(np.random.RandomState(3), 300)
    kmers = [g[i:i + 8] for i in range(293)]
    assert len(set(kmers)) == 293
    keys = rs_model.encode_kmers(kmers, 8)
    row_node = np.array([i // 50 + 1 for i in range(293)], np.uint32)
    parent = [0, 7, 7, 8, 8, 0, 0, 9, 9, 0]
    text = b"\n".join([g[5:30],                       # node 1: 18 hits
                       g[40:60],                      # 10 k-mers of node 1, 3 of node 2: node 1
                       g[10:20] + b"N" + g[60:70],    # 3 of node 1, 3 of node 2 (none across the N): node 7
                       g[10:20] + b"N" + g[110:120],  # nodes 1 and 3: node 9
                       g[10:20] + b"N" + g[210:220],  # nodes 1 and 5: nobody
                       b"ACGTNACG", b"", g[0:7]]) + b"\n"
    per, n_rec = cm.record_hits(text, keys, row_node, 8)
    assert n_rec == 7 and per[0] == {1: 18} and per[1] == {1: 10, 2: 3}
    assert {v: c for v, c in per[2].items()} == {1: 3, 2: 3}
    assert cm.classes_per_record(text, keys, row_node, parent, 8, 1).tolist() == [1, 1, 7, 9, 0, 0, 0]
    assert cm.classes_per_record(text, keys, row_node, parent, 8, 4).tolist() == [1, 1, 0, 0, 0, 0, 0]
    direct, node_hits, kmers_n = cm.classify_model(text, keys, row_node, parent, 9, 8, 1)
    assert direct.tolist() == [3, 2, 0, 0, 0, 0, 0, 1, 0, 1] and int(direct.sum()) == n_rec
    assert node_hits.tolist() == [0, 37, 6, 3, 0, 3, 0, 0, 0, 0]
    assert kmers_n.tolist() == [0, 50, 50, 50, 50, 50, 43, 0, 0, 0]
    # a k-mer listed under two nodes counts for nobody; listed twice under one it stays that node's
    keys2 = np.concatenate([keys, keys[[12, 13]]])
    rn2 = np.concatenate([row_node, [4, 1]]).astype(np.uint32)
    d2, h2, k2 = cm.classify_model(text, keys2, rn2, parent, 9, 8, 1)
    # (k-mer 12 stands in records 0, 2, 3 and 4)
    assert int(k2[1]) == 49 and int(h2[0]) == 4 and int(h2[1]) == 33 and int(h2.sum()) == int(node_hits.sum())


@pytest.fixture(scope="module")
def cases():
    g = cc.source()
    return g, {name: cc.table(name, g) for name in cc.TABLES}, cc.one_length_block(g), cc.ragged_block(g, 1)


@pytest.mark.parametrize("tname", list(cc.TABLES))
def test_the_device_test_inputs_are_not_vacuous(cases, tname):
    g, tables, one, ragged = cases
    k, _, keys, row_node = tables[tname]
    par = cc.parents()
    assert cm.check_forest(par, cc.N_NODES) and any(int(par[v]) > v for v in range(1, cc.N_NODES + 1))
    assert max(len(cm.root_path(par, v)) for v in range(1, cc.N_NODES + 1)) == 40
    assert sum(1 for v in range(1, cc.N_NODES + 1) if par[v] == 0) == 2
    _, un = cm.kmer_nodes(keys, row_node)
    assert keys.size - np.unique(keys).size == 1 and not (un == 121).any() and not (un == 300).any() and (un == 0).sum() > cc.STRETCH // cc.TABLES[tname][1]      # (a whole stretch and the slot listed twice)
    per, n_rec = cm.record_hits(one, keys, row_node, k)
    det = cm.classes_detail(one, keys, row_node, par, k, 1, per)
    ties = [d for d in det if d[2]]
    assert len(ties) >= 20                                                             # classes that came from a tie
    assert sum(1 for d in ties if d[0] and d[0] not in d[3]) >= 5                      # ... whose common ancestor has no hits itself
    assert sum(1 for d in ties if d[0] == 0) >= 1 and sum(1 for d in ties if d[0] == 40) >= 1      # across trees; up to the root
    direct = np.bincount([d[0] for d in det], minlength=cc.N_NODES + 1)
    assert int((direct[1:] > 0).sum()) >= 200 and int(direct.sum()) == n_rec == 3000
    det8 = cm.classes_detail(one, keys, row_node, par, k, 8, per)
    assert sum(1 for d in det8 if d[0] == 0 and any(d[3])) >= 1                        # unclassified with hits
    per_r, _ = cm.record_hits(ragged, keys, row_node, k)
    distinct = sorted(len([v for v in h if v]) for h in per_r)
    assert distinct[-1] > 100 and sum(1 for n in distinct if n > 8) >= 4 and 7 in distinct and 8 in distinct
    assert any(len(p) > 4096 for p in ragged.split(b"\n")) and b"\n\n" in ragged


def test_node_hits_are_the_labelled_column_sums(cases):
    g, tables, one, _ = cases
    k, _, keys, row_node = tables["k31_sampled"]
    lab = cc.relabel15(row_node)
    per15 = label_model.labeled_hits_per_record(one, keys, lab, 15, k)
    direct, node_hits, kmers = cm.classify_model(one, keys, lab, [0] * 16, 15, k, 1)
    assert node_hits.tolist() == per15.sum(axis=1).tolist() and int(node_hits[0]) > 0
    _, ul = label_model.kmer_labels(keys, lab)
    assert kmers[1:].tolist() == [int((ul == j).sum()) for j in range(1, 16)]
    assert int(direct.sum()) == per15.shape[1] == 3000
    assert int(node_hits.sum()) == int(rs_model.hits_per_record(one, np.unique(keys), k).sum())


# ---------------------------------------------------------------------------------------------- the report


def test_report_text_and_row_nodes():
    from strainscan_amd import read_reports as rr
    ids = [2, 3, 5, 8, 9, 12, 40]
    parent_of = {2: 8, 3: 8, 5: 9, 8: 12, 9: 12, 12: None, 40: None}
    leaves = {2, 3, 5, 40}
    direct = [7, 10, 0, 3, 2, 0, 5, 1]
    hits = [11, 100, 0, 30, 20, 1, 50, 9]
    kmers = [0, 4, 5, 6, 7, 8, 9, 2]
    text = rr.read_classes_text(ids, parent_of, leaves, direct, hits, kmers)
    assert text == cm.report_text(ids, parent_of, leaves, direct, hits, kmers)
    assert text == ("node\tparent\tcluster\tkmers\thits\treads_direct\treads_clade\n"
                    "unclassified\t-\t-\t0\t11\t7\t7\n"
                    "2\t8\tC2\t4\t100\t10\t10\n"
                    "3\t8\tC3\t5\t0\t0\t0\n"
                    "5\t9\tC5\t6\t30\t3\t3\n"
                    "8\t12\t-\t7\t20\t2\t12\n"
                    "9\t12\t-\t8\t1\t0\t3\n"
                    "12\t-\t-\t9\t50\t5\t20\n"
                    "40\t-\tC40\t2\t9\t1\t1\n")
    rows = [ln.split("\t") for ln in text.split("\n")[1:-1]]
    assert sum(int(r[5]) for r in rows) == sum(direct)                                  # reads_direct sums to the records
    # rows of the tree's table -> nodes: a row that two nodes list, or none, is nobody's
    node_rows = {2: [0, 1, 2], 3: [3, 2], 5: np.array([4, 4]), 8: [], 9: [7], 12: [6]}
    assert rr.tree_row_nodes(ids, node_rows, 9).tolist() == [1, 1, 0, 2, 3, 0, 6, 5, 0]


def _parsers():
    from strainscan_amd import StrainScan
    out = []
    for multi in (False, True):
        ap = argparse.ArgumentParser(prog="x")
        StrainScan.add_arguments(ap, multi=multi)
        out.append(ap)
    return out


def test_flag_parsing(capsys):
    import strainscan_amd
    from strainscan_amd import read_reports as rr
    for ap in _parsers():
        base = ["-i", "r.fq", "-d", "DB"]
        assert ap.parse_args(base).classify_reads == 0                                  # off by default
        assert ap.parse_args(base + ["--classify_reads", "1"]).classify_reads == 1
        assert ap.parse_args(base + ["--classify_reads", "12"]).classify_reads == 12
        for bad in ("0", "-1", "x", "1.5", ""):
            with pytest.raises(SystemExit) as e:
                ap.parse_args(base + ["--classify_reads", bad])
            assert e.value.code == 2, bad
    capsys.readouterr()
    try:
        strainscan_amd.set_classify_reads(2)
        assert rr.CLASSIFY_READS == {"m": 2, "rows": {}, "skipped": None}
        for bad in (-1, 1.5, True, "2"):
            with pytest.raises(ValueError):
                strainscan_amd.set_classify_reads(bad)
        strainscan_amd.set_classify_reads(0)
        assert rr.CLASSIFY_READS["m"] == 0
    finally:
        rr.reset_all()


def test_the_idle_hook_looks_at_nothing(tmp_path, capsys):
    from strainscan_amd import read_reports as rr
    rr.reset_all()
    try:
        img = types.SimpleNamespace(is_external=False, kdb=object())                    # (would fail on anything else it asked for)
        rr.tree_scanned(img, ["no such file"])
        rr.tree_scanned(types.SimpleNamespace(is_external=True), ["no such file"])
        rr.collect_read_classes(object(), ["no such file"])
        rr.write_all(str(tmp_path / "no_such_dir"))
        assert rr.CLASSIFY_READS == {"m": 0, "rows": {}, "skipped": None}
        assert os.listdir(tmp_path) == [] and capsys.readouterr().err == ""
        # on, with counts that came from elsewhere: one line, nothing written, and only once
        rr.classify_reads_reset(1)
        rr.tree_scanned(types.SimpleNamespace(is_external=True), ["no such file"])
        rr.tree_scanned(types.SimpleNamespace(is_external=True), ["no such file"])
        err = capsys.readouterr().err
        assert err.count("\n") == 1 and err.startswith("classify_reads: ") and err.endswith(" and no read was classified\n")
        assert rr.write_read_classes(str(tmp_path)) is None and os.listdir(tmp_path) == []
    finally:
        rr.reset_all()
