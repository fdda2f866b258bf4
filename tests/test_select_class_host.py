"""--extract_class on the host: the model (tests/select_class_model.py) on a hand-worked forest, the conditions that keep
tests/test_select_class_gpu.py from passing vacuously (checked on the model for that test's inputs, tests/class_cases.py, and its
clade list), the parser of the flag's list, the flag itself and the two new symbols.  What the device selects is
tests/test_select_class_gpu.py's."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

from tests import class_cases as cc, class_model as cm, select_class_model as scm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the clades of the device test: unclassified; the root of the first tree; a child of it (with reads of its own, and leaves
# below); a node inside the chain; the chain's deepest node; a leaf; the second root; a node without rows; a node beyond the
# source; and the first root once more
CLADES = [0, 40, 41, 20, 1, 61, 281, 121, 300, 40]

# test_classify_host.py's forest: 13 -- 11 -- 9 -- 1, 2 / 10 -- 3, 4;  13 -- 12 -- 5, 6, 7, 8;  14 -- 15
PARENT = [0, 9, 9, 10, 10, 12, 12, 12, 12, 11, 11, 13, 13, 0, 0, 14]


def test_hand_worked_clades():
    ic = lambda cls, c: scm.in_clade(PARENT, cls, c)      # noqa: E731
    assert ic(1, 1) and ic(1, 9) and ic(1, 11) and ic(1, 13) and not ic(1, 10) and not ic(1, 12) and not ic(1, 14)
    assert ic(9, 9) and not ic(9, 1)                                    # a node is in its own clade, not in a child's
    assert ic(15, 14) and not ic(15, 13)                                # the second tree
    assert ic(0, 0) and not ic(0, 13) and not ic(0, 1)                  # class 0 is in clade 0 and in no other
    assert not ic(1, 0) and not ic(13, 0)                               # ... which holds nothing else
    text = b"AAA\nCCC\n\nGGG\nTTT\nAAA\n"
    classes = [1, 9, 0, 15, 2]
    assert scm.records_of(text) == [b"AAA", b"CCC", b"GGG", b"TTT", b"AAA"]
    assert scm.selected(text, classes, PARENT, 9) == [b"AAA", b"AAA", b"CCC"]
    assert scm.selected(text, classes, PARENT, 1) == [b"AAA"]
    assert scm.selected(text, classes, PARENT, 0) == [b"GGG"]
    assert scm.selected(text, classes, PARENT, 14) == [b"TTT"]
    assert scm.selected(text, classes, PARENT, 12) == []
    # the clades of the roots and clade 0 hold every record once
    assert sorted(scm.selected(text, classes, PARENT, 13) + scm.selected(text, classes, PARENT, 14) + scm.selected(text, classes, PARENT, 0)) \
        == sorted(scm.records_of(text))


@pytest.fixture(scope="module")
def cases():
    g = cc.source()
    return g, {name: cc.table(name, g) for name in cc.TABLES}, {"one": cc.one_length_block(g), "ragged": cc.ragged_block(g, 1)}


@pytest.mark.parametrize("block", ["one", "ragged"])
@pytest.mark.parametrize("tname", list(cc.TABLES))
def test_the_device_test_inputs_are_not_vacuous(cases, tname, block):
    g, tables, blocks = cases
    k, _, keys, row_node = tables[tname]
    text = blocks[block]
    par = cc.parents()
    per, n_rec = cm.record_hits(text, keys, row_node, k)
    det = cm.classes_detail(text, keys, row_node, par, k, 1, per)
    classes = [d[0] for d in det]
    direct = np.bincount(classes, minlength=cc.N_NODES + 1)
    size = {c: len(scm.selected(text, classes, par, c)) for c in set(CLADES)}
    print(tname, block, "records", n_rec, "clades", size, "direct[41]", int(direct[41]), "direct[20]", int(direct[20]), "direct[61]", int(direct[61]))
    for c in (0, 40, 41, 20, 1, 61, 281):
        assert size[c] > 0, c
    assert size[121] == 0 and size[300] == 0
    assert size[41] > int(direct[41]) > 0                     # a clade is more than its node's own reads
    assert size[40] < n_rec                                   # ... and the largest one is not everything
    assert all(size[c] == cm.clade_sums(direct, par, cc.N_NODES)[c] for c in set(CLADES))      # reads_clade, by its other statement
    assert size[0] + size[40] + size[281] == n_rec
    # M = 3 moves records into clade 0
    classes3 = [d[0] for d in cm.classes_detail(text, keys, row_node, par, k, 3, per)]
    assert len(scm.selected(text, classes3, par, 0)) > size[0]
    if block == "ragged":
        recs = scm.records_of(text)
        listed = [c for c in CLADES if c]
        long_i = next(i for i, r in enumerate(recs) if len(r) > 19000)
        assert any(scm.in_clade(par, classes[long_i], c) for c in listed)                  # the 20 kb record
        many = [i for i, h in enumerate(per) if len([v for v in h if v]) > 8]               # the device's general path
        assert sum(1 for i in many if any(scm.in_clade(par, classes[i], c) for c in listed)) >= 1
        assert b"\n\n" in text                                                              # an empty record


def test_the_list_parser():
    from strainscan_amd import _lib, read_reports as rr
    assert rr.parse_class_list("unclassified") == ["unclassified"]
    assert rr.parse_class_list("called") == ["called"]
    assert rr.parse_class_list("C12") == ["C12"] and rr.parse_class_list("12") == ["12"] and rr.parse_class_list("0") == ["0"]
    assert rr.parse_class_list("unclassified,called,7,C7,C12") == ["unclassified", "called", "7", "C7", "C12"]      # (7 and C7 are two items)
    most = ",".join(str(i) for i in range(1, _lib.CLASS_CLADES_MAX + 1))
    assert _lib.CLASS_CLADES_MAX == 64 and len(rr.parse_class_list(most)) == 64
    for bad in ("", ",", "1,", ",1", "1,,2",                              # an empty item
                "foo", "c1", "C", "C-1", "-1", "1.5", " 1", "1 ", "C 1", "CC1", "01", "C01", "Unclassified", "called2", "1;2",      # another form
                "C1,C1", "unclassified,3,unclassified", "called,called", "5,5",      # the same item twice
                most + ",65"):                                                    # more than 64
        with pytest.raises(ValueError):
            rr.parse_class_list(bad)


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
    from strainscan_amd import StrainScan, read_reports as rr
    for ap in _parsers():
        base = ["-i", "r.fq", "-d", "DB"]
        assert ap.parse_args(base).extract_class is None                                    # off by default
        a = ap.parse_args(base + ["--classify_reads", "1", "--extract_class", "unclassified,called,C3,9"])
        assert a.extract_class == ["unclassified", "called", "C3", "9"]
        StrainScan.refuse_extract_class_alone(ap, a)
        for bad in ("", "foo", "C1,C1", "1,", ",".join(str(i) for i in range(65))):
            with pytest.raises(SystemExit) as e:
                ap.parse_args(base + ["--classify_reads", "1", "--extract_class", bad])
            assert e.value.code == 2, bad
        with pytest.raises(SystemExit) as e:                                                # without --classify_reads
            StrainScan.refuse_extract_class_alone(ap, ap.parse_args(base + ["--extract_class", "unclassified"]))
        assert e.value.code == 2
    capsys.readouterr()
    try:
        strainscan_amd.set_extract_reads(0, "somewhere")
        strainscan_amd.set_extract_class(["unclassified", "C3"])
        assert rr.EXTRACT_CLASS == {"items": ["unclassified", "C3"], "tree": {}, "done": {}, "skipped": None, "files": []}
        assert rr.EXTRACT_READS["dir"] == "somewhere"
        strainscan_amd.set_extract_class("called,4", "elsewhere")
        assert rr.EXTRACT_CLASS["items"] == ["called", "4"] and rr.EXTRACT_READS["dir"] == "elsewhere"
        with pytest.raises(ValueError):
            strainscan_amd.set_extract_class(["foo"])
        strainscan_amd.set_extract_class(None)
        assert rr.EXTRACT_CLASS["items"] == []
        strainscan_amd.set_extract_class("7")
        rr.reset_all()
        assert rr.EXTRACT_CLASS["items"] == []
    finally:
        rr.reset_all()


def test_the_idle_hooks_look_at_nothing(tmp_path, capsys):
    import types
    from strainscan_amd import read_reports as rr
    rr.reset_all()
    try:
        rr.collect_called_classes([1, 2], "no such dir", True, ["no such file"])
        rr.collect_read_classes(object(), ["no such file"])
        assert capsys.readouterr().err == "" and os.listdir(tmp_path) == []
        # on, and the classification is skipped (counts from elsewhere): one line each, nothing written, and only once
        rr.classify_reads_reset(1)
        rr.extract_class_reset(["unclassified", "called"])
        rr.extract_reads_reset(0, str(tmp_path))
        for _ in range(2):
            rr.tree_scanned(types.SimpleNamespace(is_external=True), ["no such file"])
            rr.collect_called_classes([1, 2], "no such dir", True, ["no such file"])
        err = capsys.readouterr().err.split("\n")
        assert len(err) == 3 and err[0].startswith("classify_reads: ") and err[2] == ""
        assert err[1].startswith("extract_class: --classify_reads was skipped (") and err[1].endswith(" and nothing was extracted")
        assert os.listdir(tmp_path) == []
    finally:
        rr.reset_all()


def test_header_and_library_carry_the_symbols():
    from strainscan_amd import _lib
    hdr = open(os.path.join(REPO, "include", "strainscan_hip.h")).read()
    assert re.search(r"#define\s+SS_SELECT_CLADES_MAX\s+64\b", hdr)
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ("ss_reads_select_class", "ss_reads_select_class_calls"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert hasattr(lib, sym) and sym in _lib.SIGNATURES, sym
