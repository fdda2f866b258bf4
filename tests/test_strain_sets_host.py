"""The strain-set model (tests/strain_set_model.py) on the inputs of tests/strain_set_cases.py, without a device: the conditions that
keep tests/test_strain_sets_gpu.py from passing vacuously, the model against label_model where every mask has one bit, the two
report texts on a hand-made example, and read_reports.strain_row_sets."""
import os
import re

import numpy as np
import pytest

from tests import class_cases as cc, label_model, strain_set_cases as sc, strain_set_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return cc.source()


@pytest.fixture(scope="module")
def texts(g):
    return sc.host_texts(g)


_TABLES = {}


def _table(name, g):
    if name not in _TABLES:
        _TABLES[name] = sc.table(name, g)
    return _TABLES[name]


@pytest.mark.parametrize("tname", [t for t, v in sc.TABLES.items() if not v[4]])
def test_every_kind_of_record_is_there(g, texts, tname):
    k, n, kmers, row_sets, keys, vsets = _table(tname, g)
    assert len(row_sets) == len(kmers) == len(keys) + 1 and int(row_sets.max()) < (1 << n)
    uk, um = sm.kmer_sets(keys, vsets)
    assert uk.size == len(keys) - 2                                   # two k-mers are listed twice ...
    dup = [int(um[np.searchsorted(uk, keys[-2 + i])]) for i in range(2)]
    first = int(vsets[np.nonzero(keys[:-2] == keys[-1])[0][0]])
    assert dup[0] == int(vsets[-2]) != 0 and dup[1] == 0 and first != 0 and first != int(vsets[-1])      # ... one keeps its mask, one loses it
    if n >= 15:
        assert int(vsets.max()) == (1 << n) - 1                       # the mask with every bit
    for sname, text in texts.items():
        if sname == "long":
            continue
        per, n_rec = sm.record_votes(text, keys, vsets, k)
        r1 = sm.classify_strains_model(text, keys, vsets, n, k, 1, per)
        sizes = np.array([sm.popcount(s) for s in r1["sets"]])
        hs = [sm.strain_hits_of(hm, n) for hm in per]
        no_hit = sum(1 for h in hs if not any(h))
        only0 = sum(1 for h in hs if h[0] and not any(h[1:]))
        print(tname, sname, "records", n_rec, "unique", int((sizes == 1).sum()), "two-way", int((sizes == 2).sum()), "three and more",
              int((sizes >= 3).sum()), "no hit", no_hit, "mask 0 only", only0, "distinct sets", int((r1["set_reads"] > 0).sum()))
        assert (sizes == 1).any() and no_hit > 0 and only0 > 0, (tname, sname)
        if n >= 2:
            assert (sizes == 2).any(), (tname, sname)
        if n >= 3:
            assert (sizes >= 3).any(), (tname, sname)
        if n >= 15:
            assert r1["set_reads"][(1 << n) - 1] > 0, (tname, sname)
        r8 = sm.classify_strains_model(text, keys, vsets, n, k, 8, per)
        low = int(((r8["scores"] > 0) & (r8["scores"] < 8)).sum())
        print(tname, sname, "M 8: 0 < score < 8", low)
        assert low > 0 and (r8["sets"][(r8["scores"] < 8)] == 0).all(), (tname, sname)
        # the invariants of the definition
        for r in (r1, r8):
            assert int(r["set_reads"].sum()) == n_rec == int(r["unique"].sum() + r["tied"][0])
            assert all(int(r["unique"][j]) == int(r["set_reads"][1 << (j - 1)]) for j in range(1, n + 1))
            assert abs(sum(sm.reads_share(r["set_reads"], n)) - n_rec) < 1e-6


def test_the_long_record_outgrows_sixteen_bits(g, texts):
    k, n, _, _, keys, vsets = _table("k31_whole_n2", g)
    r = sm.classify_strains_model(texts["long"], keys, vsets, n, k, 1)
    # (every k-mer of the record is strain 1's but the one that is listed again under another mask)
    assert r["scores"].tolist() == [len(g) - 1 - k + 1 - 1] and r["scores"][0] > 65535 and r["sets"].tolist() == [1]
    assert int(r["strain_hits"][0]) == 1
    assert int(r["strain_hits"][1]) > 65535 > int(r["strain_hits"][2]) > 4095


def test_one_bit_masks_are_labels(g, texts):
    k, n, _, _, keys, vsets = _table("k25_n15", g)
    low, lab = sc.one_bit_rows(vsets)
    text = texts["ragged_1"]
    r = sm.classify_strains_model(text, keys, low, n, k, 1)
    per = label_model.labeled_hits_per_record(text, keys, lab, n, k)
    assert r["strain_hits"][1:].tolist() == per[1:].sum(axis=1).tolist() and int(r["strain_hits"][0]) == int(per[0].sum())
    assert int(r["strain_hits"][1:].sum()) > 0


def test_set_rule_by_hand():
    assert sm.set_of([5, 0, 0], 1) == (0, 0)                          # hits of mask 0 alone
    assert sm.set_of([0, 3, 3, 1], 1) == (0b011, 3)
    assert sm.set_of([0, 3, 3, 1], 4) == (0, 3)                       # below M: unassigned, the score kept
    assert sm.set_of([0, 2, 7], 7) == (0b10, 7)
    assert sm.strain_hits_of({0: 2, 0b101: 3, 0b100: 1}, 3) == [2, 3, 0, 4]
    assert sm.selected([0, 1, 3, 2, 3], 3, 0).tolist() == [2, 4] and sm.selected([0, 1, 3, 2, 3], 1, 1).tolist() == [1, 2, 4]
    assert sm.selected([0, 1, 3], 0, 0).tolist() == [0] and sm.selected([0, 1, 3], 0, 1).tolist() == []


def test_report_texts_by_hand():
    sr = np.zeros(8, np.uint64)
    sr[0], sr[1], sr[3], sr[4], sr[7] = 4, 10, 6, 6, 3
    r = dict(unique=np.array([4, 10, 0, 6], np.uint64), tied=np.array([9, 9, 9, 3], np.uint64), strain_hits=np.array([7, 100, 50, 40], np.uint64),
             kmers=np.array([0, 11, 12, 13], np.uint64), set_reads=sr)
    cl = [("C7", ["s_a", "s_b", "s_c"], r)]
    assert sm.classes_text(cl) == ("table\tstrain\tkmers\thits\treads_unique\treads_tied\treads_share\n"
                                   "C7\tunassigned\t0\t7\t4\t0\t4.000\n"
                                   "C7.1\ts_a\t11\t100\t10\t9\t14.000\n"
                                   "C7.2\ts_b\t12\t50\t0\t9\t4.000\n"
                                   "C7.3\ts_c\t13\t40\t6\t3\t7.000\n")
    assert sm.sets_text(cl) == "table\tset\tstrains\treads\nC7\t1\t1\t10\nC7\t1,2\t2\t6\nC7\t3\t1\t6\nC7\t1,2,3\t3\t3\n"


def test_header_restates_the_rule_and_the_build_lists_the_source():
    hdr = open(os.path.join(ROOT, "include", "strainscan_hip.h")).read()
    assert re.search(r"#define\s+SS_STRAIN_SET_MAX\s+16\b", hdr) and re.search(r"#define\s+SS_SELECT_STRAINS_MAX\s+32\b", hdr)
    for name in ("ss_reads_classify_strains", "ss_reads_classify_strains_calls", "ss_reads_classify_strains_ties", "ss_reads_select_strains",
                 "ss_reads_select_strains_calls"):
        assert re.search(r"\bint\s+%s\(" % name, hdr), name
    assert "ss_strain_sets.hip" in open(os.path.join(ROOT, "strainscan_amd", "csrc", "Makefile")).read()
    assert "SS_STRAIN_SET_MAX" in open(os.path.join(ROOT, "strainscan_amd", "csrc", "ss_minik.hip")).read()
    from strainscan_amd import _lib
    assert _lib.STRAIN_SET_MAX == 16 and _lib.SELECT_STRAINS_MAX == 32
