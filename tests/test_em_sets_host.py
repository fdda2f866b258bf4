"""The EM model (tests/em_model.py) and the inputs of tests/em_cases.py without a device: the conditions that keep
tests/test_em_sets_gpu.py from passing vacuously, the rule on cases small enough to do by hand, strain_em.tsv's text on hand-made
numbers, the command's refusals and the new symbols."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import class_cases as cc, em_cases as ec, em_model as em, strain_set_cases as sc, strain_set_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return cc.source()


@pytest.fixture(scope="module")
def texts(g):
    t = sc.host_texts(g)
    t["empty"] = b""
    return t


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    return _lib


_SETS = {}


def _model_sets(g, texts, tkey, sname, m):
    """the model's classification of one (table, set, M): (n, result dict)"""
    if (tkey, sname, m) not in _SETS:
        k, n, _, _, keys, vsets = ec.table(tkey, g)
        _SETS[tkey, sname, m] = (n, sm.classify_strains_model(texts[sname], keys, vsets, n, k, m))
    return _SETS[tkey, sname, m]


def test_the_cases_cover_what_the_issue_names():
    assert {ec.TABLES[c[0]][1] for c in ec.RESAMPLED} >= {1, 2, 12, 13, 16}
    assert {c[1] for c in ec.RESAMPLED} >= {"packed", "file_order", "binned_ascii", "ragged_0", "ragged_1", "ragged_1023", "two_slabs", "empty", "long"}
    assert set(ec.REPS) == {(0, 1), (0, 16), (16, 4), (5, 15)} and len(set(ec.SEEDS)) == 2
    # both sides of the LDS limit at twelve and at thirteen strains
    for n in (12, 13):
        sides = {(r << n) <= ec.SETW_LDS for c in ec.RESAMPLED if ec.TABLES[c[0]][1] == n for _, r in c[3]}
        assert sides == {True, False}, n
    assert (16 << 16) > ec.SETW_LDS and (1 << 16) > ec.SETW_LDS
    src = open(os.path.join(ROOT, "strainscan_amd", "csrc", "ss_strain_sets.hip")).read()
    assert re.search(r"SETW_LDS\s*=\s*1u\s*<<\s*14\b", src)


@pytest.mark.parametrize("case", [c for c in ec.RESAMPLED if c[1] not in ec.FEW], ids=lambda c: "%s-%s-M%d" % c[:3])
def test_no_resampled_case_is_vacuous(L, g, texts, case):
    tkey, sname, m, reps, seeds = case
    n, r = _model_sets(g, texts, tkey, sname, m)
    sr = r["set_reads"]
    tied = [mask for mask in range(1, 1 << n) if sm.popcount(mask) > 1 and sr[mask]]
    if n >= 2:
        assert tied, "no tied set has reads"
    assert int(sr[1:].sum()) > 0
    for seed in seeds:
        for first, n_rep in reps:
            w = em.replicate_weights(L, texts[sname], seed, first, n_rep)
            vals = set(np.unique(w).tolist())
            assert 0 in vals and 1 in vals and max(vals) >= 3, (seed, first, vals)
            counts = em.replicate_set_counts(L, texts[sname], r["sets"], n, seed, first, n_rep)
            assert (counts.sum(axis=1) == w.sum(axis=1)).all()
            if n_rep > 1:
                assert len({c.tobytes() for c in counts}) >= 2, "the replicates do not differ"
    print(tkey, sname, "M", m, "assigned", int(sr[1:].sum()), "tied sets with reads", len(tied))


def test_the_few_record_sets_are_what_they_are_called(g, texts):
    assert texts["empty"] == b"" and len([r for r in texts["long"].split(b"\n") if r]) == 1
    n, r = _model_sets(g, texts, "whole", "long", 1)
    assert r["sets"].tolist() == [1]


def test_some_main_em_needs_more_than_one_iteration(g, texts):
    most = 0
    for tkey, sname, m, _, _ in ec.RESAMPLED:
        if sname in ec.FEW:
            continue
        n, r = _model_sets(g, texts, tkey, sname, m)
        counts, masks = em.compact(r["set_reads"][None, :])
        _, iters = em.em_batch(counts, masks, n, 1000, 1e-9)
        most = max(most, int(iters[0]))
    assert most > 1


def _ulps(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))))


def test_singletons_take_their_own_reads_after_one_iteration():
    counts, masks = [30, 0, 10, 60], [1, 2, 4, 8]
    rho, it = em.em(counts, masks, 4, 1, 0.0)
    assert it == 1 and rho[1] == 0.0 and _ulps(rho[[0, 2, 3]], np.array([0.3, 0.1, 0.6])) <= 2
    rho2, it2 = em.em(counts, masks, 4, 1000, 1e-9)
    assert it2 == 2 and _ulps(rho2[[0, 2, 3]], np.array([0.3, 0.1, 0.6])) <= 4      # the second iteration only finds that nothing moves


def test_the_tie_goes_to_the_strains_in_proportion():
    rho, it = em.em([30, 10, 60], [1, 2, 3], 2, 1000, 1e-9)
    assert 1 < it < 1000 and np.abs(rho - np.array([0.75, 0.25])).max() < 1e-7 and abs(rho.sum() - 1) < 1e-12
    fixed, it_f = em.em([30, 10, 60], [1, 2, 3], 2, 50, 0.0)
    assert it_f == 50                                                 # tol == 0: exactly max_iter
    down, _ = em.em([30, 10, 60], [1, 2, 3], 2, 1000, 1e-9, descending=True)
    assert np.abs(down - rho).max() < 1e-12


def test_edges_of_the_rule():
    rho, it = em.em([0, 0], [1, 3], 2, 10, 0.0)
    assert it == 0 and not rho.any()                                  # N == 0
    rho, it = em.em([5, 0], [2, 1], 3, 10, 0.0)
    assert rho.tolist() == [0.0, 1.0, 0.0]                            # inactive strains stay 0
    rho, it = em.em([1000, 1], [1, 3], 2, 200, 0.0)                   # strain 2 loses every read: underflow to 0, no NaN
    assert it == 200 and rho[1] == 0.0 and rho[0] == 1.0 and not np.isnan(rho).any()
    assert em.abundance([0.75, 0.25], [100, 50]) == pytest.approx([0.6, 0.4], abs=1e-15)
    assert em.abundance([0.5, 0.5], [0, 50]) == [0.0, 1.0] and em.abundance([0.0, 0.0], [10, 50]) == [0.0, 0.0]
    assert [em.quantile_index(q, 20) for q in em.QUANTILES] == [0, 19] and [em.quantile_index(q, 1000) for q in em.QUANTILES] == [25, 974]


def test_em_text_by_hand():
    from strainscan_amd import read_reports as rr
    r = dict(called=[(1, "s_a"), (3, "s_b")], kmers=[100, 50], enet=["0.7", "0.3"], reads=100,
             rho=np.array([[0.75, 0.25], [0.7, 0.3], [0.8, 0.2], [1.0, 0.0]]), iters=np.array([5, 6, 7, 1], np.uint32))
    head = "table\tstrain\tkmers\treads_assigned\treads_em\tfrac_reads\tabundance\tabundance_lo\tabundance_hi\tpresent\tenet_frac\titerations\n"
    assert rr.em_text([("C7", r)]) == (head + "C7.1\ts_a\t100\t100\t75.000\t0.750000\t0.600000\t0.538462\t1.000000\t3\t0.7\t5\n"
                                       "C7.3\ts_b\t50\t100\t25.000\t0.250000\t0.400000\t0.000000\t0.461538\t2\t0.3\t5\n")
    r0 = dict(r, rho=r["rho"][:1], iters=r["iters"][:1])
    assert rr.em_text([("C7", r0)]) == (head + "C7.1\ts_a\t100\t100\t75.000\t0.750000\t0.600000\t-\t-\t-\t0.7\t5\n"
                                        "C7.3\ts_b\t50\t100\t25.000\t0.250000\t0.400000\t-\t-\t-\t0.3\t5\n")
    assert rr.bootstrap_index(0.025, 3) == em.quantile_index(0.025, 3) == 0 and rr.bootstrap_index(0.975, 3) == 2
    theta = rr.em_abundance(r["rho"], r["kmers"])
    assert [list(t) for t in theta] == [em.abundance(x, r["kmers"]) for x in r["rho"]]
    # the model's table says the same on the same vectors
    vec = np.zeros((1, 4), np.uint64)
    vec[0, 1], vec[0, 2], vec[0, 3] = 30, 10, 60
    rows = em.em_table([("C7", [(1, "s_a"), (3, "s_b")], [100, 50], ["0.7", "0.3"], vec)], 0)
    assert rows[0][:4] == ["C7.1", "s_a", 100, 100] and abs(rows[0][5] - 0.75) < 1e-7 and rows[0][7:10] == [None, None, None]


def test_state_and_python_entry_point():
    import strainscan_amd
    from strainscan_amd import read_reports as rr
    try:
        strainscan_amd.set_em_strains(0, 5)
        assert rr.EM_STRAINS["on"] and rr.EM_STRAINS["b"] == 0 and rr.EM_STRAINS["seed"] == 5
        strainscan_amd.set_em_strains(20)
        assert rr.EM_STRAINS["b"] == 20 and rr.EM_STRAINS["seed"] == 1
        for bad in (1, 1001, -1, True, 2.0):
            with pytest.raises(ValueError):
                strainscan_amd.set_em_strains(bad)
        strainscan_amd.set_em_strains(None)
        assert not rr.EM_STRAINS["on"] and rr.write_em_strains(".") is None and rr.em_replicates() == {}
        strainscan_amd.set_em_strains(20)
        rr.reset_all()
        assert not rr.EM_STRAINS["on"]
    finally:
        rr.reset_all()


@pytest.mark.parametrize("cmd", ["StrainScan", "multi_db"])
@pytest.mark.parametrize("flags,message", [(["--classify_strains", "1", "--em_strains", "1"], "1 is neither 0 nor in 2..1000"),
                                           (["--classify_strains", "1", "--em_strains", "1001"], "1001 is neither 0 nor in 2..1000"),
                                           (["--em_strains", "5"], "--em_strains needs --classify_strains M")])
def test_refusals_before_any_input_is_opened(tmp_path, cmd, flags, message):
    missing = str(tmp_path / "no_such_reads.fq")
    argv = [sys.executable, "-m", "strainscan_amd." + cmd, "-i", missing, "-d", str(tmp_path / "no_such_db"), "-o", str(tmp_path / "out")] + flags
    p = subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT))
    assert p.returncode == 2, p.stderr
    assert message in p.stderr and "unrecognized arguments" not in p.stderr
    assert not os.path.exists(str(tmp_path / "out"))


def test_header_and_library_have_the_new_calls(L):
    hdr = open(os.path.join(ROOT, "include", "strainscan_hip.h")).read()
    names = ("ss_reads_strain_sets_resampled", "ss_reads_strain_sets_resampled_calls", "ss_em_strain_sets", "ss_em_strain_sets_calls")
    for name in names:
        assert re.search(r"\bint\s+%s\(" % name, hdr), name
        assert name in L.SIGNATURES
    assert re.search(r"#define\s+SS_EM_VECTORS_MAX\s+1024\b", hdr) and re.search(r"#define\s+SS_EM_LDS_SETS\s+%d\b" % L.EM_LDS_SETS, hdr)
    assert L.EM_VECTORS_MAX == 1024
    mk = open(os.path.join(ROOT, "strainscan_amd", "csrc", "Makefile")).read()
    assert "ss_em.hip" in mk and "ss_strain_sets.hip" in mk
    import ctypes
    so = ctypes.CDLL(L.LIB_PATH)
    for name in names:
        assert getattr(so, name) is not None
