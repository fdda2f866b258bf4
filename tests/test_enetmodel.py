"""What tests/test_l2_solver_gpu.py takes for granted about its own inputs, checked with the CPU oracle alone: the long-double
model follows the float64 oracle, the knife-edge pairs are rare, the few-rows cases are stable under a 1e-9 change of the
cross-validation errors and a tenth of them end at the all-zero refit."""
import numpy as np

from tests import enetmodel as em


def test_long_double_model_follows_the_oracle():
    pairs = knife = 0
    worst = 0.0
    for name in em.PATH_CASES:
        c, r = em.path_case(name), em.path_case_reference(name)
        pairs += r["knife"].size
        knife += int(r["knife"].sum())
        worst = max(worst, r["ld_diff"])
        assert c["positive"] or r["coefs"].min() < 0.0, name           # the second signal does turn coefficients negative
        if c["max_iter"] == 7:
            assert (r["iters"] == 7).any(), name
    assert pairs >= 480 and knife * 100 <= pairs, (knife, pairs)
    assert worst <= 1e-12, worst


def test_stats_from_rows_give_the_gram_statistics():
    from strainscan_amd import l2
    c = em.path_case("p7_n40_it7")
    for f in range(c["F"]):
        Q, q, yy, n = l2.gram_from_stats(c["test_stats"][f], c["p"])
        Xe, ye = c["X"][c["test_sel"][f]], c["y"][c["test_sel"][f]]
        assert np.array_equal(Q, Xe.T @ Xe) and np.array_equal(q, Xe.T @ ye) and yy == float((ye * ye).sum()) and n == len(ye)


def test_few_rows_cases_are_stable_and_reach_the_edge():
    cases = em.few_rows_cases()
    zero = 0
    for p, n_keep, seed in cases:
        case = em.few_rows_case(p, n_keep, seed)
        assert int(case["kept"].sum()) == n_keep and case["K"] % 32 != 0
        assert not case["kept"][:n_keep].all()                        # the rows not kept lie among the kept ones
        want = em.few_rows_oracle(case)
        assert want["stable"], (p, n_keep, seed)
        zero += not want["coef"].any()
    assert len(cases) >= 60 and zero * 10 >= len(cases), (zero, len(cases))
