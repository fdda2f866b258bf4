"""The last device steps of layer 2, called directly: the elastic-net path on Gram statistics (enet_path_kernel of ss_enet.hip,
through l2.enet_path_gram) against the float64 oracle and the long-double model of tests/enetmodel.py; enet_cv_fit at few
kept rows against the oracle's ElasticNetCV -> lasso_mpm -> ElasticNet on the raw rows (the residual solver wherever
scikit-learn takes it); and the bit-vector kernels of ss_l2.hip (popc2 with masks, andnot_col, fold_words, fold_words_train)
against numpy, bit for bit.  Tolerances: those of test_enet_cd_residual_form and test_detect_core_vs_oracle_medium."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

from tests import enetmodel as em

pytestmark = pytest.mark.gpu

ABUND_TOL = 1e-5     # BASELINE.json north_star: abundances within 1e-5 of the reference CPU path


def _dev_u32(buf, n):
    from strainscan_amd import _lib
    out = np.zeros(n, np.uint32)
    if n:
        _lib.check(_lib.lib().ss_memcpy_d2h(_lib.ptr(out), buf.ptr, n * 4, None), "ss_memcpy_d2h")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# B: enet_path_kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(em.PATH_CASES))
def test_enet_path_gram_vs_oracle(name):
    """Coefficients, duality gaps, sweep counts and test-fold errors of one path per fold.  The zero pattern of the first
    alpha is exact (from w = 0 the first sweep is q[ii] - l1 on both sides); sweep counts are equal except where float64
    and long double disagree among themselves (enetmodel.path_reference's knife-edge pairs)."""
    from strainscan_amd import l2
    c = em.path_case(name)
    ref = em.path_case_reference(name)
    got = l2.enet_path_gram(c["Q"], c["q"], c["yy"], c["n_train"], c["alphas"], n_test=c["n_test"] if c["test_stats"] is not None else None,
                            test_stats=c["test_stats"], l1_ratio=em.L1_RATIO, max_iter=c["max_iter"], tol=1e-4, positive=c["positive"])
    F, na, p = ref["coefs"].shape
    assert got["coefs"].shape == (F, na, p) and got["iters"].shape == (F, na) and got["gaps"].shape == (F, na)
    assert np.all(np.isfinite(got["coefs"])) and np.all(np.isfinite(got["gaps"]))
    print(name, "max |dw|", np.abs(got["coefs"] - ref["coefs"]).max(), "max |dgap| rel",
          (np.abs(got["gaps"] - ref["gaps"]) / np.maximum(1.0, np.abs(ref["gaps"]))).max(),
          "iters differ at", int((got["iters"] != ref["iters"]).sum()), "knife", int(ref["knife"].sum()))
    assert np.allclose(got["coefs"], ref["coefs"], rtol=1e-9, atol=1e-11)
    assert np.array_equal(got["coefs"][:, 0] != 0, ref["coefs"][:, 0] != 0)
    assert np.all(np.abs(got["gaps"] - ref["gaps"]) <= 1e-6 * np.maximum(1.0, np.abs(ref["gaps"])))
    ok = ~ref["knife"]
    assert np.array_equal(got["iters"][ok], ref["iters"][ok]), (got["iters"], ref["iters"])
    if c["positive"]:
        assert got["coefs"].min() >= 0.0
    else:
        assert ref["coefs"].min() < 0.0 and got["coefs"].min() < 0.0            # the unconstrained branch did run
    if c["max_iter"] == 7:
        assert (ref["iters"] == 7).any() and np.array_equal(got["iters"] == 7, ref["iters"] == 7)
    if c["special"] == "zero_col":
        assert np.all(got["coefs"][:, :, p // 2] == 0.0) and np.all(c["Q"][:, p // 2, p // 2] == 0.0)
    if c["special"] == "zero_y":                   # yy == 0: tol * yy == 0, no gap is below it, every sweep runs, w = 0
        assert c["yy"][1] == 0.0 and np.all(got["coefs"][1] == 0.0) and np.all(got["iters"][1] == c["max_iter"])
    if c["test_stats"] is None:
        assert got["mse"] is None
        return
    assert got["mse"].shape == (na, F)
    want = np.zeros((na, F))
    for f in range(F):
        te = c["test_sel"][f]
        Xe, ye = c["X"][te], c["y"][te]
        for a in range(na):
            want[a, f] = em.mse_rows(Xe, ye, ref["coefs"][f, a])
    print(name, "max mse rel", (np.abs(got["mse"] - want) / np.maximum(np.abs(want), 1e-300)).max())
    assert np.allclose(got["mse"], want, rtol=1e-7, atol=1e-9)


def test_enet_path_knife_edges_are_rare():
    """The pairs left out of the sweep-count comparison above are at most 1 % of all pairs of this file."""
    pairs = knife = 0
    worst = 0.0
    for name in em.PATH_CASES:
        r = em.path_case_reference(name)
        pairs += r["knife"].size
        knife += int(r["knife"].sum())
        worst = max(worst, r["ld_diff"])
    print("knife-edge pairs: %d of %d; worst oracle-vs-long-double coefficient difference %.1e" % (knife, pairs, worst))
    assert pairs >= 480 and knife * 100 <= pairs
    assert worst <= 1e-9


def test_enet_path_gram_refusals():
    from strainscan_amd import _lib, l2
    c = em.path_case("p2_n3")

    def code(fn):
        with pytest.raises(_lib.SSError) as e:
            fn()
        return e.value.code

    al = c["alphas"]
    assert code(lambda: l2.enet_path_gram(np.zeros((1, 0, 0)), np.zeros((1, 0)), [1.0], [1.0], al)) == _lib.SS_ERANGE
    assert code(lambda: l2.enet_path_gram(np.eye(17)[None], np.ones((1, 17)), [1.0], [1.0], al)) == _lib.SS_ERANGE
    assert code(lambda: l2.enet_path_gram(np.zeros((0, 2, 2)), np.zeros((0, 2)), [], [], al)) == _lib.SS_EINVAL
    # statistics without n_test: the C entry itself (the Python face always passes an array)
    F, na, p = c["F"], al.size, c["p"]
    mse, coefs, iters, gaps = np.zeros((na, F)), np.zeros((F, na, p)), np.zeros((F, na), np.int32), np.zeros((F, na))
    rc = _lib.lib().ss_enet_path_gram(_lib.ptr(c["Q"]), _lib.ptr(c["q"]), _lib.ptr(c["yy"]), _lib.ptr(c["n_train"]), None, F, p,
                                      _lib.ptr(al), na, 0.5, 5000, 1e-4, 1, _lib.ptr(c["test_stats"]), _lib.ptr(mse),
                                      _lib.ptr(coefs), _lib.ptr(iters), _lib.ptr(gaps))
    assert rc == _lib.SS_EINVAL


# ---------------------------------------------------------------------------------------------------------------------
# C: few kept rows, composed
# ---------------------------------------------------------------------------------------------------------------------
def _few_rows_image(case):
    import scipy.sparse as sp
    from strainscan_amd import l2
    img = l2.ClusterImage(sp.csr_matrix(case["X"]))
    img.set_overlap(sp.csr_matrix(np.ones((case["K"], 1), np.int8)))
    vec = img.prepare(case["y"], [0], em.Y_LO, em.Y_HI, em.Y_HI + 0.5)
    return img, vec


def _check_fit(trace, want, n_keep, p, tag):
    assert trace["n_rows"] == n_keep and trace["p"] == p, tag
    assert np.allclose(trace["alphas_"], want["alphas"], rtol=1e-12, atol=0), tag
    assert np.allclose(trace["mse_path_"], want["mse"], rtol=1e-7, atol=1e-9), \
        (tag, np.abs(trace["mse_path_"] - want["mse"]).max())
    assert abs(trace["alpha"] - want["alpha"]) <= 1e-12 * want["alpha"], tag
    assert np.allclose(trace["coef_"], want["coef"], rtol=0, atol=ABUND_TOL), (tag, trace["coef_"], want["coef"])
    assert np.array_equal(trace["coef_"] != 0, want["coef"] != 0), (tag, trace["coef_"], want["coef"])


@pytest.mark.parametrize("p", em.FEW_P)
def test_enet_cv_fit_few_rows(p):
    """enet_cv_fit (Gram statistics for the cross-validation AND the refit) against the oracle on the raw kept rows, where
    n_train <= p sends scikit-learn to the residual solver, columns are all ones or all zeros within a training half and
    patterns appear in the test half only."""
    from strainscan_amd import identify_strains_L2_Enet_Pscan_new_sp as m
    cases = [c for c in em.few_rows_cases() if c[0] == p]
    assert {c[1] for c in cases} == set(em.few_n_keep(p))
    worst = 0.0
    for _, n_keep, seed in cases:
        case = em.few_rows_case(p, n_keep, seed)
        want = em.few_rows_oracle(case)
        assert want["stable"], (p, n_keep, seed)
        img, vec = _few_rows_image(case)
        try:
            assert vec.n_keep == n_keep
            trace = {}
            coef = m.enet_cv_fit(img, case["cols"], vec, trace)
            assert np.array_equal(coef, trace["coef_"])
            worst = max(worst, float((np.abs(trace["mse_path_"] - want["mse"]) / np.maximum(np.abs(want["mse"]), 1e-300)).max()))
            _check_fit(trace, want, n_keep, p, (p, n_keep, seed))
        finally:
            vec.close()
            img.close()
    print("p = %d: %d cases, worst relative mse difference %.1e" % (p, len(cases), worst))


def test_few_rows_cases_reach_the_no_report_edge():
    """At least a tenth of the cases above end with an all-zero refit at alphas[0]: the report / no-report edge."""
    cases = em.few_rows_cases()
    zero = 0
    for p, n_keep, seed in cases:
        want = em.few_rows_oracle(em.few_rows_case(p, n_keep, seed))
        if not want["coef"].any():
            assert want["alpha"] == want["alphas"][0]
            zero += 1
    print("%d of %d cases end all-zero" % (zero, len(cases)))
    assert len(cases) >= 60 and zero * 10 >= len(cases)


@pytest.mark.parametrize("p,n_keep", [(3, 2), (5, 11), (16, 65)])
def test_enet_cv_fit_few_rows_split_on_device(p, n_keep):
    """The same with the folds from a SplitDev (fold_words_train) handed to enet_cv_fit."""
    from strainscan_amd import identify_strains_L2_Enet_Pscan_new_sp as m
    from strainscan_amd import l2
    seed = em.FEW_SEEDS[(p, n_keep)][0]
    case = em.few_rows_case(p, n_keep, seed)
    want = em.few_rows_oracle(case)
    img, vec = _few_rows_image(case)
    assert l2.SplitDev.usable(n_keep, m.TEST_SIZE)
    split = l2.SplitDev(n_keep, m.CV_NITER, m.TEST_SIZE, 0)
    try:
        trace = {}
        m.enet_cv_fit(img, case["cols"], vec, trace, split)
        assert "shuffle_split_walk" in trace["timing_ms"]                 # the device's bits were taken, not the host's
        _check_fit(trace, want, n_keep, p, (p, n_keep, seed))
    finally:
        split.close()
        vec.close()
        img.close()


def _two_strain_cluster():
    """70 rows, 4 strains of which 0 and 2 are present; 33 rows pass the row filter [4, 60]."""
    rs = np.random.RandomState(5)
    K, S = 70, 4
    X = np.zeros((K, S), np.int8)
    X[:30, 0] = 1
    X[20:55, 2] = 1
    X[50:62, 1] = 1
    X[60:, 3] = 1
    lam = X[:, 0] * 20.0 + X[:, 2] * 9.0
    y = rs.poisson(lam).astype(np.int64)
    y[y == 1] = 0
    y[:55] = np.maximum(y[:55], 4)
    big = rs.choice(55, 22, replace=False)
    y[big] += 100                                              # above the filter's upper bound
    return X, y


def test_detect_core_few_rows_through_split_dev(monkeypatch):
    """detect_core with ShuffleSplit's swaps forced onto the device (SPLIT_DEV_MIN down) at 33 kept rows of 70, against the
    oracle's detect_strains."""
    import scipy.sparse as sp
    from oracle import oracle as orc
    from strainscan_amd import identify_strains_L2_Enet_Pscan_new_sp as m
    from strainscan_amd import l2
    X, y = _two_strain_cluster()
    K, S = X.shape
    O = np.ones((K, 1), np.int8)
    ids = ["T%d" % i for i in range(S)]
    lo, hi = 4, 60
    keep = (y >= lo) & (y <= hi)
    assert int(keep.sum()) == 33
    used = []
    real = l2.ClusterImage.fold_words_train

    def spy(self, *a, **k):
        used.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(l2.ClusterImage, "fold_words_train", spy)
    monkeypatch.setattr(m, "SPLIT_DEV_MIN", 2)
    trace = {}
    with contextlib.redirect_stdout(io.StringIO()):
        res, res2, scov, sval, fsrc = m.detect_core(sp.csr_matrix(X), sp.csr_matrix(O), ids, y.copy(), 3, lo, hi, hi, 0.9, [1], 0, 1,
                                                    0, 0, trace=trace)
    assert used == [1]
    ores, ores2, oscov, osval, ofsrc = orc.detect_strains(X, O, ids, y, 3, lo, hi, hi, [1], 0, 1, 0, 0)
    assert len(ores2) >= 2 and trace["n_rows"] == 33
    assert {k: list(v) for k, v in scov.items()} == oscov
    assert list(res2.keys()) == list(ores2.keys())
    for k in ores2:
        assert abs(float(res2[k]) - float(ores2[k])) <= ABUND_TOL * max(1.0, abs(float(ores2[k])))
        assert abs(float(res[k]) - float(ores[k])) <= ABUND_TOL
    cols = orc.prescan(X, y, y, ids, 3, 0, 0, 0)[0]
    al, mse = orc.enet_cv(X[keep][:, cols], y[keep])
    assert np.allclose(trace["alphas_"], al, rtol=1e-12, atol=0)
    assert np.allclose(trace["mse_path_"], mse, rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("n_keep", [0, 1])
def test_enet_cv_fit_refuses_an_empty_training_half(n_keep):
    """One kept row leaves ShuffleSplit(test_size=0.5) no training row, none leaves nothing at all: scikit-learn raises
    ValueError there, and so does enet_cv_fit -- no model of zeros from Q = 0, no 0 / 0."""
    import scipy.sparse as sp
    from strainscan_amd import identify_strains_L2_Enet_Pscan_new_sp as m
    from strainscan_amd import l2
    K = 5
    X = np.array([[1, 0], [1, 1], [0, 1], [1, 1], [0, 0]], np.int8)
    y = np.array([0, 7, 0, 9000, 1], np.int64) if n_keep else np.array([0, 9000, 0, 9000, 1], np.int64)
    img = l2.ClusterImage(sp.csr_matrix(X))
    img.set_overlap(sp.csr_matrix(np.ones((K, 1), np.int8)))
    vec = img.prepare(y, [0], em.Y_LO, em.Y_HI, em.Y_HI)
    try:
        assert vec.n_keep == n_keep
        with pytest.raises(ValueError, match="%d sample" % n_keep if n_keep == 0 else "n_samples=1, test_size=0.5"):
            m.enet_cv_fit(img, [0, 1], vec, {})
    finally:
        vec.close()
        img.close()


# ---------------------------------------------------------------------------------------------------------------------
# D: the bit-vector kernels
# ---------------------------------------------------------------------------------------------------------------------
D_K = (1, 31, 32, 33, 127, 128, 129, 4097, 200_003)
D_S = (1, 7, 40)


def _words(mask, W):
    """bool[K] -> uint32[W], row i = bit i & 31 of word i >> 5, zero beyond K."""
    out = np.zeros(W * 4, np.uint8)
    pk = np.packbits(mask, bitorder="little")
    out[:pk.size] = pk
    return out.view(np.uint32)


def _bools(words, K):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:K].astype(bool)


def _image(K, S, seed):
    import scipy.sparse as sp
    from strainscan_amd import l2
    rs = np.random.RandomState(seed)
    X = rs.random_sample((K, S)) < 0.45
    X[K - 1, S - 1] = True                                       # the last row, the last plane
    img = l2.ClusterImage(sp.csr_matrix(X.astype(np.int8)))
    assert img.W % 4 == 0 and img.W * 32 >= K
    return img, X, rs


@pytest.mark.parametrize("K", D_K)
def test_popc2_with_masks_vs_numpy(K):
    """out1[s] = popcount(X_s & A), out2[s] = popcount(X_s & A & B) for A, B null or not; random words (their padding bits
    random too: the planes' padding is zero), A all zero, A = img.ones()."""
    from strainscan_amd import l2
    for S in D_S:
        img, X, rs = _image(K, S, 1000 + S)
        W = img.W
        rnd = lambda: rs.randint(0, 1 << 32, size=W, dtype=np.int64).astype(np.uint32)     # noqa: E731
        Aw, Bw = rnd(), rnd()
        A, B = _bools(Aw, K), _bools(Bw, K)
        dA, dB = l2.DevBuf.from_array(Aw), l2.DevBuf.from_array(Bw)
        every = np.ones(K, bool)
        for a_dev, a, b_dev, b in ((None, every, None, every), (dA, A, None, every), (None, every, dB, B), (dA, A, dB, B)):
            o1, o2 = img.popc2(a_dev, b_dev)
            assert np.array_equal(o1, (X & a[:, None]).sum(axis=0)), (K, S)
            assert np.array_equal(o2, (X & (a & b)[:, None]).sum(axis=0)), (K, S)
        dZ = l2.DevBuf.from_array(np.zeros(W, np.uint32))
        o1, o2 = img.popc2(dZ, dB)
        assert not o1.any() and not o2.any()
        ones = img.ones()
        assert np.all(_dev_u32(ones, W) == 0xFFFFFFFF)
        o1, o2 = img.popc2(ones, dB)
        assert np.array_equal(o1, X.sum(axis=0)) and np.array_equal(o2, (X & B[:, None]).sum(axis=0))
        for d in (dA, dB, dZ, ones):
            d.close()
        img.close()


@pytest.mark.parametrize("K", D_K)
def test_andnot_col_vs_numpy(K):
    """nu &= ~X_col over all W words: the words (and bits) of nu beyond K stay as they were; a second application changes nothing."""
    from strainscan_amd import l2
    for S in D_S:
        img, X, rs = _image(K, S, 2000 + S)
        W = img.W
        planes = img.planes().reshape(S, W)
        for s in range(S):
            assert np.array_equal(planes[s], _words(X[:, s], W))
        for col in sorted({0, S - 1}):
            nu0 = rs.randint(0, 1 << 32, size=W, dtype=np.int64).astype(np.uint32)
            nu0[-1] |= np.uint32(0x80000000)                      # a padding bit that must survive
            nu = l2.DevBuf.from_array(nu0)
            img.andnot_col(col, nu)
            want = nu0 & ~_words(X[:, col], W)
            got = _dev_u32(nu, W)
            assert np.array_equal(got, want), (K, S, col)
            if K < W * 32:
                assert got[-1] & np.uint32(0x80000000)
            img.andnot_col(col, nu)
            assert np.array_equal(_dev_u32(nu, W), want), (K, S, col)
            nu.close()
        img.close()


def _keep_patterns(K, rs):
    """(name, bool[K]): nothing kept, one row, every row, and random rows around a stretch of all-zero words with the last
    row kept."""
    pats = [("none", np.zeros(K, bool)), ("all", np.ones(K, bool))]
    one = np.zeros(K, bool)
    one[K - 1] = True
    pats.append(("last_only", one))
    one = np.zeros(K, bool)
    one[K // 2] = True
    pats.append(("one", one))
    r = rs.random_sample(K) < 0.6
    a, b = (K // 3) & ~31, ((K // 3) & ~31) + 96
    r[a:b] = False                                               # three whole words (where K has them)
    r[K - 1] = True
    pats.append(("random", r))
    return pats


def _fold_expect(keep, bits):
    out = np.zeros(keep.size, np.uint32)
    out[keep] = (bits & np.uint32(0x7FFFFFFF)) | np.uint32(0x80000000)
    return out


@pytest.mark.parametrize("K", D_K)
def test_fold_words_vs_numpy(K):
    """fold word of a kept row = bit 31 | the low 31 bits of split_bits[rank among the kept rows]; 0 for the others."""
    from strainscan_amd import l2
    img, X, rs = _image(K, 1, 3000)
    for name, keep in _keep_patterns(K, rs):
        n_keep = int(keep.sum())
        bits = rs.randint(0, 1 << 32, size=n_keep, dtype=np.int64).astype(np.uint32)
        bits[::2] |= np.uint32(0x80000000)                       # bit 31 on input: masked, not carried
        kd = l2.DevBuf.from_array(_words(keep, img.W))
        f = img.fold_words(kd, bits, n_keep)
        assert np.array_equal(_dev_u32(f, K), _fold_expect(keep, bits)), (K, name)
        f.close()
        kd.close()
    img.close()


@pytest.mark.parametrize("K", [k for k in D_K if k >= 31])
@pytest.mark.parametrize("n_splits", [20, 31])
def test_fold_words_train_vs_numpy(K, n_splits):
    """From a SplitDev's training bits: bit 31 | (~train[rank] & the folds' mask) -- what fold_words gives on ShuffleSplit's
    test bits as numpy draws them."""
    from strainscan_amd import l2
    img, X, rs = _image(K, 1, 4000)
    mask = np.uint32((1 << n_splits) - 1)
    for name, keep in _keep_patterns(K, rs):
        n_keep = int(keep.sum())
        if not l2.SplitDev.usable(n_keep):
            continue
        split = l2.SplitDev(n_keep, n_splits, 0.5, 0)
        train = split.train_bits()
        kd = l2.DevBuf.from_array(_words(keep, img.W))
        f = img.fold_words_train(kd, split, n_keep)
        got = _dev_u32(f, K)
        assert np.array_equal(got, _fold_expect(keep, ~train & mask)), (K, name)
        test_bits, n_test = l2.shuffle_split_test_bits_numpy(n_keep, n_splits, 0.5, 0)
        assert n_test == split.n_test
        f2 = img.fold_words(kd, test_bits, n_keep)
        assert np.array_equal(got, _dev_u32(f2, K)), (K, name)
        for d in (f, f2, kd):
            d.close()
        split.close()
    img.close()


def test_fold_train_refuses_other_fold_counts():
    from strainscan_amd import _lib, l2
    img, X, rs = _image(129, 1, 5000)
    keep = np.ones(129, bool)
    kd = l2.DevBuf.from_array(_words(keep, img.W))
    split = l2.SplitDev(129, 20, 0.5, 0)
    f = l2.DevBuf(129 * 4)
    for n_splits in (0, 32):
        assert _lib.lib().ss_l2_fold_train(img._h, kd.ptr, split.wait(), 129, n_splits, f.ptr) == _lib.SS_EINVAL
    assert _lib.lib().ss_l2_fold_train(img._h, kd.ptr, split.wait(), 129, 20, f.ptr) == _lib.SS_OK
    for d in (f, kd):
        d.close()
    split.close()
    img.close()


@pytest.mark.parametrize("K", [129, 4097])
def test_fold_words_into_pattern_stats(K):
    """fold_words' output fed to pattern_stats for p = 3: per fold the {count, sum y, sum y^2} table of the kept rows in its
    test half, and the table of all kept rows -- the chain enet_cv_fit relies on -- against enetmodel.stats_from_rows."""
    from strainscan_amd import l2
    n_folds, p = 20, 3
    img, X, rs = _image(K, 5, 6000)
    cols = np.array([4, 0, 2], np.uint32)
    keep = rs.random_sample(K) < 0.7
    keep[K - 1] = True
    n_keep = int(keep.sum())
    bits, _ = l2.shuffle_split_test_bits_numpy(n_keep, n_folds, 0.5, 0)
    y = rs.poisson(12, K).astype(np.int64)
    y[rs.randint(0, K, 5)] = 3_000_000
    y[~keep] = 0                                                 # (ykeep of ClusterImage.prepare)
    kd = l2.DevBuf.from_array(_words(keep, img.W))
    f = img.fold_words(kd, bits, n_keep)
    yd = img.u32(y)
    got = img.pattern_stats(cols, yd, f, n_folds)
    row_bits = np.zeros(K, np.uint32)
    row_bits[keep] = bits
    for fo in range(n_folds):
        sel = keep & (((row_bits >> np.uint32(fo)) & 1) == 1)
        assert np.array_equal(got[fo], em.stats_from_rows(X[:, cols], y, sel, p)), (K, fo)
    assert np.array_equal(got[n_folds], em.stats_from_rows(X[:, cols], y, keep, p))
    for d in (f, kd, yd):
        d.close()
    img.close()
