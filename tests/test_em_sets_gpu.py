"""ss_reads_strain_sets_resampled (ss_strain_sets.hip) and ss_em_strain_sets (ss_em.hip) on the device.

The resampled set counts are held bit for bit to the model -- tests/strain_set_model.py's set of every record, tests/boot_model.py's
weight of every record, added up by tests/em_model.py -- on the cases of tests/em_cases.py (whose conditions
tests/test_em_sets_host.py checks without a device), and on one case to the device's own classify_strains(resample(...)).

The EM is held to tests/em_model.py.  The device adds the sets' terms in another order than the model (a strided share per thread,
a tree within the wave, the waves in turn), so the tolerance is taken from the model itself: D = the largest difference in rho
between the model with the sets added in ascending and in descending order, over all cases below; the device may differ from the
ascending model by 64 D, the margin standing for the tree being a third order.  Measured on one MI355X: D = 1.36e-15, the device's
largest difference 1.10e-15 (profiles/r30_em_strains.md).

Not covered here: the SS_ERANGE of a cut record and of more records than an int holds, and the SS_EINVAL of a table and a set on
different devices, as tests/test_strain_sets_gpu.py says of ss_reads_classify_strains."""
import numpy as np
import pytest

from tests import class_cases as cc, em_cases as ec, em_model as em, strain_set_cases as sc, strain_set_model as sm
from tests.test_strain_sets_gpu import L, g, read_sets      # noqa: F401 -- the read-set shapes of the strain-set tests

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tables(L, g):
    """table name of strain_set_cases -> (KmerDB, k, row_sets of every row, keys and sets of the rows with a slot), masks uncut"""
    out = {}
    for name in sorted({v[0] for v in ec.TABLES.values()}):
        k, _, kmers, row_sets, keys, vsets = sc.table(name, g)
        db = L.KmerDB.from_text(cc.kfa(kmers), k, True)
        if sc.TABLES[name][2]:
            db.expect_hits(True)
        out[name] = (db, k, row_sets, keys, vsets)
    yield out
    for t in out.values():
        t[0].close()


def _table(tables, tkey):
    tname, n = ec.TABLES[tkey]
    db, k, row_sets, keys, vsets = tables[tname]
    row_sets, vsets = ec.cut(row_sets, vsets, n)
    return db, k, n, row_sets, keys, vsets


_SETS = {}


def _model_sets(tables, read_sets, tkey, sname, m):
    """the model's set of every record of one (table, set, M), once"""
    if (tkey, sname, m) not in _SETS:
        _, k, n, _, keys, vsets = _table(tables, tkey)
        _SETS[tkey, sname, m] = sm.classify_strains_model(read_sets[sname][1], keys, vsets, n, k, m)
    return _SETS[tkey, sname, m]


@pytest.mark.parametrize("case", ec.RESAMPLED, ids=lambda c: "%s-%s-M%d" % c[:3])
def test_resampled_set_counts_equal_the_model(L, tables, read_sets, case):
    tkey, sname, m, reps, seeds = case
    db, k, n, row_sets, keys, vsets = _table(tables, tkey)
    rset, text = read_sets[sname]
    want_sets = _model_sets(tables, read_sets, tkey, sname, m)
    total = 0
    for seed in seeds:
        for first, n_rep in reps:
            calls, ccalls = L.strain_sets_resampled_calls(), L.classify_strains_calls()
            got = rset.strain_sets_resampled(db, row_sets, n, m, seed, first, n_rep)
            assert L.strain_sets_resampled_calls() == calls + 1 and L.classify_strains_calls() == ccalls
            want = em.replicate_set_counts(L, text, want_sets["sets"], n, seed, first, n_rep)
            assert got.dtype == np.uint64 and got.shape == (n_rep, 1 << n)
            assert (got == want).all(), (seed, first, n_rep, np.argwhere(got != want)[:5])
            total += int(got.sum())
    print(tkey, sname, "M", m, "weights added", total)
    if sname == "empty":
        assert total == 0
    elif sname != "long":
        assert total > 0


def test_resampled_equals_classifying_the_resampled_set(L, tables, read_sets):
    db, k, n, row_sets, _, _ = _table(tables, "n12")
    rset = read_sets["ragged_1"][0]
    got = rset.strain_sets_resampled(db, row_sets, n, 2, 20, 3, 5)
    for j in range(5):
        sub = rset.resample(20, 3 + j)
        try:
            want = sub.classify_strains(db, row_sets, n, 2)["set_reads"]
        finally:
            sub.close()
        assert (got[j] == want).all() and int(want[1:].sum()) > 0, j


def test_shards_add_up_and_layouts_agree(L, tables, read_sets):
    for tkey, reps in (("n12", (16, 4)), ("n13", (0, 16))):
        db, k, n, row_sets, _, _ = _table(tables, tkey)
        r = {s: read_sets[s][0].strain_sets_resampled(db, row_sets, n, 1, 7, *reps) for s in ("packed", "file_order", "half_a", "half_b")}
        assert (r["half_a"] + r["half_b"] == r["packed"]).all() and (r["file_order"] == r["packed"]).all()
        assert int(r["half_a"].sum()) > 0 and int(r["half_b"].sum()) > 0


def test_resampled_leaves_the_counters_alone(L, tables, read_sets):
    db, k, n, row_sets, _, _ = _table(tables, "n16")
    rset = read_sets["packed"][0]
    db.reset()
    rset.scan_into(db)
    L.check(L.lib().ss_device_sync(), "sync")
    before = db.counts_rows().copy()
    rset.strain_sets_resampled(db, row_sets, n, 1, 7, 0, 16)
    rset.strain_sets_resampled(db, row_sets, n, 1, 7, 0, 1)
    assert (db.counts_rows() == before).all() and int(before.sum()) > 0
    db.reset()


def test_resampled_argument_errors(L, g, tables, read_sets):
    rset = read_sets["packed"][0]
    db, k, n, row_sets, _, _ = _table(tables, "n13")
    out = np.zeros((16, 1 << 16), np.uint64)

    def raw(row=row_sets, n_strains=n, m=1, first=0, n_rep=2, skip=None):
        args = dict(db=db.handle, r=rset._h, row=L.ptr(row), out=L.ptr(out))
        if skip:
            args[skip] = None
        return L.lib().ss_reads_strain_sets_resampled(args["db"], args["r"], args["row"], n_strains, m, 7, first, n_rep, args["out"])

    calls = L.strain_sets_resampled_calls()
    assert raw() == 0 and L.strain_sets_resampled_calls() == calls + 1
    for skip in ("db", "r", "row", "out"):
        assert raw(skip=skip) == L.SS_EINVAL, skip
    assert raw(m=0) == L.SS_EINVAL
    assert raw(n_strains=0) == L.SS_EINVAL and raw(n_strains=17) == L.SS_EINVAL
    assert raw(n_strains=n - 1) == L.SS_EINVAL                        # a mask bit at or above n_strains
    assert raw(n_rep=0) == L.SS_EINVAL and raw(n_rep=17) == L.SS_EINVAL
    assert raw(n_rep=16, n_strains=16) == 0                           # both caps are served
    assert L.strain_sets_resampled_calls() == calls + 2
    k15m = list(dict.fromkeys(g[i:i + 15] for i in range(0, 5000, 5)))
    k15 = L.KmerDB.from_text(cc.kfa(k15m), 15, True)
    try:
        with pytest.raises(L.SSError) as e:
            rset.strain_sets_resampled(k15, np.ones(len(k15m), np.uint16), 2, 1, 7, 0, 4)      # a flat table
        assert e.value.code == L.SS_ERANGE
    finally:
        k15.close()
    assert L.strain_sets_resampled_calls() == calls + 2


# ss_em_strain_sets -----------------------------------------------------------------------------------------------------------
CAP = 6144      # SS_EM_LDS_SETS
# name -> (n_strains, n_sets, n_vec, the max_iter values)
EM_CASES = {
    "one_strain": (1, 1, 1, (1, 7, 200)),
    "two_strains_all_sets": (2, 3, 3, (1, 7, 200)),
    "sets_63_vec_1024": (16, 63, 1024, (1, 7)),
    "sets_64": (16, 64, 3, (1, 7, 200)),
    "sets_65": (16, 65, 3, (1, 7, 200)),
    "sets_cap": (16, CAP, 3, (1, 7, 200)),
    "sets_cap_plus_1": (16, CAP + 1, 3, (1, 7, 200)),
    "sets_65535": (16, 65535, 3, (1, 7)),
    "by_hand": (2, 3, 6, (1, 7, 200)),
}
BY_HAND_MASKS = [1, 2, 3]
# a mixed vector, nothing at all, strain 2 losing every read to strain 1 (underflow), singletons only, the issue's 30 / 10 / 60,
# and a tie alone
BY_HAND = [[700, 5, 300], [0, 0, 0], [1000, 0, 1], [30, 10, 0], [30, 10, 60], [0, 0, 9]]


def _em_input(name):
    n_strains, n_sets, n_vec, _ = EM_CASES[name]
    if name == "by_hand":
        return np.array(BY_HAND, np.uint64), np.array(BY_HAND_MASKS, np.uint16)
    rng = np.random.RandomState(sum(name.encode()))
    counts, masks = ec.em_vectors(rng, n_vec, n_sets, n_strains)
    if not counts[0].any():
        counts[0, 0] = 5
    if n_vec >= 3:
        counts[1] = 0                                                 # one all-zero vector among the others
    return counts, masks


@pytest.fixture(scope="module")
def em_models():
    """name, max_iter -> (counts, masks, rho ascending, iters, rho descending); and D, the largest difference between the orders"""
    out, d = {}, 0.0
    for name, (n_strains, _, _, iters) in EM_CASES.items():
        counts, masks = _em_input(name)
        for mi in iters:
            up, it = em.em_batch(counts, masks, n_strains, mi, 0.0)
            down, it2 = em.em_batch(counts, masks, n_strains, mi, 0.0, descending=True)
            assert (it == it2).all() and not np.isnan(up).any()
            out[name, mi] = (counts, masks, up, it, down)
            d = max(d, float(np.abs(up - down).max()))
    assert 0.0 < d < 1e-12
    return out, d


_EM_SEEN = {"device": 0.0}


@pytest.mark.parametrize("name,max_iter", [(n, mi) for n, v in EM_CASES.items() for mi in v[3]])
def test_em_equals_the_model(L, em_models, name, max_iter):
    models, d = em_models
    counts, masks, want, want_it, _ = models[name, max_iter]
    n_strains = EM_CASES[name][0]
    calls = L.em_strain_sets_calls()
    rho, iters = L.em_strain_sets(counts, masks, n_strains, max_iter, 0.0)
    assert L.em_strain_sets_calls() == calls + 1
    assert rho.dtype == np.float64 and rho.shape == want.shape and iters.dtype == np.uint32
    assert not np.isnan(rho).any()
    assert iters.tolist() == want_it.tolist()                         # tol == 0: exactly max_iter, 0 for a vector without reads
    diff = float(np.abs(rho - want).max())
    _EM_SEEN["device"] = max(_EM_SEEN["device"], diff)
    print(name, "max_iter", max_iter, "D", d, "64 D", 64 * d, "device - model", diff, "largest so far", _EM_SEEN["device"])
    assert diff <= 64 * d
    has = counts.sum(axis=1) > 0
    assert (np.abs(rho[has].sum(axis=1) - 1.0) < 1e-9).all() and not rho[~has].any()
    again, iters2 = L.em_strain_sets(counts, masks, n_strains, max_iter, 0.0)
    assert again.tobytes() == rho.tobytes() and iters2.tobytes() == iters.tobytes()      # the same bits on every run
    if name == "by_hand":
        assert not rho[1].any() and iters[1] == 0                     # nothing at all
        assert rho[5].tolist() == [0.5, 0.5]                          # a tie alone stays where it starts
        ulp = np.abs(rho[3] - want[3]) / np.spacing(want[3])
        print("singletons only: ulps", ulp)
        assert (ulp <= 4).all() and np.abs(rho[3] - np.array([0.75, 0.25])).max() < 1e-15
        if max_iter == 200:
            assert rho[2].tolist() == [1.0, 0.0]                      # through the denormals down to 0, and no NaN on the way
            assert np.abs(rho[4] - np.array([0.75, 0.25])).max() < 1e-9


def test_em_stops_by_itself(L):
    counts, masks = np.array(BY_HAND, np.uint64), np.array(BY_HAND_MASKS, np.uint16)
    rng = np.random.RandomState(5)
    stopped = 0
    for c, k, n in ((counts, masks, 2),) + tuple(ec.em_vectors(rng, 4, s, 16) + (16,) for s in (65, CAP + 1)):
        want, want_it = em.em_batch(c, k, n, 1000, 1e-9)
        rho, iters = L.em_strain_sets(c, k, n, 1000, 1e-9)
        print("iters", iters.tolist(), "model", want_it.tolist(), "largest difference", float(np.abs(rho - want).max()))
        assert (np.abs(iters.astype(np.int64) - want_it.astype(np.int64)) <= 1).all()
        assert float(np.abs(rho - want).max()) <= 1e-8
        stopped += int(((iters > 1) & (iters < 1000)).sum())
    assert stopped >= 3                                               # (a flat likelihood may well take all 1000 iterations)


def test_em_argument_errors(L):
    counts, masks = np.array(BY_HAND, np.uint64), np.array(BY_HAND_MASKS, np.uint16)
    rho, iters = np.zeros((1024, 16)), np.zeros(1024, np.uint32)
    big = np.zeros(2 * 65536, np.uint64)
    many = np.arange(1, 65537).astype(np.uint16)

    def raw(c=counts, k=masks, n_sets=3, n_strains=2, n_vec=6, max_iter=5, tol=0.0, skip=None):
        args = dict(c=L.ptr(c), k=L.ptr(k), rho=L.ptr(rho), iters=L.ptr(iters))
        if skip:
            args[skip] = None
        return L.lib().ss_em_strain_sets(args["c"], args["k"], n_sets, n_strains, n_vec, max_iter, tol, args["rho"], args["iters"])

    calls = L.em_strain_sets_calls()
    assert raw() == 0 and L.em_strain_sets_calls() == calls + 1
    for skip in ("c", "k", "rho", "iters"):
        assert raw(skip=skip) == L.SS_EINVAL, skip
    assert raw(n_sets=0) == L.SS_EINVAL
    assert raw(c=big, k=many, n_sets=65536, n_strains=16, n_vec=1) == L.SS_EINVAL
    assert raw(n_strains=0) == L.SS_EINVAL and raw(n_strains=17) == L.SS_EINVAL
    assert raw(n_vec=0) == L.SS_EINVAL and raw(c=big, n_vec=1025) == L.SS_EINVAL
    assert raw(c=big, n_vec=1024) == 0                                # the cap itself is served
    assert raw(max_iter=0) == L.SS_EINVAL
    assert raw(tol=-1.0) == L.SS_EINVAL and raw(tol=float("nan")) == L.SS_EINVAL
    assert raw(k=np.array([1, 0, 3], np.uint16)) == L.SS_EINVAL       # a zero mask
    assert raw(k=np.array([1, 3, 3], np.uint16)) == L.SS_EINVAL       # a mask listed twice
    assert raw(k=np.array([1, 2, 4], np.uint16)) == L.SS_EINVAL       # a bit at or above n_strains
    assert raw(k=np.array([1, 2, 4], np.uint16), n_strains=3) == 0
    assert L.em_strain_sets_calls() == calls + 3
    with pytest.raises(ValueError):
        L.em_strain_sets(counts, masks[:2], 2, 5, 0.0)
