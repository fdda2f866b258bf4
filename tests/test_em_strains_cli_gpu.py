"""`strainscan --classify_strains 1 --em_strains B --bootstrap_seed 7` on the mid-size database and its M_mix sample (the inputs of
tests/test_classify_strains_cli_gpu.py).

strain_em.tsv is held to the model: tests/strain_set_model.py gives every read its set from the StrainVote.report files the run
wrote and each cluster's matrix and k-mers, tests/boot_model.py the weight of every read in every replicate, tests/em_model.py the EM
on the B + 1 count vectors and the table.  Names and integers are equal; the floating columns are compared after parsing, within
the tolerance of tests/test_em_sets_gpu.py (64 times the model's own difference between two orders of summation, here taken on this
file's vectors with the command's tol = 1e-9, which bounds rho by 1e-8 as that file states) plus half a unit of the last printed
digit.  The abundance is a ratio, theta_j = a_j / sum a_i with a_i = rho_i / kmers_i: an error of t in every rho moves it by at most
(|da_j| + theta_j sum |da_i|) / sum a <= 2 L t kmax / kmin (sum a >= 1 / kmax, |da_i| <= t / kmin), which is the bound used for the
three abundance columns; an order statistic of the replicates moves by no more than its values do.  With B = 0 the interval
columns are `-`; without the flag nothing new runs and every other output is byte for byte the same; strainscan-multi writes under
OUT/<label>/; with --pairs reads_assigned is that run's strain_classes.tsv total."""
import os
import pickle

import numpy as np
import pytest

from tests import em_model as em, rs_model, strain_set_model as sm
from tests.test_extract_cli_gpu import _files, _ok, _result_lines, _run, _with_cache, pair      # noqa: F401

pytestmark = pytest.mark.gpu

M, B, SEED = 1, 20, 7
EM_FILE, CLASSES = "strain_em.tsv", "strain_classes.tsv"
HEAD = "table\tstrain\tkmers\treads_assigned\treads_em\tfrac_reads\tabundance\tabundance_lo\tabundance_hi\tpresent\tenet_frac\titerations"


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def runs(L, mid_dbs, pair, tmp_path_factory):
    """name -> (err, stdout, stderr, out dir, strain_sets_resampled calls made, em_strain_sets calls made)"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("em_cli")
    cs = ["--classify_strains", str(M)]

    def go():
        out = {}
        for name, extra in (("plain", []), ("classes", cs), ("b20", cs + ["--em_strains", str(B), "--bootstrap_seed", str(SEED)]),
                            ("b20_again", cs + ["--em_strains", str(B), "--bootstrap_seed", str(SEED)]), ("b0", cs + ["--em_strains", "0"]),
                            ("pairs", cs + ["--em_strains", "2", "--pairs"])):
            before = L.strain_sets_resampled_calls(), L.em_strain_sets_calls()
            od = str(root / name)
            err, _, text, errs = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od] + extra)
            out[name] = (err, text, errs, od, L.strain_sets_resampled_calls() - before[0], L.em_strain_sets_calls() - before[1])
        return out
    return _with_cache(root, go)


def _report_rows(report):
    rows = [ln.split("\t") for ln in open(report).read().split("\n")[1:] if ln.strip()]
    return [(int(r[0]), r[1], r[3]) for r in rows]


_MODEL = {}


def _model(L, db_dir, out_dir, pair, b):
    """-> (the rows of em_model.em_table, {cluster: the [b + 1, 1 << n] count vectors}) from the reports in out_dir"""
    if (out_dir, b) in _MODEL:
        return _MODEL[out_dir, b]
    import scipy.sparse as sp
    texts = [b"".join(s + b"\n" for _, s in pair["recs"][m]) for m in range(2)]
    order = [ln.split("\t")[0] for ln in open(os.path.join(out_dir, CLASSES)).read().split("\n")[1:] if ln and ln.split("\t")[1] == "unassigned"]
    clusters, vectors = [], {}
    for cls in order:                                                 # clusters in the order they were scanned
        rows = _report_rows(os.path.join(out_dir, cls, "StrainVote.report"))
        called = [(n, name) for n, name, _ in rows]
        n = len(called)
        cdir = os.path.join(db_dir, "Kmer_Sets_L2", "Kmer_Sets", cls)
        with open(os.path.join(cdir, "id2strain_re.pkl"), "rb") as f:
            sid = pickle.load(f)
        col_of = {name: c for c, name in (sid.items() if isinstance(sid, dict) else enumerate(sid))}
        dense = np.asarray(sp.load_npz(os.path.join(cdir, "all_strains_re.npz")).todense())
        masks = np.zeros(dense.shape[0], np.uint16)
        for j, (_, name) in enumerate(called):
            masks |= ((dense[:, col_of[name]] != 0).astype(np.uint16) << np.uint16(j))
        with open(os.path.join(cdir, "all_kmer.fasta"), "rb") as f:
            kmers = [km.upper() for km in rs_model.kmers_of_fasta(f.read())]
        keys = rs_model.encode_kmers(kmers, 31)
        vec = np.zeros((b + 1, 1 << n), np.uint64)
        kmers_of = None
        for t in texts:
            r = sm.classify_strains_model(t, keys, masks, n, 31, M)
            kmers_of = r["kmers"][1:]
            vec[0] += r["set_reads"]
            if b:
                vec[1:] += em.replicate_set_counts(L, t, r["sets"], n, SEED, 0, b)
        clusters.append((cls, called, [int(x) for x in kmers_of], [frac for _, _, frac in rows], vec))
        vectors[cls] = vec
    _MODEL[out_dir, b] = (em.em_table(clusters, b), vectors, clusters)
    return _MODEL[out_dir, b]


def _tolerance(clusters):
    """64 D on this file's vectors at the command's max_iter and tol, and tol's own bound on rho"""
    d = 0.0
    for _, called, _, _, vec in clusters:
        counts, masks = em.compact(vec)
        if masks.size:
            up, _ = em.em_batch(counts, masks, len(called), 1000, 1e-9)
            down, _ = em.em_batch(counts, masks, len(called), 1000, 1e-9, descending=True)
            d = max(d, float(np.abs(up - down).max()))
    return max(64 * d, 1e-8)


def _parse(text):
    lines = text.split("\n")
    assert lines[0] == HEAD and lines[-1] == ""
    return [ln.split("\t") for ln in lines[1:-1]]


def _hold_to_model(got, want, tol, b, clusters):
    assert len(got) == len(want) and len(got) >= 2
    ratio = {}
    for cls, called, kmers, _, _ in clusters:
        pos = [k for k in kmers if k > 0]
        ratio[cls] = 2.0 * len(called) * max(pos) / min(pos) if pos else 1.0
    for g_, w in zip(got, want):
        t_tol = tol * ratio[w[0].split(".")[0]]
        assert len(g_) == 12
        assert g_[0] == w[0] and g_[1] == w[1] and int(g_[2]) == w[2] and int(g_[3]) == w[3] and g_[10] == w[10], (g_, w)
        n_reads = max(w[3], 1)
        assert abs(float(g_[4]) - w[4]) <= tol * n_reads + 0.0005 + 1e-9, (g_, w)
        assert abs(float(g_[5]) - w[5]) <= tol + 0.5e-6 + 1e-12 and abs(float(g_[6]) - w[6]) <= t_tol + 0.5e-6 + 1e-12, (g_, w)
        assert abs(int(g_[11]) - w[11]) <= 1, (g_, w)
        if b:
            assert abs(float(g_[7]) - w[7]) <= t_tol + 0.5e-6 + 1e-12 and abs(float(g_[8]) - w[8]) <= t_tol + 0.5e-6 + 1e-12, (g_, w)
            assert int(g_[9]) == w[9] and float(g_[7]) <= float(g_[8])
        else:
            assert g_[7:10] == ["-", "-", "-"]


def test_the_file_is_the_models(L, runs, mid_dbs, pair):
    err, _, errs, od, rcalls, ecalls = runs["b20"]
    assert _ok(err), err
    want, vectors, clusters = _model(L, mid_dbs["DB_M"]["db_dir"], od, pair, B)
    text = open(os.path.join(od, EM_FILE)).read()
    print(text)
    tol = _tolerance(clusters)
    print("tolerance on rho", tol)
    _hold_to_model(_parse(text), want, tol, B, clusters)
    # what keeps this from passing vacuously: a cluster with two called strains, a tie with reads, replicates that differ
    two = [c for c in clusters if len(c[1]) >= 2]
    assert two and any(int(c[4][0, 3]) > 0 for c in two)
    assert all(len({v.tobytes() for v in c[4][1:]}) > 1 for c in two)
    # B = 20 is one call of 16 and one of 4 per cluster, and one EM launch per cluster
    assert rcalls == 2 * len(clusters) and ecalls == len(clusters)
    lines = [ln for ln in errs.split("\n") if ln.startswith("em_strains:")]
    assert sorted(ln.split("\t")[0].split(" ")[1] for ln in lines) == sorted(c[0] for c in clusters), lines
    assert all(ln.split("\t")[1:3] == ["B=%d" % B, "seed=%d" % SEED] and ln.split("\t")[6] == "replicates at max_iter 0" for ln in lines), lines
    assert open(os.path.join(runs["b20_again"][3], EM_FILE)).read() == text      # the same file on a second run


def test_b_0_gives_the_estimate_alone(L, runs, mid_dbs, pair):
    err, _, errs, od, rcalls, ecalls = runs["b0"]
    assert _ok(err), err
    want, _, clusters = _model(L, mid_dbs["DB_M"]["db_dir"], od, pair, 0)
    got = _parse(open(os.path.join(od, EM_FILE)).read())
    _hold_to_model(got, want, _tolerance(clusters), 0, clusters)
    assert rcalls == 0 and ecalls == len(clusters)
    full = _parse(open(os.path.join(runs["b20"][3], EM_FILE)).read())
    assert [r[:7] + r[10:] for r in got] == [r[:7] + r[10:] for r in full]      # the estimate does not depend on B


def test_flag_off_runs_nothing_and_changes_nothing(runs):
    e0, t0, errs0, d0, r0, c0 = runs["plain"]
    e1, t1, errs1, d1, r1, c1 = runs["classes"]
    assert _ok(e0) and _ok(e1) and (r0, c0, r1, c1) == (0, 0, 0, 0)
    assert not [ln for ln in (errs0 + errs1).split("\n") if ln.startswith("em_strains:")]
    a = _files(d1)
    assert EM_FILE not in a and CLASSES in a and EM_FILE not in _files(d0)
    for name in ("b20", "b0"):
        e2, t2, _, d2, r2, c2 = runs[name]
        assert _ok(e2) and type(e2) is type(e1) and c2 > 0
        b = _files(d2)
        assert EM_FILE in b
        b.pop(EM_FILE)
        assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a), name      # every other file byte for byte
        assert t1 == t2 or _result_lines(t1) == _result_lines(t2)
    assert _result_lines(t0) == _result_lines(t1) and _result_lines(t0)


def test_pairs_count_fragments(runs):
    err, _, errs, od, rcalls, ecalls = runs["pairs"]
    assert _ok(err), err
    got = _parse(open(os.path.join(od, EM_FILE)).read())
    classes = [ln.split("\t") for ln in open(os.path.join(od, CLASSES)).read().split("\n")[1:] if ln]
    for cls in sorted({r[0].split(".")[0] for r in got}):
        mine = [r for r in classes if r[0].split(".")[0] == cls]
        unassigned = int([r for r in mine if r[1] == "unassigned"][0][4])
        total = round(sum(float(r[6]) for r in mine))                 # a cluster's reads_share column sums to the fragments
        assigned = {int(r[3]) for r in got if r[0].split(".")[0] == cls}
        assert assigned == {total - unassigned} and total - unassigned > 0, (cls, assigned, total, unassigned)
    single = _parse(open(os.path.join(runs["b0"][3], EM_FILE)).read())
    assert [r[3] for r in got] != [r[3] for r in single]            # fragments, not mates
    assert rcalls > 0 and ecalls > 0


def test_multi_db_writes_under_each_label(L, runs, mid_dbs, pair, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbm, dbmem = mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]
    od = str(tmp_path / "flag")
    e1, rc1, _, _ = _run(multi_db.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", dbm, "-d", "mem=" + dbmem, "-o", od,
                                         "--classify_strains", str(M), "--em_strains", str(B), "--bootstrap_seed", str(SEED)])
    assert e1 is None and rc1 == 0
    want = open(os.path.join(runs["b20"][3], EM_FILE)).read()
    # the two databases hold the same genomes: each label's file is the single run's, which the model has checked
    for label in (os.path.basename(os.path.normpath(dbm)), "mem"):
        assert open(os.path.join(od, label, EM_FILE)).read() == want, label
    assert not os.path.exists(os.path.join(od, EM_FILE))


def test_sample_not_resident_says_so_once(L, runs, mid_dbs, pair, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    from strainscan_amd import db as ssdb
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    monkeypatch.setattr(ssdb, "RESIDENT_LIMIT_BYTES", 0)
    before = L.em_strain_sets_calls()
    od = str(tmp_path / "out")
    err, _, text, errs = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od,
                                                "--classify_strains", str(M), "--em_strains", "2"])
    lines = [ln for ln in errs.split("\n") if ln.startswith("em_strains:")]
    assert len(lines) == 1 and "resident on the device" in lines[0], lines
    assert _ok(err) and L.em_strain_sets_calls() == before and EM_FILE not in _files(od)
    assert _result_lines(runs["plain"][1]) == _result_lines(text)
