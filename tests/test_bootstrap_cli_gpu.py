"""`strainscan --bootstrap 8 --bootstrap_seed 3` on the mid-size database and its M_mix pair (two strains of C7, three of C19, one
of C23, a singleton).

The replicate coefficients (read_reports.bootstrap_replicates) equal a model that never touches the device: the reads resampled in Python
with the weight model (tests/boot_model.py), counted by the CPU oracle, and solved by the oracle's pre-scan / elastic net with the
main solve's columns and alpha held fixed -- to the project's abundance tolerance, 1e-5 relative (|got - want| <= 1e-5 * max(1,
|want|), as the reports' depths are compared elsewhere).  strain_bootstrap.tsv is the writer applied to them; every other output is
that of the run without the flag; the file is the same under strainscan-multi, on two ranks, with the reads in file order and from
a BAM of the same reads; where it cannot run one line says why."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import boot_model
from tests import scenarios as sc
from tests.test_extract_cli_gpu import REPO, WORKER, _files, _ok, _result_lines, _run, _with_cache, pair      # noqa: F401

pytestmark = pytest.mark.gpu

B, SEED = 8, 3
TSV = "strain_bootstrap.tsv"
TOL = 1e-5
FLAGS = ["--bootstrap", str(B), "--bootstrap_seed", str(SEED)]


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _others(d):
    return {k: v for k, v in _files(d).items() if os.path.basename(k) != TSV}


class _Spy:
    """records what layer 1 hands to layer 2 (detect_strains' arguments, per cluster) and the replicates just before the command
    drops them"""

    def __init__(self):
        from strainscan_amd import Vote_Strain_L2_Lasso_new_sp as vote
        from strainscan_amd import read_reports
        self.vote, self.ssdb = vote, read_reports
        self.args, self.replicates = {}, {}

    def __enter__(self):
        self.mod = self.vote.identify_strains_L2_Enet_Pscan_new_sp
        self.detect, self.write = self.mod.detect_strains, self.ssdb.write_bootstrap

        def detect(input_csv, input_y, ids, ksize, npp25, npp75, npp_out, cls_cov, omatrix, all_cls, l2, msn, pmode, emode):
            self.args[os.path.basename(os.path.dirname(input_csv))] = dict(
                y=np.array(input_y).copy(), ksize=int(ksize), npp25=npp25, npp75=npp75, npp_out=npp_out, all_cls=list(all_cls), l2=l2, msn=msn,
                pmode=pmode, emode=emode)
            return self.detect(input_csv, input_y, ids, ksize, npp25, npp75, npp_out, cls_cov, omatrix, all_cls, l2, msn, pmode, emode)

        def write(out_dir, scope=None):
            self.replicates[scope] = self.ssdb.bootstrap_replicates(scope)
            return self.write(out_dir, scope)

        self.mod.detect_strains, self.ssdb.write_bootstrap = detect, write
        return self

    def __exit__(self, *exc):
        self.mod.detect_strains, self.ssdb.write_bootstrap = self.detect, self.write


@pytest.fixture(scope="module")
def runs(L, mid_dbs, pair, tmp_path_factory):
    """`strainscan` on DB_M with the pair, without and with the flag -> name: (err, stdout, stderr, out dir, resample calls made),
    and "spy": what the run with the flag handed to layer 2 and its replicates"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("boot_cli")

    def go():
        out = {}
        with _Spy() as spy:
            for name, extra in (("plain", []), ("flag", FLAGS)):
                before = L.resample_calls()
                od = str(root / name)
                err, _, text, errs = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od]
                                          + extra)
                out[name] = (err, text, errs, od, L.resample_calls() - before)
        out["spy"] = spy
        return out
    return _with_cache(root, go)


_MODEL = {}


def _model(L, db_dir, spy, pair):
    """{cluster: (strain names in pre-scan order, float64[B, p])} from the files of the database and the reads' bytes alone"""
    if _MODEL:
        return _MODEL
    import scipy.sparse as sp
    from oracle import oracle as orc
    recs = [r for m in range(2) for r in pair["recs"][m]]
    keys = L.flat_record_keys(b"".join(s + b"\n" for _, s in recs))
    assert keys.shape == (len(recs), 2)
    fq_b = []
    for rep in range(B):
        w = boot_model.weights_of_keys(keys[:, 1], SEED, rep)
        fq_b.append(b"".join(t * int(n) for (t, _), n in zip(recs, w.tolist())))
    for cls, a in sorted(spy.args.items()):
        cd = os.path.join(db_dir, "Kmer_Sets_L2", "Kmer_Sets", cls)
        kfa = open(os.path.join(cd, "all_kmer.fasta"), "rb").read()
        X = sp.load_npz(os.path.join(cd, "all_strains_re.npz")).toarray().astype(np.int64)
        om = sp.load_npz(os.path.join(cd, "overlap_matrix.npz")).toarray().astype(np.int64)[:, [int(c - 1) for c in a["all_cls"]]]
        sid = pickle.load(open(os.path.join(cd, "id2strain_re.pkl"), "rb"))
        ln = om.sum(axis=1)
        ln[ln > 1] = 0
        # the main solve, by the oracle: the columns in pre-scan order and the alpha
        y = a["y"].astype(np.int64)
        cols, names, _, _, _, _ = orc.prescan(X, y, y * ln, sid, a["msn"] * a["ksize"], a["l2"], a["pmode"], a["emode"])
        alpha = None
        if len(cols) > 1:
            keep = ~((y < a["npp25"]) | (y > a["npp75"]) | (y > a["npp_out"]))
            alphas, mse = orc.enet_cv(X[keep][:, cols], y[keep])
            alpha, _, _ = orc.lasso_mpm(alphas, mse)
        coefs = np.zeros((B, len(cols)))
        for rep in range(B):
            counts, _ = orc.jellyfish_count(kfa, [fq_b[rep]], k=a["ksize"], upper=False)
            yb = np.asarray(counts, np.int64).copy()
            yb[yb == 1] = 0
            if len(cols) == 1:
                yu = yb * ln
                yy = yu if yu.sum() > 0 else yb
                coefs[rep, 0] = orc.get_avg_depth(cols[0], X, yy) if np.count_nonzero(X[:, cols[0]] * yy) else 0.0
            else:
                keep = ~((yb < a["npp25"]) | (yb > a["npp75"]) | (yb > a["npp_out"]))
                if keep.any():
                    coefs[rep] = orc.enet_fit(X[keep][:, cols], yb[keep], alpha)
        _MODEL[cls] = ([str(n) for n in names], coefs)
    return _MODEL


def test_replicates_are_the_models_and_the_file_is_the_writer(L, runs, mid_dbs, pair):
    from strainscan_amd import read_reports
    err, _, errs, od, calls = runs["flag"]
    assert _ok(err), err
    assert "bootstrap:" not in errs
    got = runs["spy"].replicates[None]
    reports = sorted(c for c in runs["spy"].args if os.path.exists(os.path.join(od, c, "StrainVote.report")))
    assert sorted(got) == reports and len(reports) >= 2
    assert calls == B * len(reports)
    want = _model(L, mid_dbs["DB_M"]["db_dir"], runs["spy"], pair)
    sizes = {}
    for cls in reports:
        names, coefs = got[cls]
        wnames, wcoefs = want[cls]
        print(cls, names, "\n", coefs, "\nmodel\n", wcoefs)
        assert names == wnames and coefs.shape == wcoefs.shape == (B, len(names))
        assert (np.abs(coefs - wcoefs) <= TOL * np.maximum(1.0, np.abs(wcoefs))).all(), (cls, np.abs(coefs - wcoefs).max())
        assert coefs.std(axis=0).max() > 0                           # the replicates are not one solve repeated
        sizes[cls] = len(names)
    assert max(sizes.values()) >= 2 and min(sizes.values()) == 1, sizes      # the elastic net's way and the single strain's both ran
    # the file: the writer on these matrices and the reports' rows, clusters in the order scanned, strains in report order
    text = open(os.path.join(od, TSV)).read()
    print(text)
    lines = text.split("\n")
    assert lines[0] == "table\tstrain\treplicates\tdepth\tdepth_lo\tdepth_hi\tfrac\tfrac_lo\tfrac_hi\tpresent" and lines[-1] == ""
    order = list(dict.fromkeys(ln.split("\t")[0].split(".")[0] for ln in lines[1:-1]))
    assert sorted(order) == reports
    rows = []
    for cls in order:
        names, coefs = got[cls]
        for ln in open(os.path.join(od, cls, "StrainVote.report")).read().split("\n")[1:]:
            f = ln.split("\t")
            if len(f) > 5:
                rows.append(("%s.%s" % (cls, f[0]), f[1], f[4], f[3], names.index(f[1]), coefs))
    assert text == read_reports.bootstrap_text(rows)
    for ln in lines[1:-1]:
        f = ln.split("\t")
        assert f[2] == str(B) and float(f[4]) <= float(f[5]) and float(f[7]) <= float(f[8]) and 0 <= int(f[9]) <= B
    # the first strain of every cluster was sampled at depth 11 and more: no resampling of the reads takes it away
    top = [ln.split("\t") for ln in lines[1:-1] if ln.split("\t")[0].endswith(".1")]
    assert all(int(f[9]) == B for f in top)


def test_other_outputs_are_unchanged_and_flag_off_runs_nothing(runs):
    e0, t0, errs0, d0, calls0 = runs["plain"]
    e1, t1, _, d1, calls1 = runs["flag"]
    assert _ok(e0) and _ok(e1) and type(e0) is type(e1)
    assert calls0 == 0 and calls1 > 0 and "bootstrap" not in errs0
    a, b = _files(d0), _others(d1)
    assert TSV not in a and os.path.exists(os.path.join(d1, TSV))
    assert a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert t0 == t1 or _result_lines(t0) == _result_lines(t1)
    assert _result_lines(t0)
    assert runs["spy"].replicates.get(None) is not None


def test_multi_db_writes_under_each_label(L, runs, mid_dbs, pair, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbm, dbmem = mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]
    od = str(tmp_path / "flag")
    e1, rc1, _, _ = _run(multi_db.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", dbm, "-d", "mem=" + dbmem, "-o", od] + FLAGS)
    assert e1 is None and rc1 == 0
    want = open(os.path.join(runs["flag"][3], TSV)).read()
    for label in (os.path.basename(os.path.normpath(dbm)), "mem"):       # (the two databases hold the same genomes)
        assert open(os.path.join(od, label, TSV)).read() == want, label
    assert not os.path.exists(os.path.join(od, TSV))


def test_reads_in_file_order(runs, mid_dbs, pair, tmp_path, monkeypatch):
    """the weights depend on a read's bytes, not on where binning put it"""
    from strainscan_amd import StrainScan
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    monkeypatch.setenv("SS_READS_ORDER", "file")
    od = str(tmp_path / "out")
    err, _, _, _ = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od] + FLAGS)
    assert _ok(err)
    assert open(os.path.join(od, TSV)).read() == open(os.path.join(runs["flag"][3], TSV)).read()


def test_the_same_reads_as_a_bam(runs, mid_dbs, pair, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    from tests import bamio
    from tests.test_bam_select_gpu import HDR
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    # a BAM holds no lower case, and a read's weight is keyed by its bytes: the FASTQ run to compare with has the reads upper-cased
    rs = np.random.RandomState(5)
    recs, fq = [], ([], [])
    for i, (m1, m2) in enumerate(zip(*pair["recs"])):
        for m, (_, s) in enumerate((m1, m2)):
            s = s.upper()
            recs.append(bamio.record("pair%d" % i, s.decode(), flag=0x1 | (0x40, 0x80)[m],
                                     qual=rs.randint(2, 41, size=len(s)).astype(np.uint8).tobytes()))
            fq[m].append(b"@pair%d/%d\n%s\n+\n%s\n" % (i, m + 1, s, b"I" * len(s)))
    bam = tmp_path / "P.bam"
    bam.write_bytes(bamio.bgzf(HDR, recs, level=6))
    paths = []
    for m in range(2):
        paths.append(str(tmp_path / ("U_R%d.fastq" % (m + 1))))
        open(paths[m], "wb").write(b"".join(fq[m]))
    db_dir = mid_dbs["DB_M"]["db_dir"]
    e1, _, _, _ = _run(StrainScan.main, ["-i", str(bam), "-d", db_dir, "-o", str(tmp_path / "b")] + FLAGS)
    e2, _, _, _ = _run(StrainScan.main, ["-i", paths[0], "-j", paths[1], "-d", db_dir, "-o", str(tmp_path / "f")] + FLAGS)
    assert _ok(e1) and _ok(e2)
    text = open(os.path.join(str(tmp_path / "b"), TSV)).read()
    assert text.count("\n") == open(os.path.join(runs["flag"][3], TSV)).read().count("\n") >= 4
    assert text == open(os.path.join(str(tmp_path / "f"), TSV)).read()


def test_sample_not_resident(L, runs, mid_dbs, pair, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    from strainscan_amd import db as ssdb
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    monkeypatch.setattr(ssdb, "RESIDENT_LIMIT_BYTES", 0)
    before = L.resample_calls()
    od = str(tmp_path / "out")
    err, _, text, errs = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od] + FLAGS)
    lines = [ln for ln in errs.split("\n") if ln.startswith("bootstrap:")]
    assert len(lines) == 1 and "resident on the device" in lines[0] and "no intervals were computed" in lines[0], lines
    e0, t0, _, d0, _ = runs["plain"]
    assert _ok(err) and type(err) is type(e0) and L.resample_calls() == before
    a, b = _files(d0), _files(od)
    assert TSV not in b and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert _result_lines(t0) == _result_lines(text)


def test_only_single_strain_clusters_no_file(L, mid_dbs, tmp_path, monkeypatch):
    """a sample of one singleton cluster: layer 2 solves nothing, and nothing is resampled or written"""
    from strainscan_amd import StrainScan
    from tests import synth
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    info = mid_dbs["DB_M"]
    s0 = info["spec"]["sampled_singletons"][0]
    fq = tmp_path / "single.fq"
    fq.write_bytes(synth.simulate_reads([(info["leaf_genome"][s0], 12.0)], 99))
    before = L.resample_calls()
    od = str(tmp_path / "out")
    err, _, text, errs = _run(StrainScan.main, ["-i", str(fq), "-d", info["db_dir"], "-o", od] + FLAGS)
    assert _ok(err), err
    assert os.path.exists(os.path.join(od, "final_report.txt")) and not os.path.exists(os.path.join(od, TSV))
    assert not [d for d in os.listdir(od) if os.path.exists(os.path.join(od, d, "StrainVote.report"))]
    assert L.resample_calls() == before and "bootstrap:" not in errs


def test_two_ranks_write_the_single_process_file(runs, mid_dbs, pair, tmp_path):
    """Two ranks on one GPU (fresh child processes, gloo, each under its own timeout): each resamples its shard of the reads; the
    weights are keyed by content, so the summed counts -- and the file -- are those of one process."""
    od = str(tmp_path / "out")
    code = WORKER % dict(repo=REPO, seed=sc.POISSON_SEED,
                         argv=["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od] + FLAGS)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", SS_IMAGE_CACHE=str(tmp_path / "cache"),
                   SS_TEST_STORE=str(tmp_path / "store"))
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, "-c", code], env=env, stderr=subprocess.PIPE))
    errs = [p.communicate(timeout=300)[1].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), [e[-3000:] for e in errs]
    assert not [ln for e in errs for ln in e.split("\n") if ln.startswith("bootstrap:")]
    assert open(os.path.join(od, TSV)).read() == open(os.path.join(runs["flag"][3], TSV)).read()
