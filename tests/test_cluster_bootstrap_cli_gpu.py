"""`strainscan --bootstrap_clusters 4 --bootstrap_seed 7` on the mid-size database and its M_mix sample.

Replicate b of read_reports.cluster_bootstrap_replicates() equals, exactly, what the flag-off identify_with_ladder returns on a
materialised replicate -- the FASTQ with every read as often as tests/boot_model.py's weight says -- because the counts are
bit-equal (tests/test_scan_resampled_gpu.py) and the walk is deterministic once numpy's generator is seeded as
read_reports.cluster_bootstrap_walk_seed says.  cluster_bootstrap.tsv is the writer applied to them; every other output is that of
the run without the flag; with --pairs a fragment draws one weight; where it cannot run one line says why."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import boot_model, pairs_model
from tests import scenarios as sc
from tests.test_extract_cli_gpu import REPO, WORKER, _files, _ok, _result_lines, _run, _with_cache, pair      # noqa: F401

pytestmark = pytest.mark.gpu

B, SEED = 4, 7
TSV = "cluster_bootstrap.tsv"
FLAGS = ["--bootstrap_clusters", str(B), "--bootstrap_seed", str(SEED)]


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _others(d):
    return {k: v for k, v in _files(d).items() if os.path.basename(k) != TSV}


def _lines(errs):
    return [ln for ln in errs.split("\n") if ln.startswith("bootstrap_clusters:")]


class _Spy:
    """keeps the replicates, the main dict and `failed` of every scope just before the command drops them"""

    def __init__(self):
        from strainscan_amd import read_reports
        self.rr = read_reports
        self.rows = {}

    def __enter__(self):
        self.write = self.rr.write_cluster_bootstrap

        def write(out_dir, scope=None):
            r = self.rr.CLUSTER_BOOTSTRAP["rows"].get(scope)
            if r is not None:
                self.rows[scope] = dict(main=dict(r["main"]), replicates=self.rr.cluster_bootstrap_replicates(scope),
                                        failed=self.rr.cluster_bootstrap_failed(scope))
            return self.write(out_dir, scope)

        self.rr.write_cluster_bootstrap = write
        return self

    def __exit__(self, *exc):
        self.rr.write_cluster_bootstrap = self.write


def _go(L, main, argv):
    """-> (err, return value, stdout, stderr, scan_resampled calls made, what the spy kept)"""
    with _Spy() as spy:
        before = L.scan_resampled_calls()
        err, rc, text, errs = _run(main, argv)
        return err, rc, text, errs, L.scan_resampled_calls() - before, spy.rows


@pytest.fixture(scope="module")
def runs(L, mid_dbs, tmp_path_factory):
    """`strainscan` on DB_M with M_mix: without the flag, with it, with it again, and with another seed"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("cboot_cli")
    fq = mid_dbs["reads"]["M_mix"][0]

    def go():
        out = {}
        for name, extra in (("plain", []), ("flag", FLAGS), ("again", FLAGS), ("other_seed", FLAGS[:2] + ["--bootstrap_seed", "8"])):
            od = str(root / name)
            out[name] = _go(L, StrainScan.main, ["-i", fq, "-d", mid_dbs["DB_M"]["db_dir"], "-o", od] + extra) + (od,)
        return out
    return _with_cache(root, go)


def _walk_materialised(rr, paths, db_dir, seed, b):
    """the flag-off ladder on materialised files -> {leaf id: (cls_ab, cls_cov)}, {} where it ends in "no clusters" """
    from strainscan_amd import StrainScan
    from strainscan_amd import db as ssdb
    ssdb.clear_cache()
    np.random.seed(rr.cluster_bootstrap_walk_seed(seed, b))
    with contextlib.redirect_stdout(io.StringIO()):
        try:
            cls, _ = StrainScan.identify_with_ladder((paths[0], paths[1] if len(paths) > 1 else ""), db_dir + "/Tree_database", 0, 0)
        except SystemExit:
            return {}
        except ValueError:
            return {}
    return {cid: (float(e["cls_ab"]), float(e["cls_cov"])) for cid, e in cls.items()}


def _fastq_records(data):
    lines = data.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [(b"\n".join(lines[i:i + 4]) + b"\n", lines[i + 1]) for i in range(0, len(lines) - 1, 4)]


def test_flag_on_against_flag_off(runs):
    e0, _, t0, errs0, calls0, rows0, d0 = runs["plain"]
    e1, _, t1, errs1, calls1, rows1, d1 = runs["flag"]
    assert _ok(e0) and _ok(e1) and type(e0) is type(e1)
    assert calls0 == 0 and not rows0 and "bootstrap_clusters" not in errs0
    assert calls1 == 1                                      # ceil(B / chunk): four replicates fit one call
    a, b = _files(d0), _others(d1)
    assert TSV not in a and os.path.exists(os.path.join(d1, TSV))
    assert a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert t0 == t1 or _result_lines(t0) == _result_lines(t1)
    assert _result_lines(t0)
    (line,) = _lines(errs1)
    assert line.startswith("bootstrap_clusters: B=4\tS=7\tcalled ") and line.endswith("failed 0")


def test_against_the_materialised_replicates(L, runs, mid_dbs, tmp_path, monkeypatch):
    from strainscan_amd import read_reports as rr
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    got = runs["flag"][5][None]
    assert got["failed"] == 0 and len(got["replicates"]) == B     # (a condition on the input: every replicate calls a cluster)
    recs = _fastq_records(mid_dbs["reads"]["M_mix"][1])
    keys = L.flat_record_keys(b"".join(s + b"\n" for _, s in recs))
    assert keys.shape == (len(recs), 2)
    for b in range(B):
        w = boot_model.weights_of_keys(keys[:, 1], SEED, b)
        p = tmp_path / ("rep%d.fq" % b)
        p.write_bytes(b"".join(t * int(n) for (t, _), n in zip(recs, w.tolist())))
        want = _walk_materialised(rr, [str(p)], mid_dbs["DB_M"]["db_dir"], SEED, b)
        print(b, got["replicates"][b], want)
        assert want and got["replicates"][b] == want, b
    assert len({tuple(sorted(r.items())) for r in got["replicates"]}) > 1      # the replicates are not one walk repeated


def test_the_file_is_the_writer(runs):
    from strainscan_amd import read_reports as rr
    got, od = runs["flag"][5][None], runs["flag"][6]
    text = open(os.path.join(od, TSV)).read()
    print(text)
    assert text == rr.cluster_bootstrap_text(got["main"], got["replicates"])
    rows = {f[0]: f for f in (ln.split("\t") for ln in text.split("\n")[1:-1])}
    assert got["main"] and all("C%s" % cid in rows and rows["C%s" % cid][1] == "1" for cid in got["main"])
    # the main dict is the one the command printed
    assert all(("%s: " % cid) in "\n".join(_result_lines(runs["flag"][2])) for cid in got["main"])
    for f in rows.values():
        assert f[2] == str(B) and 0 <= int(f[3]) <= B and float(f[5]) <= float(f[6]) and float(f[8]) <= float(f[9])


def test_seeds(runs):
    od1, od2, od3 = runs["flag"][6], runs["again"][6], runs["other_seed"][6]
    assert open(os.path.join(od1, TSV), "rb").read() == open(os.path.join(od2, TSV), "rb").read()
    assert runs["flag"][5][None]["replicates"] == runs["again"][5][None]["replicates"]
    assert runs["flag"][5][None]["replicates"] != runs["other_seed"][5][None]["replicates"]
    assert os.path.exists(os.path.join(od3, TSV))


def test_pairs(L, runs, mid_dbs, pair, tmp_path, monkeypatch):
    """with --pairs a fragment (mate 1, N, mate 2) draws one weight: the file is the writer on the walks of the materialised pairs"""
    from strainscan_amd import StrainScan, read_reports as rr
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    db_dir = mid_dbs["DB_M"]["db_dir"]
    base = ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", db_dir]
    e0, _, t0, _, calls0, _ = _go(L, StrainScan.main, base + ["-o", str(tmp_path / "plain")])
    e1, _, t1, errs1, calls1, rows = _go(L, StrainScan.main, base + ["-o", str(tmp_path / "flag"), "--pairs"] + FLAGS)
    assert _ok(e0) and _ok(e1) and calls0 == 0 and calls1 == 1 and len(_lines(errs1)) == 1
    a, b = _files(str(tmp_path / "plain")), _others(str(tmp_path / "flag"))
    assert a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert _result_lines(t0) == _result_lines(t1)
    keys = pairs_model.pair_digests(L, [s for _, s in pair["recs"][0]], [s for _, s in pair["recs"][1]])
    reps = []
    for rep in range(B):
        w = boot_model.weights_of_keys(keys[:, 1], SEED, rep)
        paths = []
        for m in range(2):
            paths.append(str(tmp_path / ("rep%d_R%d.fq" % (rep, m + 1))))
            with open(paths[m], "wb") as f:
                f.write(b"".join(t * int(n) for (t, _), n in zip(pair["recs"][m], w.tolist())))
        reps.append(_walk_materialised(rr, paths, db_dir, SEED, rep))
    assert all(reps)
    assert rows[None]["replicates"] == reps
    assert open(os.path.join(str(tmp_path / "flag"), TSV)).read() == rr.cluster_bootstrap_text(rows[None]["main"], reps)


def _skipped(L, runs, main, argv, od, what):
    """a run that cannot resample: one line with `what`, no file, no call, and the reports of the run without the flag"""
    err, _, text, errs, calls, rows = _go(L, main, argv)
    lines = _lines(errs)
    assert len(lines) == 1 and what in lines[0] and "no intervals were computed" in lines[0], (lines, errs[-2000:])
    assert calls == 0 and not rows
    assert not [k for k in _files(od) if os.path.basename(k) == TSV]
    return err, text


def test_sample_not_resident(L, runs, mid_dbs, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    from strainscan_amd import db as ssdb
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    monkeypatch.setattr(ssdb, "RESIDENT_LIMIT_BYTES", 0)
    od = str(tmp_path / "out")
    err, text = _skipped(L, runs, StrainScan.main, ["-i", mid_dbs["reads"]["M_mix"][0], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od] + FLAGS, od,
                         "resident on the device")
    e0, _, t0, _, _, _, d0 = runs["plain"]
    assert _ok(err) and type(err) is type(e0)
    a, b = _files(d0), _files(od)
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert _result_lines(t0) == _result_lines(text)


def test_single_cluster_database(L, runs, l1_dbs, l1_reads, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    argv = ["-i", l1_reads["D_one"][0], "-d", l1_dbs["D"]["db_dir"]]
    e0, _, t0, errs0, _, _ = _go(L, StrainScan.main, argv + ["-o", str(tmp_path / "plain")])
    assert "bootstrap_clusters" not in errs0
    od = str(tmp_path / "out")
    err, text = _skipped(L, runs, StrainScan.main, argv + ["-o", od] + FLAGS, od, "single cluster")
    assert type(err) is type(e0) and getattr(err, "code", None) == getattr(e0, "code", None)
    a, b = _files(str(tmp_path / "plain")), _files(od)
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert _result_lines(t0) == _result_lines(text)


def test_two_ranks_say_so(runs, mid_dbs, tmp_path):
    """Two ranks on one GPU (fresh child processes, gloo, each under its own timeout): several ranks are out of scope -- one line
    on rank 0's stderr, no file, the reports of the single-process run."""
    od = str(tmp_path / "out")
    code = WORKER % dict(repo=REPO, seed=sc.POISSON_SEED,
                         argv=["-i", mid_dbs["reads"]["M_mix"][0], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od] + FLAGS)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", SS_IMAGE_CACHE=str(tmp_path / "cache"),
                   SS_TEST_STORE=str(tmp_path / "store"))
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, "-c", code], env=env, stderr=subprocess.PIPE))
    errs = [p.communicate(timeout=300)[1].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), [e[-3000:] for e in errs]
    lines = [_lines(e) for e in errs]
    assert len(lines[0]) == 1 and "one rank" in lines[0][0] and not lines[1], lines
    a, b = _files(runs["plain"][6]), _files(od)
    assert TSV not in b and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)


def test_multi_db_writes_one_file_per_label(L, runs, mid_dbs, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbm, dbmem = mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]
    od = str(tmp_path / "flag")
    err, rc, _, errs, calls, rows = _go(L, multi_db.main, ["-i", mid_dbs["reads"]["M_mix"][0], "-d", dbm, "-d", "mem=" + dbmem, "-o", od] + FLAGS)
    assert err is None and rc == 0 and calls == 2 and len(_lines(errs)) == 2
    from strainscan_amd import read_reports as rr
    labels = (os.path.basename(os.path.normpath(dbm)), "mem")
    assert sorted(rows) == sorted(labels)
    for label in labels:
        assert open(os.path.join(od, label, TSV)).read() == rr.cluster_bootstrap_text(rows[label]["main"], rows[label]["replicates"]), label
    assert open(os.path.join(od, labels[0], TSV)).read() == open(os.path.join(runs["flag"][6], TSV)).read()
    assert not os.path.exists(os.path.join(od, TSV))
