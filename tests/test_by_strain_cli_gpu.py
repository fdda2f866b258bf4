"""`strainscan --by_strain` with --read_support and -x N, on the mid-size database and its M_mix sample (built on the CPU from the
fixture's genomes: two strains of C7, three of C19, one of C23 and a singleton -- the reports the run writes must show a cluster
with exactly two called strains, and do: C7).

strain_support.tsv equals the model (tests/label_model.py) computed from the StrainVote.report files the run wrote, each cluster's
all_strains_re.npz / id2strain_re.pkl / all_kmer.fasta and the sample's sequences; every extracted/C<id>.<n>_*.fastq holds the
model's pairs as whole FASTQ records in file order; every other output file and the result lines of stdout are those of the run
without --by_strain; without the flag the labelled calls do not run."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import label_model, rs_model
from tests import scenarios as sc
from tests.test_extract_cli_gpu import DIR, REPO, WORKER, _files, _ok, _result_lines, _run, _with_cache, pair      # noqa: F401

pytestmark = pytest.mark.gpu

N = 8
TSV = "strain_support.tsv"


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _is_strain_file(rel):
    parts = rel.split(os.sep)
    return parts[-1] == TSV or (DIR in parts and "." in parts[-1].split("_")[0])


def _others(d):
    return {k: v for k, v in _files(d).items() if not _is_strain_file(k)}


@pytest.fixture(scope="module")
def single_runs(L, mid_dbs, pair, tmp_path_factory):
    """`strainscan --read_support -x 8` on DB_M with the pair, without and with --by_strain -> name: (err, stdout, stderr, out dir,
    labelled calls made)"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("bs_cli")

    def go():
        out = {}
        for name, extra in (("plain", []), ("flag", ["--by_strain"])):
            before = L.labeled_calls()
            od = str(root / name)
            err, _, text, errs = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od,
                                                        "--read_support", "-x", str(N)] + extra)
            out[name] = (err, text, errs, od, L.labeled_calls() - before)
        return out
    return _with_cache(root, go)


def _called(report):
    rows = [ln.split("\t") for ln in open(report).read().split("\n")[1:] if ln.strip()]
    return [(int(r[0]), r[1]) for r in rows]


_MODEL = {}


def _model(db_dir, out_dir, pair):
    """-> (tsv text, {table: [mate 1 bytes, mate 2 bytes]}, {cluster: called strains}) from the reports in out_dir"""
    if out_dir in _MODEL:
        return _MODEL[out_dir]
    import scipy.sparse as sp
    from strainscan_amd import read_reports
    rs_rows = [ln.split("\t")[0] for ln in open(os.path.join(out_dir, "read_support.tsv")).read().split("\n")[1:] if ln]
    texts = [b"".join(s + b"\n" for _, s in pair["recs"][m]) for m in range(2)]
    n_reads = 2 * len(pair["recs"][0])
    rows, files, called_of = [], {}, {}
    for cls in [t for t in rs_rows if t != "tree"]:                 # clusters in the order they were scanned
        report = os.path.join(out_dir, cls, "StrainVote.report")
        if not os.path.exists(report):
            continue
        called = _called(report)
        called_of[cls] = called
        cdir = os.path.join(db_dir, "Kmer_Sets_L2", "Kmer_Sets", cls)
        with open(os.path.join(cdir, "id2strain_re.pkl"), "rb") as f:
            sid = pickle.load(f)
        col_of = {name: c for c, name in (sid.items() if isinstance(sid, dict) else enumerate(sid))}
        dense = np.asarray(sp.load_npz(os.path.join(cdir, "all_strains_re.npz")).todense())
        lab = label_model.row_labels(dense, [col_of[name] for _, name in called])
        with open(os.path.join(cdir, "all_kmer.fasta"), "rb") as f:
            kmers = [km.upper() for km in rs_model.kmers_of_fasta(f.read())]
        assert len(kmers) == dense.shape[0]
        keys = rs_model.encode_kmers(kmers, 31)
        Ln = len(called)
        per = [label_model.labeled_hits_per_record(texts[m], keys, lab, Ln, 31) for m in range(2)]
        _, ul = label_model.kmer_labels(keys, lab)
        for j, (n, name) in enumerate(called, 1):
            both = np.concatenate([per[0][j], per[1][j]])
            rows.append(("%s.%d" % (cls, n), name, int((ul == j).sum()), n_reads, int(both.sum()), rs_model.histogram(both, 65)))
            keep = np.nonzero((per[0][j] >= N) | (per[1][j] >= N))[0]
            files["%s.%d" % (cls, n)] = [b"".join(pair["recs"][m][i][0] for i in keep) for m in range(2)]
    _MODEL[out_dir] = (read_reports.strain_support_text(rows), files, called_of)
    return _MODEL[out_dir]


def test_strain_support_and_strain_files_are_the_models(single_runs, mid_dbs, pair):
    err, _, errs, od, calls = single_runs["flag"]
    assert _ok(err), err
    want_tsv, want_files, called_of = _model(mid_dbs["DB_M"]["db_dir"], od, pair)
    print({c: v for c, v in called_of.items()})
    assert any(len(v) == 2 for v in called_of.values()), called_of          # two strains called in one cluster
    got_tsv = open(os.path.join(od, TSV)).read()
    print(got_tsv)
    assert got_tsv == want_tsv
    assert got_tsv.split("\n")[0] == "table\tstrain\tkmers\treads\thits\tge1\tge2\tge4\tge8\tge16\tge32\tge64"
    ex = os.path.join(od, DIR)
    strain_files = sorted(f for f in os.listdir(ex) if "." in f.split("_")[0])
    assert strain_files == sorted("%s_%d.fastq" % (t, m) for t in want_files for m in (1, 2))
    total = len(pair["recs"][0])
    sizes = {}
    for t, want in want_files.items():
        for m in range(2):
            got = open(os.path.join(ex, "%s_%d.fastq" % (t, m + 1)), "rb").read()
            assert got == want[m], (t, m + 1, len(got), len(want[m]))
        sizes[t] = want[0].count(b"\n") // 4
    print(sizes, "of", total)
    two = [c for c, v in called_of.items() if len(v) == 2][0]
    assert all(0 < sizes["%s.%d" % (two, n)] < total for n, _ in called_of[two]), sizes
    # one labelled support call per cluster with a report, one labelled select per strain
    assert calls == len(called_of) + len(want_files)
    lines = [ln for ln in errs.split("\n") if ln.startswith("extract_reads:") and "." in ln.split("\t")[0]]
    assert sorted(ln.split("\t")[0].split(" ")[1] for ln in lines) == sorted(want_files), lines
    for ln in lines:
        t = ln.split("\t")[0].split(" ")[1]
        assert ln.split("\t")[1] == "N=%d" % N and ln.endswith("written %d" % (2 * sizes[t])), ln


def test_other_outputs_are_unchanged_and_flag_off_runs_nothing(single_runs):
    e0, t0, errs0, d0, calls0 = single_runs["plain"]
    e1, t1, _, d1, calls1 = single_runs["flag"]
    assert _ok(e0) and _ok(e1) and type(e0) is type(e1)
    assert calls0 == 0 and calls1 > 0
    a, b = _files(d0), _others(d1)
    assert not [k for k in a if _is_strain_file(k)]
    assert "read_support.tsv" in a and [k for k in a if DIR in k.split(os.sep)]
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert t0 == t1 or _result_lines(t0) == _result_lines(t1)
    assert _result_lines(t0)


def test_multi_db_writes_under_each_label(L, single_runs, mid_dbs, pair, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbm, dbmem = mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]
    od = str(tmp_path / "flag")
    e1, rc1, _, _ = _run(multi_db.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", dbm, "-d", "mem=" + dbmem, "-o", od,
                                         "--read_support", "-x", str(N), "--by_strain"])
    assert e1 is None and rc1 == 0
    # the two databases hold the same genomes: each label's strain files are the single run's, which the model has checked
    want = {k: v for k, v in _files(single_runs["flag"][3]).items() if _is_strain_file(k)}
    assert TSV in want and len(want) >= 5
    got_all = _files(od)
    for label in (os.path.basename(os.path.normpath(dbm)), "mem"):
        got = {os.path.relpath(k, label): v for k, v in got_all.items() if k.startswith(label + os.sep) and _is_strain_file(k)}
        assert sorted(got) == sorted(want) and all(got[k] == want[k] for k in want), label
    assert not os.path.exists(os.path.join(od, TSV)) and not os.path.exists(os.path.join(od, DIR))


def test_sample_not_resident(L, single_runs, mid_dbs, pair, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    from strainscan_amd import db as ssdb
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    monkeypatch.setattr(ssdb, "RESIDENT_LIMIT_BYTES", 0)
    before = L.labeled_calls()
    od = str(tmp_path / "out")
    err, _, text, errs = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od,
                                                "--read_support", "-x", str(N), "--by_strain"])
    for tag in ("read_support:", "extract_reads:"):
        lines = [ln for ln in errs.split("\n") if ln.startswith(tag)]
        assert len(lines) == 1 and "resident on the device" in lines[0], lines
    e0 = single_runs["plain"][0]
    assert _ok(err) and type(err) is type(e0) and L.labeled_calls() == before
    assert not os.path.exists(os.path.join(od, TSV)) and not os.path.exists(os.path.join(od, DIR))
    assert _result_lines(single_runs["plain"][1]) == _result_lines(text)


def test_two_ranks_write_the_single_process_file_and_extract_nothing(single_runs, mid_dbs, pair, tmp_path):
    """Two ranks on one GPU (fresh child processes, gloo): each counts its shard, the sums are the single-process
    strain_support.tsv; per-strain extraction inherits -x's limit -- one line on rank 0's stderr, no directory."""
    od = str(tmp_path / "out")
    code = WORKER % dict(repo=REPO, seed=sc.POISSON_SEED,
                         argv=["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od,
                               "--read_support", "-x", str(N), "--by_strain"])
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", SS_IMAGE_CACHE=str(tmp_path / "cache"),
                   SS_TEST_STORE=str(tmp_path / "store"))
        procs.append(subprocess.Popen([sys.executable, "-c", code], env=env, stderr=subprocess.PIPE))
    errs = [p.communicate(timeout=300)[1].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), [e[-3000:] for e in errs]
    lines = [[ln for ln in e.split("\n") if ln.startswith("extract_reads:")] for e in errs]
    assert len(lines[0]) == 1 and "one rank only" in lines[0][0] and lines[1] == [], lines
    assert not os.path.exists(os.path.join(od, DIR))
    assert open(os.path.join(od, TSV)).read() == open(os.path.join(single_runs["flag"][3], TSV)).read()
    assert open(os.path.join(od, "read_support.tsv")).read() == open(os.path.join(single_runs["plain"][3], "read_support.tsv")).read()
