"""`strainscan -x N` / `strainscan-multi -x N`: extracted/<table>_1.fastq and _2.fastq hold, for the tree's table and for every cluster
table scanned at layer 2, exactly the pairs the model (tests/rs_model.py) selects from the FASTQ bytes and the k-mer files -- a pair
when either mate has at least N hits -- in file order and byte for byte; stdout's result lines and every report are what a run
without the flag writes; without the flag nothing new runs; where nothing can be extracted one line on stderr says why."""
import contextlib
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import rs_model
from tests import scenarios as sc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 16
DIR = "extracted"


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _files(d):
    out = {}
    for root, _, fs in os.walk(d):
        for f in fs:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def _reports(d):
    return {k: v for k, v in _files(d).items() if DIR not in k.split(os.sep)}


def _result_lines(text):
    """the dict lines of stdout (the cluster dictionaries the commands print), without the lines that carry running times"""
    lines = [ln for ln in text.split("\n") if ln.startswith(("{", "defaultdict("))]
    return [re.sub(r" at 0x[0-9a-fA-F]+>", " at 0x>", ln) for ln in lines]


def _run(main, argv):
    """-> (how it ended, return value, stdout, stderr)"""
    from strainscan_amd import db as ssdb
    ssdb.clear_cache()
    np.random.seed(sc.POISSON_SEED)
    out, errs = io.StringIO(), io.StringIO()
    err = rc = None
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(errs):
        try:
            rc = main(argv)
        except BaseException as e:      # noqa: B902 -- how the run ended is part of what is compared
            err = e
    return err, rc, out.getvalue(), errs.getvalue()


def _ok(err):
    return err is None or (isinstance(err, SystemExit) and err.code in (None, 0))


@pytest.fixture(scope="module")
def pair(mid_dbs, tmp_path_factory):
    """M_mix as a FASTQ pair with unique names: its records dealt out in turn -> dict(paths=, recs=[(mate 1 records), (mate 2
    records)]), a record being (text, sequence)"""
    _, data = mid_dbs["reads"]["M_mix"]
    lines = data.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    seqs = lines[1:-1:4]
    assert all(ln.startswith(b"@") for ln in lines[0:-1:4]) and all(ln.startswith(b"+") for ln in lines[2:-1:4])
    rs = np.random.RandomState(31)
    qa = np.frombuffer(b"5678ABCDEFGHIJ", np.uint8)
    n = len(seqs) // 2
    recs = ([], [])
    for i in range(n):
        for m in range(2):
            s = seqs[2 * i + m]
            recs[m].append((b"@pair%d/%d\n%s\n+\n%s\n" % (i, m + 1, s, qa[rs.randint(0, qa.size, size=len(s))].tobytes()), s))
    root = tmp_path_factory.mktemp("x_pair")
    paths = []
    for m in range(2):
        p = root / ("mix_R%d.fastq" % (m + 1))
        p.write_bytes(b"".join(t for t, _ in recs[m]))
        paths.append(str(p))
    return dict(paths=paths, recs=recs)


def _with_cache(root, fn):
    old = os.environ.get("SS_IMAGE_CACHE")
    os.environ["SS_IMAGE_CACHE"] = str(root / "cache")
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("SS_IMAGE_CACHE", None)
        else:
            os.environ["SS_IMAGE_CACHE"] = old


@pytest.fixture(scope="module")
def single_runs(L, mid_dbs, pair, tmp_path_factory):
    """`strainscan` on DB_M with the pair, without and with -x 16 -> dict(plain=, flag=) of (err, stdout, stderr, out dir, select
    calls made)"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("x_cli")

    def go():
        out = {}
        for name, extra in (("plain", []), ("flag", ["-x", str(N)])):
            before = L.select_calls()
            od = str(root / name)
            err, _, text, errs = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od]
                                      + extra)
            out[name] = (err, text, errs, od, L.select_calls() - before)
        return out
    return _with_cache(root, go)


def _model_files(pair, fasta_path, k=31):
    """the two files the model writes for a table: every pair with a mate of at least N hits, in file order"""
    with open(fasta_path, "rb") as f:
        kmers = list(dict.fromkeys(km.upper() for km in rs_model.kmers_of_fasta(f.read())))
    keys = rs_model.encode_kmers(kmers, k)
    per = [rs_model.hits_per_record(b"".join(s + b"\n" for _, s in pair["recs"][m]), keys, k) for m in range(2)]
    assert per[0].size == per[1].size == len(pair["recs"][0])
    keep = np.nonzero((per[0] >= N) | (per[1] >= N))[0]
    return [b"".join(pair["recs"][m][i][0] for i in keep) for m in range(2)], keep.size


def _check_extracted(ex_dir, db_dir, out_dir, pair):
    """every table's two files against the model -> {table: pairs written}"""
    clusters = sorted(d for d in os.listdir(out_dir) if d.startswith("C") and os.path.isdir(os.path.join(out_dir, d)))
    assert len(clusters) >= 2
    tables = ["tree"] + clusters
    assert sorted(os.listdir(ex_dir)) == sorted("%s_%d.fastq" % (t, m) for t in tables for m in (1, 2))
    sizes = {}
    for t in tables:
        fa = (os.path.join(db_dir, "Tree_database", "kmer.fa") if t == "tree"
              else os.path.join(db_dir, "Kmer_Sets_L2", "Kmer_Sets", t, "all_kmer.fasta"))
        want, n_pairs = _model_files(pair, fa)
        for m in range(2):
            got = open(os.path.join(ex_dir, "%s_%d.fastq" % (t, m + 1)), "rb").read()
            assert got == want[m], (t, m + 1, len(got), len(want[m]))
        print(t, "pairs", n_pairs, "of", len(pair["recs"][0]))
        sizes[t] = n_pairs
    return sizes


def test_extracted_files_are_the_models(single_runs, mid_dbs, pair):
    err, _, errs, od, calls = single_runs["flag"]
    assert _ok(err), err
    sizes = _check_extracted(os.path.join(od, DIR), mid_dbs["DB_M"]["db_dir"], od, pair)
    assert calls == len(sizes)
    total = len(pair["recs"][0])
    assert any(0 < n < total for t, n in sizes.items() if t != "tree"), sizes      # a cluster file that is neither empty nor everything
    # one summary line per table on stderr: table, N, records selected on the device, records written
    lines = [ln for ln in errs.split("\n") if ln.startswith("extract_reads:")]
    assert len(lines) == len(sizes), lines
    for ln in lines:
        m = re.match(r"extract_reads: (\S+)\tN=16\tselected on the device (\d+)\twritten (\d+)$", ln)
        assert m and m.group(1) in sizes and int(m.group(3)) == 2 * sizes[m.group(1)], ln
        assert 0 < int(m.group(2)) <= int(m.group(3))


def test_flag_off_runs_nothing_and_reports_are_unchanged(single_runs):
    e0, t0, errs0, d0, calls0 = single_runs["plain"]
    e1, t1, _, d1, _ = single_runs["flag"]
    assert _ok(e0) and _ok(e1) and type(e0) is type(e1)
    assert calls0 == 0 and "extract_reads" not in errs0
    assert not os.path.exists(os.path.join(d0, DIR)) and os.path.isdir(os.path.join(d1, DIR))
    a, b = _files(d0), _reports(d1)
    assert a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert t0 == t1 or _result_lines(t0) == _result_lines(t1)
    assert _result_lines(t0)


def test_multi_db_writes_one_directory_per_label(L, single_runs, mid_dbs, pair, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbm, dbmem = mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]
    base = ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", dbm, "-d", "mem=" + dbmem]
    before = L.select_calls()
    e0, rc0, t0, _ = _run(multi_db.main, base + ["-o", str(tmp_path / "plain")])
    assert L.select_calls() == before
    e1, rc1, t1, _ = _run(multi_db.main, base + ["-o", str(tmp_path / "flag"), "-x", str(N)])
    assert e0 is None and e1 is None and rc0 == 0 and rc1 == 0
    a, b = _files(str(tmp_path / "plain")), _files(str(tmp_path / "flag"))
    assert not [k for k in a if DIR in k.split(os.sep)]
    # the two databases hold the same genomes: each label's directory is the single run's, which the model has checked
    want = _files(os.path.join(single_runs["flag"][3], DIR))
    assert want
    for label in (os.path.basename(os.path.normpath(dbm)), "mem"):
        got = {os.path.relpath(k, os.path.join(label, DIR)): v for k, v in b.items() if k.startswith(os.path.join(label, DIR) + os.sep)}
        assert sorted(got) == sorted(want) and all(got[k] == want[k] for k in want), label
    assert not os.path.exists(str(tmp_path / "flag" / DIR))
    rep = {k: v for k, v in b.items() if DIR not in k.split(os.sep)}
    assert sorted(a) == sorted(rep) and all(a[k] == rep[k] for k in a)
    assert _result_lines(t0) == _result_lines(t1)


def test_sample_not_resident(L, single_runs, mid_dbs, pair, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    from strainscan_amd import db as ssdb
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    monkeypatch.setattr(ssdb, "RESIDENT_LIMIT_BYTES", 0)
    before = L.select_calls()
    od = str(tmp_path / "out")
    err, _, text, errs = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od,
                                                "-x", str(N)])
    lines = [ln for ln in errs.split("\n") if ln.startswith("extract_reads:")]
    assert len(lines) == 1 and "resident on the device" in lines[0] and "nothing was extracted" in lines[0], lines
    e0, t0, _, d0, _ = single_runs["plain"]
    assert _ok(err) and type(err) is type(e0) and L.select_calls() == before
    a, b = _files(d0), _files(od)
    assert not os.path.exists(os.path.join(od, DIR)) and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert _result_lines(t0) == _result_lines(text)


WORKER = r'''
import contextlib, io, os, sys
import numpy as np
sys.path.insert(0, %(repo)r)
import torch
import torch.distributed as dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", init_method="file://" + os.environ["SS_TEST_STORE"], rank=rank, world_size=world)
from strainscan_amd import StrainScan
np.random.seed(%(seed)d)
with contextlib.redirect_stdout(io.StringIO()):
    try:
        StrainScan.main(%(argv)r)
    except SystemExit as e:
        assert e.code in (None, 0), e.code
dist.barrier()
dist.destroy_process_group()
'''


def test_two_ranks_extract_nothing_and_say_so(single_runs, mid_dbs, pair, tmp_path):
    """Two ranks on one GPU (fresh child processes, gloo, as tests/test_dist_gpu.py): several ranks are out of scope -- one line on
    rank 0's stderr, no directory, the reports of the single-process run."""
    od = str(tmp_path / "out")
    code = WORKER % dict(repo=REPO, seed=sc.POISSON_SEED,
                         argv=["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od, "-x", str(N)])
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
    assert sorted(_files(od)) == sorted(_files(single_runs["plain"][3]))
