"""`strainscan --read_support` / `strainscan-multi --read_support`: read_support.tsv holds, for the tree's table and for every
cluster table scanned at layer 2, the numbers of the model (tests/rs_model.py) computed from the FASTQ bytes and the k-mer
files; stdout's result lines and every other report are what a run without the flag writes; without the flag nothing new runs."""
import contextlib
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import rs_model, synth
from tests import scenarios as sc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TSV = "read_support.tsv"
HEADER = "table\tkmers\treads\thits\tge1\tge2\tge4\tge8\tge16\tge32\tge64"


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


def _result_lines(text):
    """the dict lines of stdout (the cluster dictionaries the commands print), without the lines that carry running times"""
    lines = [ln for ln in text.split("\n") if ln.startswith(("{", "defaultdict("))]
    # (a defaultdict prints its factory with the address it has in this run: "<function ... at 0x7be2...>")
    return [re.sub(r" at 0x[0-9a-fA-F]+>", " at 0x>", ln) for ln in lines]


def _run(main, argv):
    from strainscan_amd import db as ssdb
    ssdb.clear_cache()
    np.random.seed(sc.POISSON_SEED)
    buf = io.StringIO()
    err = rc = None
    with contextlib.redirect_stdout(buf):
        try:
            rc = main(argv)
        except BaseException as e:      # noqa: B902 -- how the run ended is part of what is compared
            err = e
    return err, rc, buf.getvalue()


def _ok(err):
    return err is None or (isinstance(err, SystemExit) and err.code in (None, 0))


def _model_row(flat, fasta_path, k=31):
    with open(fasta_path, "rb") as f:
        kmers = list(dict.fromkeys(km.upper() for km in rs_model.kmers_of_fasta(f.read())))
    per = rs_model.hits_per_record(flat, rs_model.encode_kmers(kmers, k), k)
    n_rec = per.size
    return [len(kmers), n_rec, int(per.sum())] + [int((per >= t).sum()) for t in (1, 2, 4, 8, 16, 32, 64)]


def _check_tsv(path, db_dir, out_dir, flat):
    lines = open(path).read().split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    rows = [ln.split("\t") for ln in lines[1:-1]]
    names = [r[0] for r in rows]
    clusters = sorted(d for d in os.listdir(out_dir) if d.startswith("C") and os.path.isdir(os.path.join(out_dir, d)))
    assert names[0] == "tree" and sorted(names[1:]) == clusters and len(clusters) >= 2, (names, clusters)
    for r in rows:
        fa = (os.path.join(db_dir, "Tree_database", "kmer.fa") if r[0] == "tree"
              else os.path.join(db_dir, "Kmer_Sets_L2", "Kmer_Sets", r[0], "all_kmer.fasta"))
        want = _model_row(flat, fa)
        print(r[0], [int(x) for x in r[1:]], want)
        assert [int(x) for x in r[1:]] == want, r[0]
        assert int(r[3]) > 0 and int(r[2]) >= int(r[4]) >= int(r[5]) >= int(r[10])
    return rows


@pytest.fixture(scope="module")
def mix(mid_dbs):
    fq, data = mid_dbs["reads"]["M_mix"]
    return fq, synth.flat_bases_from_fastx(data)


@pytest.fixture(scope="module")
def single_runs(L, mid_dbs, mix, tmp_path_factory):
    """`strainscan` on DB_M with M_mix, without and with the flag -> dict(plain=, flag=) of (err, stdout, out dir, calls made)"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("rs_cli")
    old = os.environ.get("SS_IMAGE_CACHE")
    os.environ["SS_IMAGE_CACHE"] = str(root / "cache")
    try:
        out = {}
        for name, extra in (("plain", []), ("flag", ["--read_support"])):
            before = L.support_calls()
            od = str(root / name)
            err, _, text = _run(StrainScan.main, ["-i", mix[0], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od] + extra)
            out[name] = (err, text, od, L.support_calls() - before)
    finally:
        if old is None:
            os.environ.pop("SS_IMAGE_CACHE", None)
        else:
            os.environ["SS_IMAGE_CACHE"] = old
    return out


def test_flag_writes_the_models_numbers(single_runs, mid_dbs, mix):
    err, _, od, calls = single_runs["flag"]
    assert _ok(err), err
    rows = _check_tsv(os.path.join(od, TSV), mid_dbs["DB_M"]["db_dir"], od, mix[1])
    assert calls == len(rows)


def test_flag_off_runs_nothing_and_reports_are_unchanged(single_runs):
    e0, t0, d0, calls0 = single_runs["plain"]
    e1, t1, d1, _ = single_runs["flag"]
    assert _ok(e0) and _ok(e1) and type(e0) is type(e1)
    assert calls0 == 0
    a, b = _files(d0), _files(d1)
    assert TSV not in a and TSV in b
    b.pop(TSV)
    assert a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert _result_lines(t0) and _result_lines(t0) == _result_lines(t1)


def test_multi_db_writes_one_file_per_label(L, mid_dbs, mix, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbm, dbmem = mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]
    base = ["-i", mix[0], "-d", dbm, "-d", "mem=" + dbmem]
    before = L.support_calls()
    e0, rc0, t0 = _run(multi_db.main, base + ["-o", str(tmp_path / "plain")])
    assert L.support_calls() == before
    e1, rc1, t1 = _run(multi_db.main, base + ["-o", str(tmp_path / "flag"), "--read_support"])
    assert e0 is None and e1 is None and rc0 == 0 and rc1 == 0
    a, b = _files(str(tmp_path / "plain")), _files(str(tmp_path / "flag"))
    labels = [os.path.basename(os.path.normpath(dbm)), "mem"]
    for label, d in zip(labels, (dbm, dbmem)):
        rel = os.path.join(label, TSV)
        assert rel in b and rel not in a
        _check_tsv(os.path.join(str(tmp_path / "flag"), rel), d, os.path.join(str(tmp_path / "flag"), label), mix[1])
        b.pop(rel)
    assert not [k for k in b if k.endswith(TSV)]
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert _result_lines(t0) == _result_lines(t1)


def test_sample_not_resident(L, single_runs, mid_dbs, mix, tmp_path, monkeypatch, capsys):
    from strainscan_amd import StrainScan
    from strainscan_amd import db as ssdb
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    monkeypatch.setattr(ssdb, "RESIDENT_LIMIT_BYTES", 0)
    capsys.readouterr()
    before = L.support_calls()
    od = str(tmp_path / "out")
    err, _, text = _run(StrainScan.main, ["-i", mix[0], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od, "--read_support"])
    lines = [ln for ln in capsys.readouterr().err.split("\n") if ln.startswith("read_support:")]
    assert len(lines) == 1 and "resident on the device" in lines[0] and "not computed" in lines[0], lines
    assert _ok(err) and L.support_calls() == before
    e0, t0, d0, _ = single_runs["plain"]
    a, b = _files(d0), _files(od)
    assert TSV not in b and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
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


def test_two_ranks_write_the_single_process_file(single_runs, mid_dbs, mix, tmp_path):
    """Two ranks on one GPU (fresh child processes, gloo, as tests/test_dist_gpu.py): each computes over its shard, the integers
    are summed over the ranks, rank 0 writes the file."""
    od = str(tmp_path / "out")
    code = WORKER % dict(repo=REPO, seed=sc.POISSON_SEED,
                         argv=["-i", mix[0], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od, "--read_support"])
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", SS_IMAGE_CACHE=str(tmp_path / "cache"),
                   SS_TEST_STORE=str(tmp_path / "store"))
        procs.append(subprocess.Popen([sys.executable, "-c", code], env=env, stderr=subprocess.PIPE))
    errs = [p.communicate(timeout=300)[1].decode()[-3000:] for p in procs]
    assert all(p.returncode == 0 for p in procs), errs
    want = open(os.path.join(single_runs["flag"][2], TSV)).read()
    assert open(os.path.join(od, TSV)).read() == want
    assert json.dumps(sorted(k for k in _files(od))) == json.dumps(sorted(k for k in _files(single_runs["flag"][2])))
