"""`strainscan --read_calls` / `strainscan-multi --read_calls`: read_calls_<i>.tsv is the model's text (tests/read_calls_model.py)
computed from the FASTQ bytes, kmer.fa, kmers/<id> and tree_structure.txt; the histogram of its node column is read_classes.tsv's
reads_direct column; stdout and every other file are what a run without the flag writes; without the flag nothing new runs."""
import os
import re
import subprocess
import sys
from collections import Counter

import pytest

from tests import read_calls_model as rcm, synth
from tests import scenarios as sc
from tests.test_extract_class_cli_gpu import tree_model
from tests.test_extract_cli_gpu import _files, _ok, _result_lines, _run, _with_cache, pair      # noqa: F401
from tests.test_read_support_cli_gpu import WORKER

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 2


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def tm(mid_dbs):
    return {name: tree_model(mid_dbs[name]["db_dir"]) for name in ("DB_M", "DB_Mmem")}


def model_files(t, texts, m, joined=False):
    """[read_calls_<i>.tsv] for the input texts against the tree model `t`: each file on its own, or the two joined line by line"""
    flats = [synth.flat_bases_from_fastx(x) for x in texts]
    node_value = [-1] + list(t["node_ids"])
    if joined:
        a, b = (f.split(b"\n")[:-1] for f in flats)
        assert len(a) == len(b)
        flat = b"".join(x + b"N" + y + b"\n" for x, y in zip(a, b))
        return rcm.table_text(texts, rcm.calls_model(flat, t["keys"], t["row_node"], t["parent"], t["k"], m), node_value)
    return [rcm.table_text([x], rcm.calls_model(f, t["keys"], t["row_node"], t["parent"], t["k"], m), node_value)[0] for x, f in zip(texts, flats)]


def node_histogram(*tables):
    """{node text: lines} over the node column of read_calls files (bytes), the records without a sequence left out"""
    c = Counter()
    for text in tables:
        for ln in text.split(b"\n")[1:-1]:
            f = ln.split(b"\t")
            if not (f[1:] == [b"-1", b"0", b"0", b"-"]):
                c[f[1].decode()] += 1
    return c


def direct_column(od):
    """{node text (-1: unclassified): reads_direct} of a run's read_classes.tsv, zeros left out"""
    rows = [ln.split("\t") for ln in open(os.path.join(od, "read_classes.tsv")).read().split("\n")[1:-1]]
    return Counter({("-1" if r[0] == "unclassified" else r[0]): int(r[5]) for r in rows if int(r[5])})


def stderr_lines(errs):
    return [ln for ln in errs.split("\n") if ln.startswith("read_calls:")]


@pytest.fixture(scope="module")
def single_runs(L, mid_dbs, tmp_path_factory):
    """`strainscan --classify_reads M` on DB_M with M_mix, without and with --read_calls -> name: (err, stdout, stderr, out dir, calls)"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("rc_cli")
    fq, _ = mid_dbs["reads"]["M_mix"]

    def go():
        out = {}
        for name, extra in (("plain", []), ("flag", ["--read_calls"])):
            before = L.read_calls_calls()
            od = str(root / name)
            err, _, text, errs = _run(StrainScan.main, ["-i", fq, "-d", mid_dbs["DB_M"]["db_dir"], "-o", od, "--classify_reads", str(M)] + extra)
            out[name] = (err, text, errs, od, L.read_calls_calls() - before)
        return out
    return _with_cache(root, go)


def test_single_end_file_is_the_models_text(single_runs, mid_dbs, tm):
    err, _, errs, od, calls = single_runs["flag"]
    assert _ok(err), err
    _, data = mid_dbs["reads"]["M_mix"]
    want, = model_files(tm["DB_M"], [data], M)
    got = open(os.path.join(od, "read_calls_1.tsv"), "rb").read()
    hist = node_histogram(got)
    print("lines", got.count(b"\n") - 1, "classified", sum(v for k, v in hist.items() if k != "-1"), "nodes", len(hist),
          "with a list", sum(1 for ln in got.split(b"\n")[1:-1] if not ln.endswith(b"\t-")))
    assert got == want
    assert 1 <= calls <= 2 and not os.path.exists(os.path.join(od, "read_calls_2.tsv"))      # (2: the lists needed more room than the first call brought)
    assert hist == direct_column(od) and len(hist) >= 3
    lines = stderr_lines(errs)
    assert len(lines) == 1
    m = re.match(r"read_calls: (\S+)\tM=%d\trecords (\d+)\tclassified (\d+)\tempty (\d+)$" % M, lines[0])
    assert m and m.group(1) == os.path.join(od, "read_calls_1.tsv")
    assert int(m.group(2)) == got.count(b"\n") - 1 and int(m.group(3)) == sum(v for k, v in hist.items() if k != "-1") and int(m.group(4)) == 0


def test_flag_off_runs_nothing_and_the_other_files_are_unchanged(single_runs):
    e0, t0, errs0, d0, calls0 = single_runs["plain"]
    e1, t1, _, d1, _ = single_runs["flag"]
    assert _ok(e0) and _ok(e1) and type(e0) is type(e1)
    assert calls0 == 0 and not stderr_lines(errs0)
    a, b = _files(d0), _files(d1)
    assert not [k for k in a if "read_calls" in k]
    assert b.pop("read_calls_1.tsv")
    assert a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert _result_lines(t0) and _result_lines(t0) == _result_lines(t1)


@pytest.fixture(scope="module")
def pair_runs(L, mid_dbs, pair, tmp_path_factory):      # noqa: F811
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("rc_pair")

    def go():
        out = {}
        for name, extra in (("mates", []), ("pairs", ["--pairs"])):
            od = str(root / name)
            before = L.read_calls_calls()
            err, _, text, errs = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od,
                                                        "--classify_reads", str(M), "--read_calls"] + extra)
            out[name] = (err, text, errs, od, L.read_calls_calls() - before)
        return out
    return _with_cache(root, go)


def test_two_files_without_pairs(pair_runs, pair, tm):      # noqa: F811
    err, _, errs, od, calls = pair_runs["mates"]
    assert _ok(err), err
    texts = [b"".join(t for t, _ in pair["recs"][m]) for m in range(2)]
    got = [open(os.path.join(od, "read_calls_%d.tsv" % i), "rb").read() for i in (1, 2)]
    assert got == model_files(tm["DB_M"], texts, M)
    assert 2 <= calls <= 4 and len(stderr_lines(errs)) == 2                                   # the mates are classified independently
    assert node_histogram(*got) == direct_column(od)


def test_two_files_with_pairs(pair_runs, pair, tm):      # noqa: F811
    err, _, errs, od, calls = pair_runs["pairs"]
    assert _ok(err), err
    texts = [b"".join(t for t, _ in pair["recs"][m]) for m in range(2)]
    got = [open(os.path.join(od, "read_calls_%d.tsv" % i), "rb").read() for i in (1, 2)]
    assert got == model_files(tm["DB_M"], texts, M, joined=True)
    assert 1 <= calls <= 2 and len(stderr_lines(errs)) == 2
    rows = [[ln.split(b"\t") for ln in g.split(b"\n")[1:-1]] for g in got]
    assert len(rows[0]) == len(rows[1]) == len(pair["recs"][0])
    assert all(a[1:3] + a[4:] == b[1:3] + b[4:] and a[0][:-2] == b[0][:-2] for a, b in zip(*rows))      # mates share node, score and hits
    assert Counter(r[1].decode() for r in rows[0]) == direct_column(od)                                     # counted once per pair
    assert got != [open(os.path.join(pair_runs["mates"][3], "read_calls_%d.tsv" % i), "rb").read() for i in (1, 2)]


def test_multi_db_writes_one_file_set_per_label(L, mid_dbs, tm, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    fq, data = mid_dbs["reads"]["M_mix"]
    dbm, dbmem = mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]
    before = L.read_calls_calls()
    err, rc, _, errs = _run(multi_db.main, ["-i", fq, "-d", dbm, "-d", "mem=" + dbmem, "-o", str(tmp_path / "out"), "--classify_reads", str(M),
                                            "--read_calls"])
    assert err is None and rc == 0
    assert before + 2 <= L.read_calls_calls() <= before + 4
    for label, name in ((os.path.basename(os.path.normpath(dbm)), "DB_M"), ("mem", "DB_Mmem")):
        od = os.path.join(str(tmp_path / "out"), label)
        got = open(os.path.join(od, "read_calls_1.tsv"), "rb").read()
        assert got == model_files(tm[name], [data], M)[0], label
        assert node_histogram(got) == direct_column(od)
    assert len(stderr_lines(errs)) == 2
    assert not os.path.exists(os.path.join(str(tmp_path / "out"), "read_calls_1.tsv"))


def test_sample_not_resident(L, single_runs, mid_dbs, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    from strainscan_amd import db as ssdb
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    monkeypatch.setattr(ssdb, "RESIDENT_LIMIT_BYTES", 0)
    fq, _ = mid_dbs["reads"]["M_mix"]
    before = L.read_calls_calls()
    od = str(tmp_path / "out")
    err, _, text, errs = _run(StrainScan.main, ["-i", fq, "-d", mid_dbs["DB_M"]["db_dir"], "-o", od, "--classify_reads", str(M), "--read_calls"])
    lines = stderr_lines(errs)
    assert len(lines) == 1 and "--classify_reads was skipped" in lines[0] and "no per-read table was written" in lines[0], lines
    assert type(err) is type(single_runs["plain"][0]) and L.read_calls_calls() == before
    assert not [k for k in _files(od) if "read_calls" in k]
    assert _result_lines(text) == _result_lines(single_runs["plain"][1])


def test_two_ranks_skip_the_table_and_keep_read_classes(single_runs, mid_dbs, tmp_path):
    """Two ranks on one GPU (fresh child processes, gloo): the table is not written, one line says so, read_classes.tsv is the
    single process's"""
    od = str(tmp_path / "out")
    fq, _ = mid_dbs["reads"]["M_mix"]
    code = WORKER % dict(repo=REPO, seed=sc.POISSON_SEED,
                         argv=["-i", fq, "-d", mid_dbs["DB_M"]["db_dir"], "-o", od, "--classify_reads", str(M), "--read_calls"])
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", SS_IMAGE_CACHE=str(tmp_path / "cache"),
                   SS_TEST_STORE=str(tmp_path / "store"))
        procs.append(subprocess.Popen([sys.executable, "-c", code], env=env, stderr=subprocess.PIPE))
    errs = [p.communicate(timeout=300)[1].decode()[-3000:] for p in procs]
    assert all(p.returncode == 0 for p in procs), errs
    lines = [ln for e in errs for ln in stderr_lines(e)]
    assert len(lines) == 1 and "one rank only" in lines[0] and "no per-read table was written" in lines[0], lines
    assert not [k for k in _files(od) if "read_calls" in k]
    assert open(os.path.join(od, "read_classes.tsv")).read() == open(os.path.join(single_runs["flag"][3], "read_classes.tsv")).read()
