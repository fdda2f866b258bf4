"""`strainscan --classify_reads M` / `strainscan-multi --classify_reads M`: read_classes.tsv is the model's text
(tests/class_model.py) computed from the FASTQ bytes, kmer.fa, kmers/<id> and tree_structure.txt; stdout's result lines and every
other file are what a run without the flag writes; without the flag nothing new runs."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import class_model as cm, rs_model, synth
from tests import scenarios as sc
from tests.test_read_support_cli_gpu import WORKER, _files, _ok, _result_lines, _run

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TSV = "read_classes.tsv"


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def model_text(db_dir, flat, m, k=31):
    """read_classes.tsv for the sample `flat` (its flat bases) against db_dir/Tree_database, from the database's files alone"""
    tdb = os.path.join(db_dir, "Tree_database")
    with open(os.path.join(tdb, "kmer.fa"), "rb") as f:
        kmers = [km.upper() for km in rs_model.kmers_of_fasta(f.read())]
    keys = rs_model.encode_kmers(kmers, k)
    parent_of, has_children = {}, set()
    with open(os.path.join(tdb, "tree_structure.txt")) as f:
        for ln in f:
            t = ln.rstrip("\n").split("\t")
            parent_of[int(t[0])] = None if t[1] == "N" else int(t[1])
    for p in parent_of.values():
        has_children.add(p)
    listed = sorted(int(f) for f in os.listdir(os.path.join(tdb, "kmers")) if f.isdigit())
    node_ids = sorted(set(listed) | set(parent_of))
    num = {nid: v for v, nid in enumerate(node_ids, 1)}
    owner = {}                                   # row -> the node that lists it, 0 once two different nodes do
    for nid in listed:
        with open(os.path.join(tdb, "kmers", str(nid))) as f:
            for r in set(map(int, f.readline().split())):
                owner[r] = num[nid] if owner.get(r, num[nid]) == num[nid] else 0
    row_node = np.array([owner.get(r, 0) for r in range(len(kmers))], np.int64)
    parent = [0] * (len(node_ids) + 1)
    for nid in node_ids:
        if parent_of.get(nid) is not None:
            parent[num[nid]] = num[parent_of[nid]]
    direct, node_hits, kmers_n = cm.classify_model(flat, keys, row_node, parent, len(node_ids), k, m)
    leaves = {nid for nid in parent_of if nid not in has_children}
    return cm.report_text(node_ids, {nid: parent_of.get(nid) for nid in node_ids}, leaves, direct, node_hits, kmers_n), direct


@pytest.fixture(scope="module")
def mix(mid_dbs):
    fq, data = mid_dbs["reads"]["M_mix"]
    return fq, synth.flat_bases_from_fastx(data)


@pytest.fixture(scope="module")
def single_runs(L, mid_dbs, mix, tmp_path_factory):
    """`strainscan` on DB_M with M_mix, without and with the flag -> dict(plain=, flag=) of (err, stdout, out dir, calls made)"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("cls_cli")
    old = os.environ.get("SS_IMAGE_CACHE")
    os.environ["SS_IMAGE_CACHE"] = str(root / "cache")
    try:
        out = {}
        for name, extra in (("plain", []), ("flag", ["--classify_reads", "1"])):
            before = L.classify_calls()
            od = str(root / name)
            err, _, text = _run(StrainScan.main, ["-i", mix[0], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od] + extra)
            out[name] = (err, text, od, L.classify_calls() - before)
    finally:
        if old is None:
            os.environ.pop("SS_IMAGE_CACHE", None)
        else:
            os.environ["SS_IMAGE_CACHE"] = old
    return out


@pytest.fixture(scope="module")
def want(mid_dbs, mix):
    return model_text(mid_dbs["DB_M"]["db_dir"], mix[1], 1)


def test_flag_writes_the_models_text(single_runs, want):
    err, _, od, calls = single_runs["flag"]
    assert _ok(err), err
    text, direct = want
    got = open(os.path.join(od, TSV)).read()
    rows = [ln.split("\t") for ln in got.split("\n")[1:-1]]
    print("nodes", len(rows) - 1, "records", int(direct.sum()), "unclassified", int(direct[0]), "nodes with reads", int((direct[1:] > 0).sum()))
    assert got == text
    assert calls == 1
    assert rows[0][0] == "unclassified" and sum(int(r[5]) for r in rows) == int(direct.sum()) > 0
    assert int((direct[1:] > 0).sum()) >= 2 and any(r[2].startswith("C") and int(r[6]) > 0 for r in rows)
    roots = [r for r in rows[1:] if r[1] == "-"]
    assert len(roots) == 1 and int(roots[0][6]) == int(direct[1:].sum())             # the root's clade: every classified read


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


def test_the_stderr_line(L, mid_dbs, mix, want, tmp_path, monkeypatch, capsys):
    from strainscan_amd import StrainScan
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    capsys.readouterr()
    err, _, _ = _run(StrainScan.main, ["-i", mix[0], "-d", mid_dbs["DB_M"]["db_dir"], "-o", str(tmp_path / "out"), "--classify_reads", "2"])
    assert _ok(err)
    lines = [ln for ln in capsys.readouterr().err.split("\n") if ln.startswith("classify_reads:")]
    assert len(lines) == 1
    m = re.match(r"classify_reads: M=2\trecords (\d+)\tclassified (\d+)\tfrom a tie (\d+)$", lines[0])
    text2, direct2 = model_text(mid_dbs["DB_M"]["db_dir"], mix[1], 2)
    assert m and int(m.group(1)) == int(direct2.sum()) and int(m.group(2)) == int(direct2[1:].sum()) and int(m.group(3)) <= int(m.group(2))
    assert open(os.path.join(str(tmp_path / "out"), TSV)).read() == text2


def test_multi_db_writes_one_file_per_label(L, mid_dbs, mix, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbm, dbmem = mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]
    base = ["-i", mix[0], "-d", dbm, "-d", "mem=" + dbmem]
    before = L.classify_calls()
    e0, rc0, t0 = _run(multi_db.main, base + ["-o", str(tmp_path / "plain")])
    assert L.classify_calls() == before
    e1, rc1, t1 = _run(multi_db.main, base + ["-o", str(tmp_path / "flag"), "--classify_reads", "1"])
    assert L.classify_calls() == before + 2
    assert e0 is None and e1 is None and rc0 == 0 and rc1 == 0
    a, b = _files(str(tmp_path / "plain")), _files(str(tmp_path / "flag"))
    labels = [os.path.basename(os.path.normpath(dbm)), "mem"]
    for label, d in zip(labels, (dbm, dbmem)):
        rel = os.path.join(label, TSV)
        assert rel in b and rel not in a
        assert b.pop(rel).decode() == model_text(d, mix[1], 1)[0], label
    assert not [k for k in b if k.endswith(TSV)]
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert _result_lines(t0) == _result_lines(t1)


def test_sample_not_resident(L, single_runs, mid_dbs, mix, tmp_path, monkeypatch, capsys):
    from strainscan_amd import StrainScan
    from strainscan_amd import db as ssdb
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    monkeypatch.setattr(ssdb, "RESIDENT_LIMIT_BYTES", 0)
    capsys.readouterr()
    before = L.classify_calls()
    od = str(tmp_path / "out")
    err, _, text = _run(StrainScan.main, ["-i", mix[0], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od, "--classify_reads", "1"])
    lines = [ln for ln in capsys.readouterr().err.split("\n") if ln.startswith("classify_reads:")]
    assert len(lines) == 1 and "resident on the device" in lines[0] and "no read was classified" in lines[0], lines
    assert _ok(err) and L.classify_calls() == before
    e0, t0, d0, _ = single_runs["plain"]
    assert type(err) is type(e0)                                                      # the run ends the way it ends without the flag
    a, b = _files(d0), _files(od)
    assert TSV not in b and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert _result_lines(t0) == _result_lines(text)


def test_two_ranks_write_the_single_process_file(single_runs, mid_dbs, mix, tmp_path):
    """Two ranks on one GPU (fresh child processes, gloo): each classifies its shard, the integers are summed over the ranks, rank 0
    writes the file."""
    od = str(tmp_path / "out")
    code = WORKER % dict(repo=REPO, seed=sc.POISSON_SEED,
                         argv=["-i", mix[0], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od, "--classify_reads", "1"])
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
    assert sum(e.count("classify_reads: M=1") for e in errs) == 1                     # rank 0 alone says the line
