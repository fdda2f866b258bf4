"""`strainscan-multi` on the MI355X: the several-tables scan with every tree table behind its own Bloom filter
(ss_scan_reads_multi) bit-exact against one ss_scan_reads per table and against the oracle; the whole command against
single `strainscan` runs in the same process (file for file, byte for byte, and the printed layer-1 dicts); one ingest and
one tree index per database; sharded ranks; the fallback without a resident read set."""
import ast
import contextlib
import gzip
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import scenarios as sc
from tests import scenarios_fuzz as sf
from tests import scenarios_mid as sm
from tests import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


# ------------------------------------------------------------------------------------------------
# 1. kernel parity
# ------------------------------------------------------------------------------------------------
def _tree_tables(seed, n_tables, G=30000, density=0.35):
    """n_tables tree-like k-mer FASTA texts: a sampled share of the k-mers of a genome of their own (both strands), so every
    table gets a Bloom filter and sees hits only from the reads of its own genome.  -> (texts, genomes)"""
    rs = np.random.RandomState(seed)
    lut = np.frombuffer(b"ACGT", np.uint8)
    texts, genomes = [], []
    for _ in range(n_tables):
        g = lut[rs.randint(0, 4, size=G)].tobytes()
        pick = np.nonzero(rs.random_sample(G - 30) < density)[0]
        kms = [g[i:i + 31] for i in pick] + [synth.revcomp(g[i:i + 31]) for i in pick[::3]]
        texts.append(b"".join(b">1\n" + km + b"\n" for km in kms))
        genomes.append(g)
    return texts, genomes


def _reads(seed, genomes, n_reads=12000, L_=150):
    """Reads of one length (binned sets hold them packed): most from genome 0, some from genome 1, the rest random."""
    rs = np.random.RandomState(seed)
    lut = np.frombuffer(b"ACGT", np.uint8)
    recs = []
    for i in range(n_reads):
        u = rs.random_sample()
        src = genomes[0] if u < 0.5 else genomes[1 % len(genomes)] if u < 0.6 else None
        if src is None:
            r = lut[rs.randint(0, 4, size=L_)].copy()
        else:
            s = rs.randint(0, len(src) - L_)
            r = np.frombuffer(src[s:s + L_], np.uint8).copy()
            m = rs.random_sample(L_) < 0.005
            r[m] = lut[rs.randint(0, 4, size=int(m.sum()))]
        if rs.random_sample() < 0.03:
            r[rs.randint(0, L_)] = ord("N")
        b = r.tobytes()
        recs.append(synth.revcomp(b) if rs.random_sample() < 0.5 else b)
    flat = b"\n".join(recs) + b"\n"
    fq = b"".join(b"@r\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for r in recs)
    return flat, fq


@pytest.mark.parametrize("n_tree", [1, 2, 4, 5, 9])
def test_fused_tree_tables_equal_single_scans(L, n_tree):
    """1-9 tree tables (Bloom filters, few hits: groups of four, and a group of one, are crossed) plus a cluster table that
    expects hits, in ONE ss_scan_reads_multi call: every table's counts equal ss_scan_reads on it alone, bit for bit, for a
    binned packed set, a binned ASCII set (ss_test_hook 5) and a set in file order; table 0 also equals the oracle."""
    import torch
    from oracle import oracle as orc
    texts, genomes = _tree_tables(500 + n_tree, n_tree + 1)
    flat, fq = _reads(600 + n_tree, genomes)
    trees = [L.KmerDB.from_text(t, 31, True) for t in texts[:n_tree]]
    assert all(db.info()["filter_bits"] > 0 for db in trees), "every tree table needs its Bloom filter for this test"
    g0 = genomes[0]
    dense = b"".join(b">1\n" + g0[i:i + 31] + b"\n>1\n" + synth.revcomp(g0[i:i + 31]) + b"\n" for i in range(0, 12000))
    cluster = L.KmerDB.from_text(dense, 31, True).expect_hits()
    tables = trees[:2] + [cluster] + trees[2:]                     # the cluster table in the middle of the list
    want_orc, _ = orc.jellyfish_count(texts[0], [fq], k=31, upper=True)
    d = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    for mode in ("packed", "ascii", "file"):
        L.check(L.lib().ss_test_hook(5, 1 if mode == "ascii" else 0), "ss_test_hook")
        try:
            rs = L.ReadSet.from_flat_dev(d.data_ptr(), d.numel(), order=mode != "file")
        finally:
            L.lib().ss_test_hook(5, 0)
        assert (rs.packed_slabs() > 0) == (mode == "packed"), mode
        want = []
        for db in tables:
            db.reset()
            rs.scan_into(db)
            L.check(L.lib().ss_device_sync(), "sync")
            want.append(db.counts_rows())
            db.reset()
        assert want[0].sum() > 50_000 and want[tables.index(cluster)].sum() > 50_000
        if n_tree > 2:
            assert want[3].sum() < want[0].sum() // 20          # a table of another genome: (almost) nothing
        before = L.scan_multi_launches()
        rs.scan_into_many(tables)
        L.check(L.lib().ss_device_sync(), "sync")
        after = L.scan_multi_launches()
        for i, (db, w) in enumerate(zip(tables, want)):
            assert np.array_equal(db.counts_rows(), w), (mode, n_tree, i)
        assert np.array_equal(tables[0].counts_rows(), want_orc), mode
        # the tree tables go four at a time through the Bloom variant (a group of one through the single-table scan), the
        # cluster table on its own; nothing through the filterless several-tables kernel
        fused = any(min(4, n_tree - g) > 1 for g in range(0, n_tree, 4))
        assert (after["bloom"] > before["bloom"]) == fused, (mode, before, after)
        assert after["plain"] == before["plain"] and after["expect_hits"] == before["expect_hits"]
        rs.close()
    for db in tables:
        db.close()


def test_multi_launch_export_is_declared(L):
    import ctypes as C
    out = (C.c_uint64 * 3)()
    assert L.lib().ss_scan_multi_launches(out) == 0
    assert L.lib().ss_scan_multi_launches(None) != 0


# ------------------------------------------------------------------------------------------------
# 2. the whole command against single runs
# ------------------------------------------------------------------------------------------------
FLOW_SEEDS = [0, 2, 28]


@pytest.fixture(scope="module")
def flow_dbs(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("ss_multi_flow"))
    return [sf.build_flow(s, root) for s in FLOW_SEEDS]


@pytest.fixture(scope="module")
def samples(mid_dbs, flow_dbs, tmp_path_factory):
    """name -> (fq1, fq2): the mid samples as .fq, M_mix as a .fastq.gz pair, and a flow database's own sample."""
    root = tmp_path_factory.mktemp("ss_multi_reads")
    out = {n: (mid_dbs["reads"][n][0], "") for n in ("M_mix", "M_one", "M_low")}
    data = mid_dbs["reads"]["M_mix"][1]
    recs = data.split(b"\n@")
    h = len(recs) // 2
    p1, p2 = root / "mix_R1.fastq.gz", root / "mix_R2.fastq.gz"
    p1.write_bytes(gzip.compress(b"\n@".join(recs[:h]) + b"\n", 6))
    p2.write_bytes(gzip.compress(b"@" + b"\n@".join(recs[h:]), 6))
    out["M_mix_gz"] = (str(p1), str(p2))
    f = root / "flow0.fq"
    f.write_bytes(sf.flow_reads(flow_dbs[0], FLOW_SEEDS[0]))
    out["flow0"] = (str(f), "")
    return out


def _all_dbs(mid_dbs, built_db, flow_dbs):
    return ([mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"], os.path.dirname(built_db["tdb"])]
            + [f["db_dir"] for f in flow_dbs])


def _files(d):
    out = {}
    for root, _, fs in os.walk(d):
        for f in fs:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def _dicts(text):
    """The printed layer-1 dicts (the defaultdict's factory without its address)."""
    return [re.sub(r" at 0x[0-9a-f]+>", ">", ln) for ln in text.splitlines() if ln.startswith("defaultdict(") or ln.startswith("{")]


def _single(db_dir, fq, argv, out):
    from strainscan_amd import StrainScan
    from strainscan_amd import db as ssdb
    ssdb.clear_cache()
    np.random.seed(sc.POISSON_SEED)
    buf = io.StringIO()
    err = None
    cmd = ["-i", fq[0]] + (["-j", fq[1]] if fq[1] else []) + ["-d", db_dir, "-o", out] + list(argv)
    with contextlib.redirect_stdout(buf):
        try:
            StrainScan.main(cmd)
        except BaseException as e:      # noqa: B902 -- how the run ended is part of what is compared
            err = e
    text = buf.getvalue()
    if err is None:
        status = "reports"
    elif isinstance(err, SystemExit) and err.code is None:
        status = "single_cluster" if "Only single cluster is identified" in text else "no_clusters"
    else:
        status = "error:" + type(err).__name__
    return status, text


def _multi(dbs, fq, argv, out):
    from strainscan_amd import multi_db
    from strainscan_amd import StrainScan
    from strainscan_amd import db as ssdb
    import argparse
    ssdb.clear_cache()
    ap = argparse.ArgumentParser()
    StrainScan.add_arguments(ap)
    opts = StrainScan.settings(ap.parse_args(["-i", "x", "-d", "x"] + list(argv)))
    opts.pop("pmode")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rows = multi_db.identify_databases(fq, dbs, out, before_each=lambda i: np.random.seed(sc.POISSON_SEED), **opts)
    text = buf.getvalue()
    parts = {}
    for label, _, _ in rows:
        a = text.index("== database %s: " % label)
        b = text.find("== database ", a + 1)
        parts[label] = text[a:b if b >= 0 else len(text)]
    return rows, parts


CASES = [("M_mix", []), ("M_mix", ["-b", "1"]), ("M_mix", ["-l", "1"]), ("M_mix", ["-e", "1"]), ("M_mix", ["-k", "25"]),
         ("M_mix_gz", []), ("M_one", []), ("M_low", []), ("flow0", [])]


@pytest.mark.parametrize("sname,argv", CASES)
def test_whole_command_equals_single_runs(sname, argv, mid_dbs, built_db, flow_dbs, samples, golden_dir, tmp_path, monkeypatch):
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    fq = samples[sname]
    dbs = _all_dbs(mid_dbs, built_db, flow_dbs)
    out = str(tmp_path / "multi")
    rows, parts = _multi(dbs, fq, argv, out)
    from strainscan_amd import multi_db
    assert multi_db.read_table(os.path.join(out, multi_db.TSV)) == [(lb, os.path.abspath(d), st) for lb, d, st in rows]
    assert [r[0] for r in rows] == [os.path.basename(d) for d in dbs]
    for (label, d, status), db_dir in zip(rows, dbs):
        sout = str(tmp_path / "single" / label)
        want_status, want_text = _single(db_dir, fq, argv, sout)
        assert status == want_status, (sname, argv, label)
        assert _dicts(parts[label]) == _dicts(want_text), (sname, argv, label)
        got_files, want_files = _files(os.path.join(out, label)), _files(sout)
        assert sorted(got_files) == sorted(want_files), (sname, argv, label)
        for rel in want_files:
            assert got_files[rel] == want_files[rel], (sname, argv, label, rel)
    st = dict((r[0], r[2]) for r in rows)
    if sname == "M_mix" and not argv:
        assert st["DB_M"] == "reports" and "no_clusters" in [st[os.path.basename(f["db_dir"])] for f in flow_dbs]
    # the reference's own result where tests/golden/mid_flow.json holds one for this sample, database and flags
    if not fq[1]:
        g = json.load(open(os.path.join(golden_dir, "mid_flow.json")))
        for name, (gs, dbn, gargv) in sm.MID_FLOW.items():
            if gs != sname or list(gargv) != list(argv):
                continue
            want = g[name]
            label = dbn
            if want["error"] == "SystemExit":
                assert st[label] in ("no_clusters", "single_cluster"), (name, st[label])
            else:
                assert st[label] == ("error:" + want["error"] if want["error"] else "reports"), (name, st[label])
            if st[label] == "reports":
                got = ast.literal_eval(_dicts(parts[label])[-1][_dicts(parts[label])[-1].index("{"):].rstrip(")"))
                assert list(got) == list(ast.literal_eval(want["cls_dict"])), name
                assert sorted(_files(os.path.join(out, label))) == sorted(want["files"]), name


# ------------------------------------------------------------------------------------------------
# 3. one ingest, one tree index per database
# ------------------------------------------------------------------------------------------------
def test_one_ingest_and_one_index_per_database(L, mid_dbs, flow_dbs, samples, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    from strainscan_amd import db as ssdb
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    ssdb.clear_cache()
    made = []
    real_init = L.ReadSet.__init__

    def counted(self, *a, **k):
        made.append(a)
        real_init(self, *a, **k)

    monkeypatch.setattr(L.ReadSet, "__init__", counted)
    trees = []
    real_index = ssdb.TreeImage._index

    def index(db_dir, keys, flags, upper_keys):
        trees.append(os.path.realpath(db_dir))
        return real_index(db_dir, keys, flags, upper_keys)

    monkeypatch.setattr(ssdb.TreeImage, "_index", staticmethod(index))
    dbs = [mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]] + [f["db_dir"] for f in flow_dbs[:2]]
    ev0 = dict(ssdb.INDEX_EVENTS)
    bl0 = L.scan_multi_launches()
    with contextlib.redirect_stdout(io.StringIO()):
        rows = multi_db.identify_databases(samples["M_mix"], dbs, str(tmp_path / "out"))
    assert len(made) == 1, made
    assert sorted(trees) == sorted(os.path.realpath(d + "/Tree_database") for d in dbs)
    assert sum(ssdb.INDEX_EVENTS.values()) - sum(ev0.values()) >= len(dbs)
    assert L.scan_multi_launches()["bloom"] > bl0["bloom"]        # the four tree tables went through the fused Bloom pass
    assert rows[0][2] == "reports"
    ssdb.clear_cache()


# ------------------------------------------------------------------------------------------------
# 4. sharded
# ------------------------------------------------------------------------------------------------
WORKER = r'''
import contextlib, io, os, sys
import numpy as np
sys.path.insert(0, %(repo)r)
import torch
import torch.distributed as dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", init_method="file://" + os.environ["SS_TEST_STORE"], rank=rank, world_size=world)
from strainscan_amd import multi_db, dist as sdist
assert sdist.is_distributed()
out = %(out)r if rank == 0 else None
import tempfile
out = out or tempfile.mkdtemp()
with contextlib.redirect_stdout(io.StringIO()):
    multi_db.identify_databases(%(fq)r, %(dbs)r, out, before_each=lambda i: np.random.seed(%(seed)d), rank=rank)
dist.barrier()
dist.destroy_process_group()
'''


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_equals_world_one(world, mid_dbs, flow_dbs, samples, tmp_path, monkeypatch):
    import socket
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbs = [mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"], flow_dbs[0]["db_dir"]]
    fq = samples["M_mix"]
    one = str(tmp_path / "one")
    _multi(dbs, fq, [], one)
    out = str(tmp_path / "sharded")
    code = WORKER % dict(repo=REPO, out=out, fq=tuple(fq), dbs=dbs, seed=sc.POISSON_SEED)
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), SS_IMAGE_CACHE=str(tmp_path / "cache"), SS_TEST_STORE=str(tmp_path / ("store_%d" % port)))
        procs.append(subprocess.Popen([sys.executable, "-c", code], env=env, stderr=subprocess.PIPE))
    errs = [p.communicate(timeout=600)[1].decode()[-3000:] for p in procs]
    assert all(p.returncode == 0 for p in procs), errs
    assert _files(out) == _files(one)


# ------------------------------------------------------------------------------------------------
# 5. no resident read set
# ------------------------------------------------------------------------------------------------
def test_fallback_without_resident_reads(mid_dbs, flow_dbs, samples, tmp_path, monkeypatch, capsys):
    from strainscan_amd import db as ssdb
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbs = [mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"], flow_dbs[0]["db_dir"]]
    fq = samples["M_mix"]
    rows_a, parts_a = _multi(dbs, fq, ["-b", "1"], str(tmp_path / "a"))
    capsys.readouterr()
    monkeypatch.setattr(ssdb, "RESIDENT_LIMIT_BYTES", 0)
    rows_b, parts_b = _multi(dbs, fq, ["-b", "1"], str(tmp_path / "b"))
    assert "resident budget" in capsys.readouterr().err
    assert [r[2] for r in rows_a] == [r[2] for r in rows_b]
    assert _files(str(tmp_path / "a")).keys() == _files(str(tmp_path / "b")).keys()
    fa, fb = _files(str(tmp_path / "a")), _files(str(tmp_path / "b"))
    for rel in fa:
        assert fa[rel] == fb[rel], rel
    for lb in parts_a:
        assert _dicts(parts_a[lb]) == _dicts(parts_b[lb])
    ssdb.clear_cache()
