#!/usr/bin/env python3
"""What `-x N` costs on a BAM sample: ss_bam_extract of the BAM of scripts/bench_bam.py (--reads reads of 150 bases, unaligned,
htslib-style members) against two tables made from the sample's own reads --
    tree     one 31-mer of every second read (a sampled table): N = 1 selects half the sample
    cluster  every 31-mer of --cluster-reads reads (a table that holds all k-mers of what it describes): N = 16 selects those reads
-- split into the steps ss_bam_extract_timing reports (the library's host clock around steps that each end with the stream
synchronised: stream on the device, walk + decode, hits, join, gather, download, compress + write), the median of --reps calls
after a warm-up.  Beside them: ss_reads_load of the same BAM (the feature repeats its inflate and decode per table); `-x 16`'s
FASTQ path on the same reads as a bgzip FASTQ (load, ReadSet.select, read back, digests, ss_extract_write); and, unless --no-cli,
the wall time of fresh `strainscan -i S.bam` processes without and with `-x 16` (--cli-root DIR: another checkout's command
without the flag, for the comparison with the commit before).
    bench_extract_bam.py [--reads N] [--cluster-reads N] [--reps R] [--no-cli] [--no-fastq] [--cli-root DIR]
-> one JSON line (profiles/r20_extract_bam.md)."""
import argparse
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench_bam  # noqa: E402

K = 31


def say(what):
    print("[bench_extract_bam] " + what, file=sys.stderr, flush=True)


def med(v):
    return round(float(np.median(v)), 2)


def sample_kmers(n_reads, every, per_read, limit=None):
    """the FASTA text of a table from the sample's own reads: `per_read` 31-mers (all: None) of every `every`-th read"""
    lut = np.frombuffer(b"ACTG", np.uint8)
    per = max(1, 250000 * 150 // bench_bam.L_READ)
    out, taken = [], 0
    for i in range((n_reads + per - 1) // per):
        n = min(per, n_reads - i * per)
        codes, _ = bench_bam._reads(1000 + i, n)
        rows = lut[codes[::every]]
        if limit is not None:
            rows = rows[:max(0, limit - taken)]
        taken += rows.shape[0]
        starts = range(bench_bam.L_READ - K + 1) if per_read is None else range(per_read)
        for s in starts:
            km = np.empty((rows.shape[0], 3 + K + 1), np.uint8)
            km[:, :3] = np.frombuffer(b">1\n", np.uint8)
            km[:, 3:3 + K] = rows[:, s:s + K]
            km[:, -1] = 10
            out.append(km.tobytes())
        if limit is not None and taken >= limit:
            break
    return b"".join(out)


def extract_steps(_lib, bam, db, n, out_path, reps):
    steps = {k: [] for k in _lib.BAM_EXTRACT_STEPS}
    walls, c = [], None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        c = _lib.bam_extract(bam, db, n, out_path)
        wall = (time.perf_counter() - t0) * 1e3
        if r:                                   # (the first call warms the pool and the pinned buffers)
            walls.append(wall)
            for k, v in _lib.bam_extract_timing().items():
                steps[k].append(v)
    return dict(min_hits=n, rows=db.n_rows, counters=c, out_mb=round(os.path.getsize(out_path) / 1e6, 1), wall_ms=med(walls),
                wall_ms_min_max=[round(min(walls), 1), round(max(walls), 1)], steps_ms={k: med(v) for k, v in steps.items()})


def fastq_path(_lib, fq_gz, db, n, d):
    """-x's FASTQ path on the same reads, step by step, once (wall, ms)"""
    out = {}
    t0 = time.perf_counter()
    rs = _lib.ReadSet([fq_gz])
    _lib.check(_lib.lib().ss_device_sync(), "sync")
    out["load"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    sub = rs.select(db, n)
    out["selected"] = sub.info()["n_records"]
    out["select"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    flat = sub.read_back()
    sub.close()
    out["read_back"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    keys = _lib.flat_record_keys(flat)
    out["digests"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    c = _lib.extract_write([fq_gz], keys, [os.path.join(d, "x_1.fastq")])
    out["extract_write"] = (time.perf_counter() - t0) * 1e3
    out["written"] = c["written"]
    rs.close()
    out["total"] = out["load"] + out["select"] + out["read_back"] + out["digests"] + out["extract_write"]
    return {k: round(v, 1) if isinstance(v, float) else v for k, v in out.items()}


def cli_runs(root, bam, db_dir, d, extra, runs):
    env = dict(os.environ, SS_IMAGE_CACHE=os.path.join(d, "cache_" + str(abs(hash(root)) % 1000)))
    ts = []
    say("fresh processes in %s %s" % (root, extra))
    for _ in range(runs + 1):
        o = os.path.join(d, "out_cli")
        shutil.rmtree(o, ignore_errors=True)
        t0 = time.perf_counter()
        subprocess.run([sys.executable, "-m", "strainscan_amd.StrainScan", "-i", bam, "-d", db_dir, "-o", o] + extra,
                       env=env, cwd=root, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
        ts.append(round(time.perf_counter() - t0, 3))
    return dict(median=round(float(np.median(ts[1:])), 3), all=ts)      # (the first run writes the image cache: not counted)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--cluster-reads", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--no-fastq", action="store_true")
    ap.add_argument("--cli-root", default=None, help="another checkout (built) whose plain `strainscan -i S.bam` is timed beside this one's")
    a = ap.parse_args()
    from strainscan_amd import _lib
    _lib.require_gpu()
    d = tempfile.mkdtemp(prefix="ss_bench_xbam_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = dict(reads=a.reads, read_len=bench_bam.L_READ, reps=a.reps)
    try:
        t0 = time.perf_counter()
        p = bench_bam.make_sample(d, a.reads, a.procs)
        out["generate_s"] = round(time.perf_counter() - t0, 1)
        out["bam_mb"] = round(os.path.getsize(p["bam"]) / 1e6, 1)
        say("sample written (%.0f s)" % out["generate_s"])
        _lib.warm_up(gz=1)
        bench_bam.load_ms(_lib, p["bam"])
        out["load_ms"] = med([bench_bam.load_ms(_lib, p["bam"])[0] for _ in range(a.reps)])
        os.environ.pop("SS_GZ_GPU", None)
        tables = dict(tree=(sample_kmers(a.reads, 2, 1), 1), cluster=(sample_kmers(a.reads, 7, None, a.cluster_reads), 16))
        say("tables made")
        for name, (kfa, n) in tables.items():
            db = _lib.KmerDB.from_text(kfa, K, True)
            try:
                o = os.path.join(d, name + ".bam")
                out[name] = extract_steps(_lib, p["bam"], db, n, o, a.reps)
                say("%s: %s" % (name, json.dumps(out[name])))
                # the file is a BAM of the written records
                with open(o, "rb") as f:
                    head = gzip.GzipFile(fileobj=f).read(4)
                assert head == b"BAM\1"
                if name == "cluster" and not a.no_fastq:
                    out["fastq_path_x16_ms"] = fastq_path(_lib, p["fq_gz"], db, n, d)
                    say("fastq path: %s" % json.dumps(out["fastq_path_x16_ms"]))
            finally:
                db.close()
        if not a.no_cli:
            from tests import scenarios_mid as sm
            info = sm.build_mid(d)
            out["cli_s"] = dict(plain=cli_runs(ROOT, p["bam"], info["db_dir"], d, [], 3),
                                x16=cli_runs(ROOT, p["bam"], info["db_dir"], d, ["-x", "16"], 3))
            if a.cli_root:
                out["cli_s"]["plain_other_checkout"] = cli_runs(os.path.abspath(a.cli_root), p["bam"], info["db_dir"], d, [], 3)
                out["cli_s"]["plain_again"] = cli_runs(ROOT, p["bam"], info["db_dir"], d, [], 3)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
