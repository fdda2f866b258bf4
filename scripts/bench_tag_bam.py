#!/usr/bin/env python3
"""What `--tag_bam` costs: ss_bam_tag_file of the BAM of scripts/bench_bam.py (--reads reads of 150 bases, unaligned, htslib-style
members) against the sampled tree table bench.py measures (823 leaves, 1645 nodes; node h of its heap-ordered binary tree is
node h + 1 here), M = 1 -- split into the eight steps ss_bam_tag_timing reports (the library's host clock around steps that each
end with the stream synchronised), plain and with `pairs`, the median of --reps calls after a warm-up.  Beside them, on the same
file and table: ss_bam_extract (N = 1) for the steps the two share -- stream, walk + decode, download, compress + write -- and
ss_reads_classify of the same reads loaded as a resident set, for the classify step.
    bench_tag_bam.py [--reads N] [--leaves C] [--reps R]
-> one JSON line (profiles/r26_tag_bam.md)."""
import argparse
import gzip
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench_bam  # noqa: E402


def say(what):
    print("[bench_tag_bam] " + what, file=sys.stderr, flush=True)


def med(v):
    return round(float(np.median(v)), 2)


def steps_of(call, timing, names, reps):
    steps = {k: [] for k in names}
    walls, c = [], None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        c = call()
        wall = (time.perf_counter() - t0) * 1e3
        if r:                                   # (the first call warms the pool and the pinned buffers)
            walls.append(wall)
            for k, v in timing().items():
                steps[k].append(v)
    return dict(counters=c, wall_ms=med(walls), wall_ms_min_max=[round(min(walls), 1), round(max(walls), 1)],
                steps_ms={k: med(v) for k, v in steps.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--leaves", type=int, default=823)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="ss_bench_tag_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = dict(reads=a.reads, read_len=bench_bam.L_READ, reps=a.reps)
    try:
        t0 = time.perf_counter()
        p = bench_bam.make_sample(d, a.reads, a.procs)                  # (worker processes: before this one opens the device)
        out["generate_s"] = round(time.perf_counter() - t0, 1)
        out["bam_mb"] = round(os.path.getsize(p["bam"]) / 1e6, 1)
        say("sample written (%.0f s)" % out["generate_s"])
        import torch
        import bench
        from strainscan_amd import _lib
        _lib.require_gpu()
        _lib.warm_up(gz=1)
        dev = torch.device("cuda", 0)
        spec = bench.make_db(torch, dev, a.leaves, 1, shape="sampled", hit_frac=0.05)
        n = int(spec["n_nodes"])
        row_node = np.zeros(spec["keys"].size, np.uint32)
        row_node[spec["rows"]] = np.repeat(np.arange(1, n + 1, dtype=np.uint32), np.diff(spec["row_off"].astype(np.int64)))
        parent = np.zeros(n + 1, np.uint32)
        parent[2:] = (np.arange(1, n) - 1) // 2 + 1
        value = np.arange(-1, n, dtype=np.int32)
        value[1:] = np.arange(1, n + 1)
        db = _lib.KmerDB(spec["keys"], np.ones(spec["keys"].size, np.uint8), bench.K, True)
        out.update(rows=db.n_rows, nodes=n)
        say("table made")
        try:
            o = os.path.join(d, "tagged.bam")
            for name, pairs in (("tag", False), ("tag_pairs", True)):
                out[name] = steps_of(lambda: _lib.bam_tag_file(p["bam"], db, row_node, parent, 1, value, o, pairs=pairs), _lib.bam_tag_timing,
                                     _lib.BAM_TAG_STEPS, a.reps)
                out[name]["out_mb"] = round(os.path.getsize(o) / 1e6, 1)
                say("%s: %s" % (name, json.dumps(out[name])))
                with open(o, "rb") as f:
                    assert gzip.GzipFile(fileobj=f).read(4) == b"BAM\1"
            o = os.path.join(d, "extracted.bam")
            out["extract"] = steps_of(lambda: _lib.bam_extract(p["bam"], db, 1, o), _lib.bam_extract_timing, _lib.BAM_EXTRACT_STEPS, a.reps)
            out["extract"]["out_mb"] = round(os.path.getsize(o) / 1e6, 1)
            say("extract: %s" % json.dumps(out["extract"]))
            rs = _lib.ReadSet([p["bam"]])
            try:
                ts = []
                for _ in range(a.reps + 1):
                    _lib.check(_lib.lib().ss_device_sync(), "sync")
                    t0 = time.perf_counter()
                    res = rs.classify(db, row_node, parent, 1)
                    ts.append((time.perf_counter() - t0) * 1e3)
                out["classify_resident"] = dict(wall_ms=med(ts[1:]), wall_ms_min_max=[round(min(ts[1:]), 1), round(max(ts[1:]), 1)],
                                                packed_slabs=rs.packed_slabs(), classified=int(res["direct"][1:].sum()),
                                                equal_direct=bool(int(res["direct"][1:].sum()) == out["tag"]["counters"]["classified"]))
            finally:
                rs.close()
        finally:
            db.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
