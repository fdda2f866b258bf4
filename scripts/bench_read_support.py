#!/usr/bin/env python3
"""What `--read_support` costs next to the scan it follows: ReadSet.support beside ReadSet.scan_into of the same (table, read
set) pair in one process, at the two shapes bench.py measures --
    tree     the sampled tree table (823 leaves, ~25 M rows, behind its Bloom filter) and 20 M reads of a three-strain mix
    cluster  a 10 M-row cluster table (every 31-mer of a 5 Mb genome, both orientations; ss_db_expect_hits) and 20 M reads of it
both against the binned (packed) resident set.  Device events around each call, the median of `--reps` after a warm-up; the
support call is synchronous (three passes, a copy back of the histogram), so its wall time is given too.
    bench_read_support.py [--reads N] [--cluster-genome G] [--leaves C] [--reps R] [--only tree|cluster]
-> one JSON line per shape (profiles/r11_read_support.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(torch, name, db, rs, reps, n_reads):
    stream = torch.cuda.current_stream().cuda_stream

    def events(fn):
        ts, walls = [], []
        for _ in range(reps + 1):
            db.reset(stream)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            ts.append(a.elapsed_time(b))
        return ts[1:], walls[1:]

    scan_ms, _ = events(lambda: rs.scan_into(db, stream))
    scan_hits = int(db.counts_rows().astype(np.int64).sum())
    got = {}
    sup_ms, sup_wall = events(lambda: got.update(zip(("hist", "hits"), rs.support(db))))
    hist = got["hist"]
    return dict(shape=name, rows=db.n_rows, reads=n_reads, records=int(hist.sum()), packed_slabs=rs.packed_slabs(),
                scan_ms=round(float(np.median(scan_ms)), 3), scan_ms_min_max=[round(min(scan_ms), 3), round(max(scan_ms), 3)],
                support_ms=round(float(np.median(sup_ms)), 3), support_ms_min_max=[round(min(sup_ms), 3), round(max(sup_ms), 3)],
                support_wall_ms=round(float(np.median(sup_wall)), 3),
                support_over_scan=round(float(np.median(sup_ms)) / float(np.median(scan_ms)), 2),
                hits=got["hits"], hits_equal_scan=bool(got["hits"] == scan_hits), ge1=int(hist[1:].sum()), ge64=int(hist[64]), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--cluster-genome", type=int, default=5_000_000)
    ap.add_argument("--leaves", type=int, default=823)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["tree", "cluster"])
    args = ap.parse_args()
    import torch
    import bench
    from strainscan_amd import _lib
    dev = torch.device("cuda", 0)
    if args.only != "cluster":
        spec = bench.make_db(torch, dev, args.leaves, 1, shape="sampled", hit_frac=0.05)
        reads = bench.make_reads(torch, dev, spec, args.reads, 2, 0.05)
        db = _lib.KmerDB(spec["keys"], np.ones(spec["keys"].size, np.uint8), bench.K, True)
        rs = _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=True)
        print(json.dumps(measure(torch, "tree", db, rs, args.reps, args.reads)), flush=True)
        rs.close()
        db.close()
        del spec, reads
        torch.cuda.empty_cache()
    if args.only != "tree":
        G = args.cluster_genome
        g = torch.Generator(device=dev)
        g.manual_seed(3)
        genome = torch.randint(0, 4, (G + 200,), generator=g, device=dev, dtype=torch.uint8)
        key, rc, _, _ = bench._kmer_keys(torch, genome, torch.arange(0, G, device=dev), dev)
        keys = torch.stack([key, rc], 1).reshape(-1).cpu().numpy().view(np.uint64)
        reads = bench.reads_of(torch, dev, [genome], [args.reads], g)
        db = _lib.KmerDB(keys, np.ones(keys.size, np.uint8), bench.K, True).expect_hits()
        rs = _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=True)
        print(json.dumps(measure(torch, "cluster", db, rs, args.reps, args.reads)), flush=True)
        rs.close()
        db.close()


if __name__ == "__main__":
    main()
