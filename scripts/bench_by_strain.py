#!/usr/bin/env python3
"""What `--by_strain` costs next to the call it extends: ReadSet.support_labeled at L = 1, 3 and 8 labels beside ReadSet.support
of the same (table, read set) pair in one process, at the cluster shape of bench_read_support.py --
    a 10 M-row cluster table (every 31-mer of a 5 Mb genome, both orientations; ss_db_expect_hits) and 20 M reads of it,
    binned (packed); the rows labelled at random, a fifth of them 0
Device events around each call, the median of `--reps` after a warm-up; both calls are synchronous, so the wall time is given
too.  The labelled call uploads the row labels and makes the slot labels on every call: that is part of what is measured.
--select N adds ReadSet.select / select_labeled (label 1 of 3) at that N.
    bench_by_strain.py [--reads N] [--cluster-genome G] [--reps R] [--labels 1,3,8] [--select N]
-> one JSON line (profiles/r18_by_strain.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def events(torch, fn, reps):
    ts, walls = [], []
    for _ in range(reps + 1):
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


def summary(ts, walls):
    return dict(ms=round(float(np.median(ts)), 3), ms_min_max=[round(min(ts), 3), round(max(ts), 3)], wall_ms=round(float(np.median(walls)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--cluster-genome", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--labels", default="1,3,8")
    ap.add_argument("--select", type=int, default=0)
    args = ap.parse_args()
    import torch
    import bench
    from strainscan_amd import _lib
    dev = torch.device("cuda", 0)
    G = args.cluster_genome
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    genome = torch.randint(0, 4, (G + 200,), generator=g, device=dev, dtype=torch.uint8)
    key, rc, _, _ = bench._kmer_keys(torch, genome, torch.arange(0, G, device=dev), dev)
    keys = torch.stack([key, rc], 1).reshape(-1).cpu().numpy().view(np.uint64)
    reads = bench.reads_of(torch, dev, [genome], [args.reads], g)
    db = _lib.KmerDB(keys, np.ones(keys.size, np.uint8), bench.K, True).expect_hits()
    rs = _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=True)
    out = dict(rows=db.n_rows, reads=args.reads, packed_slabs=rs.packed_slabs(), reps=args.reps)
    got = {}
    ts, walls = events(torch, lambda: got.update(plain=rs.support(db)), args.reps)
    out["support"] = summary(ts, walls)
    total = got["plain"][1]
    rng = np.random.RandomState(1)
    for nl in [int(x) for x in args.labels.split(",")]:
        lab = rng.randint(0, 5 * nl, size=db.n_rows)
        lab = np.where(lab < nl, 0, lab % nl + 1).astype(np.uint8)      # a fifth of the rows: label 0
        ts, walls = events(torch, lambda: got.update(lab=rs.support_labeled(db, lab, nl)), args.reps)
        hist, hits, kmers = got["lab"]
        s = summary(ts, walls)
        s.update(over_support=round(s["ms"] / out["support"]["ms"], 2), hits_labelled=int(hits.sum()), hits_all=total,
                 kmers_labelled=int(kmers.sum()))
        out["support_labeled_L%d" % nl] = s
    if args.select:
        def closing(fn):
            fn().close()
        ts, walls = events(torch, lambda: closing(lambda: rs.select(db, args.select)), args.reps)
        out["select"] = summary(ts, walls)
        lab = (rng.randint(0, 4, size=db.n_rows)).astype(np.uint8)
        ts, walls = events(torch, lambda: closing(lambda: rs.select_labeled(db, lab, 3, 1, args.select)), args.reps)
        out["select_labeled_1_of_3"] = summary(ts, walls)
        out["select_min_hits"] = args.select
    print(json.dumps(out), flush=True)
    rs.close()
    db.close()


if __name__ == "__main__":
    main()
