#!/usr/bin/env python3
"""What `--bootstrap_clusters` costs on the device, at the benchmark's shape: the sampled tree table of bench.py (823 leaves, 25.8 M
rows, behind its Bloom filter) and N reads of 150 bases, as a packed set and in file order.

  new        one ReadSet.scan_resampled call at n = 1, 4 and 16 (record index, spans, weights, the weighted scan, slots -> rows);
             device events around the synchronous call, the median of --reps after a warm-up, and the wall time
  existing   n times the route a materialised replicate takes, in the same process: resample -> order -> reset -> scan ->
             counts_rows_dev (-> destroy), timed as one block
  load       one vector of the new call's buffer loaded into the table (ss_counts_load_rows_dev), what a replicate's walk starts with
Every step also says whether replicate 0 of the new call equals the existing route's vector.
    bench_cluster_bootstrap.py [--reads N] [--leaves L] [--reps R] [--ns 1,4,16]
-> one JSON line per step (profiles/r28_cluster_bootstrap.md)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.bench_extract_reads import events, med  # noqa: E402


def spread(v):
    return [round(min(v), 3), round(max(v), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--leaves", type=int, default=823)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ns", default="1,4,16")
    args = ap.parse_args()
    import torch
    import bench
    from strainscan_amd import _lib
    dev = torch.device("cuda", 0)
    spec = bench.make_db(torch, dev, args.leaves, 1, shape="sampled", hit_frac=0.05)
    reads = bench.make_reads(torch, dev, spec, args.reads, 2, 0.05)
    db = _lib.KmerDB(spec["keys"], np.ones(spec["keys"].size, np.uint8), bench.K, True)
    info = db.info()
    row_buf = _lib.ReplicateCounts(1, db.n_rows)
    for layout, order in (("packed", True), ("file_order", False)):
        rs = _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=order)
        for n in [int(v) for v in args.ns.split(",")]:
            keep = {}

            def new():
                out = rs.scan_resampled(db, 1, 0, n)
                if "v" not in keep:
                    keep["v"] = out.row_vector(0)
                out.close()

            def existing():
                for j in range(n):
                    sub = rs.resample(1, j)
                    try:
                        db.reset()
                        sub.order().scan_into(db)
                        db.counts_rows_dev(row_buf.dptr)
                        _lib.check(_lib.lib().ss_device_sync(), "sync")
                        if j == 0 and "w" not in keep:
                            keep["w"] = row_buf.row_vector(0)
                    finally:
                        sub.close()
            ms_new, wall_new = events(torch, new, args.reps)
            ms_old, wall_old = events(torch, existing, args.reps)
            print(json.dumps(dict(step="replicates", layout=layout, reads=args.reads, rows=db.n_rows, n_slots=info["n_slots"],
                                  filter_bits=info["filter_bits"], packed_slabs=rs.packed_slabs(), n=n, reps=args.reps,
                                  new_ms=med(ms_new), new_ms_min_max=spread(ms_new), new_wall_ms=med(wall_new),
                                  existing_ms=med(ms_old), existing_ms_min_max=spread(ms_old), existing_wall_ms=med(wall_old),
                                  existing_over_new=round(med(wall_old) / med(wall_new), 2), hits=int(keep["v"].astype(np.uint64).sum()),
                                  equal=bool(np.array_equal(keep["v"], keep["w"])))), flush=True)
        out = rs.scan_resampled(db, 1, 0, 1)
        ms_load, _ = events(torch, lambda: (out.load_into(db, 0), _lib.check(_lib.lib().ss_device_sync(), "sync")), args.reps)
        out.close()
        print(json.dumps(dict(step="load", layout=layout, rows=db.n_rows, load_ms=med(ms_load), load_ms_min_max=spread(ms_load))), flush=True)
        rs.close()
    row_buf.close()
    db.close()


if __name__ == "__main__":
    main()
