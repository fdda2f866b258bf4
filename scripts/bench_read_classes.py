#!/usr/bin/env python3
"""What `--classify_reads` costs: one ss_reads_classify call beside ss_reads_support of the same (table, read set) pair in one
process, at the tree shapes bench.py measures --
    sampled     the sampled tree table (823 leaves, 1645 nodes, ~25 M rows, behind its Bloom filter)
    contiguous  the same tree with every k-mer of each node's stretch
and 20 M reads of a three-strain mix, as the binned (packed) resident set and in file order.  The nodes are bench.py's: node h
of its heap-ordered binary tree is node h + 1 here, its rows those of its list.  Device events around each call, the median of
`--reps` after a warm-up; both calls are synchronous, so the wall time is given too.  M = 1; `classes`: rec_class requested.
    bench_read_classes.py [--reads N] [--leaves C] [--reps R] [--only sampled|contiguous] [--once]
-> one JSON line per (shape, layout) (profiles/r22_read_classes.md).  --once: one classify call per pair and nothing else (the
run a kernel trace is taken of)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(torch, name, layout, db, rs, row_node, parent, reps, n_reads):
    from strainscan_amd import _lib
    n = parent.size - 1
    bufs = [np.zeros(n + 1, np.uint64) for _ in range(3)]
    n_rec = int(rs.support(db, 2)[0].sum())
    classes = np.zeros(n_rec, np.uint32)

    def classify(want):
        _lib.check(_lib.lib().ss_reads_classify(db.handle, rs._h, _lib.ptr(row_node), n, _lib.ptr(parent), 1, _lib.ptr(bufs[0]),
                                                _lib.ptr(bufs[1]), _lib.ptr(bufs[2]), _lib.ptr(classes) if want else None), "ss_reads_classify")

    def events(fn):
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

    def med(v):
        return round(float(np.median(v)), 3)

    got = {}
    sup, sup_wall = events(lambda: got.update(hits=rs.support(db)[1]))
    cls, cls_wall = events(lambda: classify(False))
    direct, node_hits = bufs[0].copy(), bufs[1].copy()
    clc, clc_wall = events(lambda: classify(True))
    return dict(shape=name, layout=layout, rows=db.n_rows, nodes=n, reads=n_reads, records=n_rec, packed_slabs=rs.packed_slabs(),
                support_ms=med(sup), support_ms_min_max=[round(min(sup), 3), round(max(sup), 3)], support_wall_ms=med(sup_wall),
                classify_ms=med(cls), classify_ms_min_max=[round(min(cls), 3), round(max(cls), 3)], classify_wall_ms=med(cls_wall),
                classify_classes_ms=med(clc), classify_classes_ms_min_max=[round(min(clc), 3), round(max(clc), 3)],
                classify_classes_wall_ms=med(clc_wall), classify_over_support=round(float(np.median(cls_wall)) / float(np.median(sup_wall)), 2),
                hits=int(node_hits.sum()), hits_equal_support=bool(int(node_hits.sum()) == got["hits"]), classified=int(direct[1:].sum()),
                classes_equal_direct=bool((np.bincount(classes, minlength=n + 1) == bufs[0]).all()), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--leaves", type=int, default=823)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["sampled", "contiguous"])
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    from strainscan_amd import _lib
    dev = torch.device("cuda", 0)
    for shape in ("sampled", "contiguous"):
        if args.only and args.only != shape:
            continue
        spec = bench.make_db(torch, dev, args.leaves, 1, shape=shape, hit_frac=0.05)
        reads = bench.make_reads(torch, dev, spec, args.reads, 2, 0.05)
        n = int(spec["n_nodes"])
        row_node = np.zeros(spec["keys"].size, np.uint32)
        off = spec["row_off"].astype(np.int64)
        row_node[spec["rows"]] = np.repeat(np.arange(1, n + 1, dtype=np.uint32), np.diff(off))
        parent = np.zeros(n + 1, np.uint32)
        parent[2:] = (np.arange(1, n) - 1) // 2 + 1
        db = _lib.KmerDB(spec["keys"], np.ones(spec["keys"].size, np.uint8), bench.K, True)
        for layout, order in (("packed", True), ("file_order", False)):
            rs = _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=order)
            if args.once:
                rs.classify(db, row_node, parent, 1)
            else:
                print(json.dumps(measure(torch, shape, layout, db, rs, row_node, parent, args.reps, args.reads)), flush=True)
            rs.close()
        db.close()
        del spec, reads
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
