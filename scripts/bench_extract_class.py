#!/usr/bin/env python3
"""What `--extract_class` costs on the device: one ss_reads_select_class call beside ss_reads_classify of the same (table, read set)
pair in one process, in the setting of bench_read_classes.py -- the sampled tree table of bench.py (823 leaves, 1645 nodes, ~25 M
rows), 20 M reads of a three-strain mix as the binned (packed) resident set and in file order, M = 1.  The clade lists:
    unclassified   [0]
    leaf           the leaf with the most reads of its own
    root           [1]: every classified read
    eight          the eight nodes of depth 3, whose clades split the classified reads between them
Device events around each synchronous call, the median of `--reps` after a warm-up, the wall time beside it; the sets of a call
are destroyed outside the timed region.
    bench_extract_class.py [--reads N] [--leaves C] [--reps R] [--tree DIR]
--tree: measure the library of another checkout of this project (one without ss_reads_select_class gives the classify numbers
alone: the baseline).  -> one JSON line per layout (profiles/r23_extract_class.md)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np


def measure(torch, _lib, layout, db, rs, row_node, parent, reps, n_reads):
    n = parent.size - 1
    bufs = [np.zeros(n + 1, np.uint64) for _ in range(3)]
    lib = _lib.lib()

    def classify():
        _lib.check(lib.ss_reads_classify(db.handle, rs._h, _lib.ptr(row_node), n, _lib.ptr(parent), 1, _lib.ptr(bufs[0]), _lib.ptr(bufs[1]),
                                         _lib.ptr(bufs[2]), None), "ss_reads_classify")

    def events(fn, after=None):
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
            if after:
                after()
        return dict(ms=round(float(np.median(ts[1:])), 3), ms_min_max=[round(min(ts[1:]), 3), round(max(ts[1:]), 3)],
                    wall_ms=round(float(np.median(walls[1:])), 3))

    out = dict(layout=layout, rows=db.n_rows, nodes=n, reads=n_reads, packed_slabs=rs.packed_slabs(), reps=reps, classify=events(classify))
    direct = bufs[0].copy()
    out.update(records=int(direct.sum()), classified=int(direct[1:].sum()))
    if not hasattr(lib, "ss_reads_select_class"):
        return out
    leaves = np.setdiff1d(np.arange(1, n + 1), parent[1:])
    leaf = int(leaves[np.argmax(direct[leaves])])
    lists = dict(unclassified=[0], leaf=[leaf], root=[1], eight=list(range(8, 16)))
    for name, clades in lists.items():
        cl = np.array(clades, np.uint32)
        hs = (C.c_void_p * cl.size)()
        got = {}

        def select(with_counts):
            _lib.check(lib.ss_reads_select_class(db.handle, rs._h, _lib.ptr(row_node), n, _lib.ptr(parent), 1, _lib.ptr(cl), cl.size, hs,
                                                 *([_lib.ptr(b) for b in bufs] if with_counts else [None] * 3)), "ss_reads_select_class")

        def destroy():
            rec = bases = 0
            for h in hs:
                a, b, c, d = (C.c_uint64() for _ in range(4))
                _lib.check(lib.ss_reads_info(C.c_void_p(h), C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "ss_reads_info")
                rec, bases = rec + a.value, bases + b.value
                _lib.check(lib.ss_reads_destroy(C.c_void_p(h)), "ss_reads_destroy")
            got.update(selected=rec, gathered_bytes=rec + bases)

        r = events(lambda: select(True), destroy)
        r.update(clades=clades, counts_equal_classify=bool((bufs[0] == direct).all()), **got)
        r["without_counts"] = events(lambda: select(False), destroy)
        out["select_" + name] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--leaves", type=int, default=823)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import bench
    from strainscan_amd import _lib
    dev = torch.device("cuda", 0)
    spec = bench.make_db(torch, dev, args.leaves, 1, shape="sampled", hit_frac=0.05)
    reads = bench.make_reads(torch, dev, spec, args.reads, 2, 0.05)
    n = int(spec["n_nodes"])
    row_node = np.zeros(spec["keys"].size, np.uint32)
    row_node[spec["rows"]] = np.repeat(np.arange(1, n + 1, dtype=np.uint32), np.diff(spec["row_off"].astype(np.int64)))
    parent = np.zeros(n + 1, np.uint32)
    parent[2:] = (np.arange(1, n) - 1) // 2 + 1
    db = _lib.KmerDB(spec["keys"], np.ones(spec["keys"].size, np.uint8), bench.K, True)
    for layout, order in (("packed", True), ("file_order", False)):
        rs = _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=order)
        print(json.dumps(dict(tree=os.path.abspath(args.tree), **measure(torch, _lib, layout, db, rs, row_node, parent, args.reps, args.reads))),
              flush=True)
        rs.close()
    db.close()


if __name__ == "__main__":
    main()
