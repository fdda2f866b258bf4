#!/usr/bin/env python3
"""What `--read_calls` costs, in the setting of bench_read_classes.py: the sampled tree table of bench.py (823 leaves, 1645 nodes,
~25 M rows), N reads of 150 bases of a three-strain mix as one ASCII set in FILE ORDER, M = 1.
    classify  ss_reads_classify with rec_class, and one ss_reads_select_class call (the root's clade), on that set: calls that exist
              without the feature, so this part also runs on a build of the parent commit.
    calls     ss_reads_calls on the same set in the same process, with room for exactly n_list entries (a first call counts them);
              n_list and the bytes the call copies back.
    load      (--load_reads R, 0 = skip) ss_reads_load_ordered beside ss_reads_load of one file of R reads, as text and as
              .fastq.gz (gzip -6), wall time of one call each after one warm-up call.
    writer    ss_reads_load_ordered, ss_reads_calls and ss_read_calls_write of the text file of `load`: wall time of each, and the
              writer's time per record.
Device events around each synchronous call, the median of `--reps` after a warm-up, the wall time beside it.
    bench_read_calls.py [--reads N] [--leaves C] [--reps R] [--load_reads R] [--parts classify,calls,load,writer] [--tmp DIR]
-> one JSON line per part (profiles/r27_read_calls.md)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def events(torch, fn, reps, after=None):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--leaves", type=int, default=823)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--load_reads", type=int, default=4_000_000)
    ap.add_argument("--parts", default="classify,calls,load,writer")
    ap.add_argument("--tmp", default=None)
    args = ap.parse_args()
    parts = set(args.parts.split(","))
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from strainscan_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    spec = bench.make_db(torch, dev, args.leaves, 1, shape="sampled", hit_frac=0.05)
    reads = bench.make_reads(torch, dev, spec, args.reads, 2, 0.05)
    n = int(spec["n_nodes"])
    row_node = np.zeros(spec["keys"].size, np.uint32)
    row_node[spec["rows"]] = np.repeat(np.arange(1, n + 1, dtype=np.uint32), np.diff(spec["row_off"].astype(np.int64)))
    parent = np.zeros(n + 1, np.uint32)
    parent[2:] = (np.arange(1, n) - 1) // 2 + 1
    db = _lib.KmerDB(spec["keys"], np.ones(spec["keys"].size, np.uint8), bench.K, True)
    base = dict(reads=args.reads, rows=db.n_rows, nodes=n, reps=args.reps)
    rs = _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=False)
    bufs = [np.zeros(n + 1, np.uint64) for _ in range(3)]
    classes = np.zeros(args.reads + 1, np.uint32)

    if "classify" in parts:
        def classify():
            _lib.check(lib.ss_reads_classify(db.handle, rs._h, _lib.ptr(row_node), n, _lib.ptr(parent), 1, _lib.ptr(bufs[0]), _lib.ptr(bufs[1]),
                                             _lib.ptr(bufs[2]), _lib.ptr(classes)), "ss_reads_classify")

        clade, h = np.array([1], np.uint32), (C.c_void_p * 1)()

        def select_class():
            _lib.check(lib.ss_reads_select_class(db.handle, rs._h, _lib.ptr(row_node), n, _lib.ptr(parent), 1, _lib.ptr(clade), 1, h, None, None,
                                                 None), "ss_reads_select_class")

        out = dict(part="classify", classify_rec_class=events(torch, classify, args.reps), classified=int(bufs[0][1:].sum()),
                   select_class_root=events(torch, select_class, args.reps, lambda: lib.ss_reads_destroy(C.c_void_p(h[0]))), **base)
        print(json.dumps(out), flush=True)

    if "calls" in parts:
        scores, first = np.zeros(args.reads + 1, np.uint32), np.zeros(args.reads + 2, np.uint64)
        n_list = C.c_uint64()

        def calls(nodes, hits, cap):
            return lib.ss_reads_calls(db.handle, rs._h, _lib.ptr(row_node), n, _lib.ptr(parent), 1, _lib.ptr(classes), _lib.ptr(scores),
                                      _lib.ptr(first), _lib.ptr(nodes) if cap else None, _lib.ptr(hits) if cap else None, cap, C.byref(n_list),
                                      _lib.ptr(bufs[0]), _lib.ptr(bufs[1]), _lib.ptr(bufs[2]))

        rc = calls(None, None, 0)
        assert rc in (_lib.SS_OK, _lib.SS_ERANGE), rc
        cap = int(n_list.value)
        nodes, hits = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32)
        out = dict(part="calls", n_list=cap, calls=events(torch, lambda: _lib.check(calls(nodes, hits, cap), "ss_reads_calls"), args.reps),
                   count_only=events(torch, lambda: calls(None, None, 0), args.reps), classified=int(bufs[0][1:].sum()),
                   bytes_back=int(16 * args.reads + 8 + 8 * cap + 3 * 8 * (n + 1)), largest_list=int(np.diff(first[:args.reads + 1].astype(np.int64)).max()),
                   **base)
        print(json.dumps(out), flush=True)
    rs.close()

    if parts & {"load", "writer"} and args.load_reads:
        n_load = min(args.load_reads, args.reads)
        tmp = tempfile.mkdtemp(prefix="bench_read_calls_", dir=args.tmp)
        p = os.path.join(tmp, "r1.fastq")
        bench.write_fastq(reads[:n_load * (bench.READ_LEN + 1)], n_load, p, noisy_quality_seed=77)

        def wall(fn):
            fn().close()
            t0 = time.perf_counter()
            s = fn()
            dt = time.perf_counter() - t0
            info = s.info()
            s.close()
            return dict(s=round(dt, 4), records=info["n_records"])

        if "writer" in parts:
            t0 = time.perf_counter()
            s = _lib.ReadSet.load_ordered(p)
            t1 = time.perf_counter()
            got = s.calls(db, row_node, parent, 1)
            t2 = time.perf_counter()
            s.close()
            table = os.path.join(tmp, "read_calls_1.tsv")
            c = _lib.read_calls_write([p], [table], got, np.concatenate([[-1], np.arange(1, n + 1)]).astype(np.int64))
            t3 = time.perf_counter()
            out = dict(part="writer", reads=n_load, load_ordered_s=round(t1 - t0, 4), calls_s=round(t2 - t1, 4), write_s=round(t3 - t2, 4),
                       write_ns_per_record=round((t3 - t2) * 1e9 / max(c["read"], 1), 1), table_bytes=os.path.getsize(table), threads=os.environ.get("SS_HOST_THREADS", "min(16, CPUs)"),
                       n_list=int(got["list_node"].size), **{k: c[k] for k in ("read", "classified", "empty")})
            os.remove(table)
            print(json.dumps(out), flush=True)
        if "load" in parts:
            out = dict(part="load", reads=n_load, text_bytes=os.path.getsize(p))
            out["text"] = dict(load=wall(lambda: _lib.ReadSet([p])), load_ordered=wall(lambda: _lib.ReadSet.load_ordered(p)))
            if subprocess.call(["gzip", "-6", "-f", p]) == 0:
                p += ".gz"
                out["gz_bytes"] = os.path.getsize(p)
                out["gz"] = dict(load=wall(lambda: _lib.ReadSet([p])), load_ordered=wall(lambda: _lib.ReadSet.load_ordered(p)))
            print(json.dumps(out), flush=True)
        os.remove(p)
        os.rmdir(tmp)
    db.close()


if __name__ == "__main__":
    main()
