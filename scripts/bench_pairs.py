#!/usr/bin/env python3
"""What `--pairs` costs on the device, in the setting of bench_read_classes.py: the sampled tree table of bench.py (823 leaves,
1645 nodes, ~25 M rows) and N reads of 150 bases of a three-strain mix, the first half of them mate 1 and the second half mate 2.
    join      ss_reads_join_pairs_dev of the two flat blocks in line order (line index + join kernel: a copy of n1 + n2 bytes), and
              with the binning behind it (order = 1).  Beside it ss_reads_select with min_hits = 1 and ss_reads_support of the plain
              set in file order: the two share their first pass, so select - support is the span pass, the prefix sum and
              gather_records moving `selected_bytes`.
    calls     ss_reads_support, ss_reads_classify (M = 1) and one bootstrap replicate (resample, order, scan) on the joined packed
              set and on the plain packed set of the same reads.
    load      (--load_reads R, 0 = skip) ss_reads_load_pairs beside ss_reads_load of the same two files, as text and as .fastq.gz
              (gzip -6), R reads in all, wall time of one call each after one warm-up call.
Device events around each synchronous call, the median of `--reps` after a warm-up, the wall time beside it; sets are destroyed
outside the timed region.
    bench_pairs.py [--reads N] [--leaves C] [--reps R] [--load_reads R] [--tmp DIR]
-> one JSON line per part (profiles/r24_pairs.md)."""
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
    ap.add_argument("--tmp", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from strainscan_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    spec = bench.make_db(torch, dev, args.leaves, 1, shape="sampled", hit_frac=0.05)
    n_reads = args.reads // 2 * 2
    reads = bench.make_reads(torch, dev, spec, n_reads, 2, 0.05)
    half = n_reads // 2 * (bench.READ_LEN + 1)
    b1, b2 = reads[:half], reads[half:]
    n = int(spec["n_nodes"])
    row_node = np.zeros(spec["keys"].size, np.uint32)
    row_node[spec["rows"]] = np.repeat(np.arange(1, n + 1, dtype=np.uint32), np.diff(spec["row_off"].astype(np.int64)))
    parent = np.zeros(n + 1, np.uint32)
    parent[2:] = (np.arange(1, n) - 1) // 2 + 1
    db = _lib.KmerDB(spec["keys"], np.ones(spec["keys"].size, np.uint8), bench.K, True)
    base = dict(reads=n_reads, pairs=n_reads // 2, rows=db.n_rows, reps=args.reps)

    # ---- the join alone
    h = C.c_void_p()

    def join(order):
        _lib.check(lib.ss_reads_join_pairs_dev(b1.data_ptr(), b1.numel(), b2.data_ptr(), b2.numel(), order, C.byref(h)), "ss_reads_join_pairs_dev")

    def destroy():
        _lib.check(lib.ss_reads_destroy(h), "ss_reads_destroy")

    out = dict(part="join", joined_bytes=int(b1.numel() + b2.numel()), line_order=events(torch, lambda: join(0), args.reps, destroy),
               ordered=events(torch, lambda: join(1), args.reps, destroy), **base)
    plain_file = _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=False)
    got = {}

    def select():
        _lib.check(lib.ss_reads_select(db.handle, plain_file._h, 1, C.byref(h)), "ss_reads_select")

    def destroy_selected():
        a, b = C.c_uint64(), C.c_uint64()
        _lib.check(lib.ss_reads_info(h, C.byref(a), C.byref(b), None, None), "ss_reads_info")
        got.update(selected=a.value, selected_bytes=a.value + b.value)
        destroy()

    out["select_min_hits_1"] = events(torch, select, args.reps, destroy_selected)
    out["support_file_order"] = events(torch, lambda: plain_file.support(db), args.reps)
    out.update(got)
    plain_file.close()
    print(json.dumps(out), flush=True)

    # ---- the per-record calls on fragments and on mates
    bufs = [np.zeros(n + 1, np.uint64) for _ in range(3)]
    sets = dict(mates=_lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=True),
                fragments=_lib.ReadSet.join_pairs_dev(b1.data_ptr(), b1.numel(), b2.data_ptr(), b2.numel(), order=True))
    out = dict(part="calls", **base)
    for name, rs in sets.items():
        def classify():
            _lib.check(lib.ss_reads_classify(db.handle, rs._h, _lib.ptr(row_node), n, _lib.ptr(parent), 1, _lib.ptr(bufs[0]), _lib.ptr(bufs[1]),
                                             _lib.ptr(bufs[2]), None), "ss_reads_classify")

        def replicate():
            with_hits = rs.resample(1, 0)
            db.reset()
            with_hits.order().scan_into(db)
            _lib.check(lib.ss_device_sync(), "ss_device_sync")
            with_hits.close()

        r = dict(packed_slabs=rs.packed_slabs(), records=rs.info()["n_records"], device_bytes=rs.info()["device_bytes"])
        r["support"] = events(torch, lambda: rs.support(db), args.reps)
        r["hits"] = rs.support(db)[1]
        r["classify"] = events(torch, classify, args.reps)
        r["classified"] = int(bufs[0][1:].sum())
        r["bootstrap_replicate"] = events(torch, replicate, args.reps)
        out[name] = r
    for rs in sets.values():
        rs.close()
    print(json.dumps(out), flush=True)

    # ---- the load
    if args.load_reads:
        n_pair = min(args.load_reads, n_reads) // 2
        tmp = tempfile.mkdtemp(prefix="bench_pairs_", dir=args.tmp)
        paths = []
        for f in range(2):
            p = os.path.join(tmp, "r%d.fastq" % (f + 1))
            bench.write_fastq((b1, b2)[f][:n_pair * (bench.READ_LEN + 1)], n_pair, p, noisy_quality_seed=77 + f)
            paths.append(p)

        def wall(fn):
            fn().close()
            t0 = time.perf_counter()
            rs = fn()
            dt = time.perf_counter() - t0
            info = rs.info()
            rs.close()
            return dict(s=round(dt, 4), records=info["n_records"])

        out = dict(part="load", reads=2 * n_pair, text_bytes=sum(os.path.getsize(p) for p in paths))
        out["text"] = dict(load=wall(lambda: _lib.ReadSet(paths)), load_pairs=wall(lambda: _lib.ReadSet.load_pairs(paths[0], paths[1])))
        procs = [subprocess.Popen(["gzip", "-6", "-f", p]) for p in paths]
        if all(pr.wait() == 0 for pr in procs):
            gz = [p + ".gz" for p in paths]
            out["gz_bytes"] = sum(os.path.getsize(p) for p in gz)
            out["gz"] = dict(load=wall(lambda: _lib.ReadSet(gz)), load_pairs=wall(lambda: _lib.ReadSet.load_pairs(gz[0], gz[1])))
            paths = gz
        for p in paths:
            os.remove(p)
        os.rmdir(tmp)
        print(json.dumps(out), flush=True)
    db.close()


if __name__ == "__main__":
    main()
