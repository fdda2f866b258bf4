#!/usr/bin/env python3
"""What `-x N` costs: ReadSet.select beside ReadSet.support of the same (table, read set) pair in one process, at the two shapes
scripts/bench_read_support.py measures --
    tree     the sampled tree table (823 leaves, ~25 M rows, behind its Bloom filter) and 20 M reads of a three-strain mix
    cluster  a 10 M-row cluster table (every 31-mer of a 5 Mb genome, both orientations; ss_db_expect_hits) and 20 M reads of it
both against the binned (packed) resident set; device events around each call, the median of `--reps` after a warm-up (both calls
are synchronous, so their wall time is given too).  select - support of the same pair is what the record spans, the prefix sum and
the gather cost; a kernel-stats run of this script (scripts/gpu_kstats.sh) says how that splits.
With --files (cluster shape): the host half -- read back, digests, and ss_extract_write from the sample's FASTQ text (the reads
of the set, one file) and from a .fastq.gz pair (--gz-reads each), next to ss_reads_load of the same files.
    bench_extract_reads.py [--reads N] [--cluster-genome G] [--leaves C] [--reps R] [--only tree|cluster] [--min-hits-tree N]
                           [--min-hits-cluster N] [--no-select] [--files DIR] [--gz-reads N]
-> one JSON line per shape and step (profiles/r15_extract_reads.md).  --no-select: support alone (a library without
ss_reads_select, for the comparison with the commit before)."""
import argparse
import json
import os
import subprocess
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


def med(v):
    return round(float(np.median(v)), 3)


def measure(torch, name, db, rs, reps, n_reads, min_hits, select):
    got = {}
    sup_ms, sup_wall = events(torch, lambda: got.update(zip(("hist", "hits"), rs.support(db))), reps)
    out = dict(shape=name, rows=db.n_rows, reads=n_reads, packed_slabs=rs.packed_slabs(), reps=reps, hits=got["hits"],
               support_ms=med(sup_ms), support_ms_min_max=[round(min(sup_ms), 3), round(max(sup_ms), 3)], support_wall_ms=med(sup_wall))
    if select:
        def sel():
            sub = rs.select(db, min_hits)
            got["info"] = sub.info()
            sub.close()
        sel_ms, sel_wall = events(torch, sel, reps)
        want = int(got["hist"][min(min_hits, 64):].sum()) if min_hits <= 64 else None
        out.update(min_hits=min_hits, select_ms=med(sel_ms), select_ms_min_max=[round(min(sel_ms), 3), round(max(sel_ms), 3)],
                   select_wall_ms=med(sel_wall), select_minus_support_ms=round(med(sel_ms) - med(sup_ms), 3),
                   selected=got["info"]["n_records"], selected_bases=got["info"]["n_bases"],
                   selected_equals_support_ge=bool(want is None or want == got["info"]["n_records"]))
    return out


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, round((time.perf_counter() - t0) * 1e3, 1)


def measure_files(torch, _lib, bench, db, rs, reads, n_reads, min_hits, base, gz_reads):
    """the host half for the cluster shape: text of all the set's reads (one file), then a .fastq.gz pair of its first reads"""
    os.makedirs(base, exist_ok=True)
    sub, select_ms = timed(lambda: rs.select(db, min_hits))
    flat, read_back_ms = timed(sub.read_back)
    selected = sub.info()["n_records"]
    sub.close()
    keys, keys_ms = timed(lambda: _lib.flat_record_keys(flat))
    del flat
    print(json.dumps(dict(step="select + read back + digests", min_hits=min_hits, selected=selected, select_wall_ms=select_ms,
                          read_back_ms=read_back_ms, digests_ms=keys_ms, distinct_digests=int(np.unique(keys[:, 0]).size))), flush=True)
    text = os.path.join(base, "sample.fastq")
    bench.write_fastq(reads, n_reads, text)
    L1 = bench.READ_LEN + 1
    gz = []
    if gz_reads:
        for f in range(2):
            p = os.path.join(base, "pair_%d.fastq" % (f + 1))
            bench.write_fastq(reads[f * gz_reads * L1:(f + 1) * gz_reads * L1], gz_reads, p, noisy_quality_seed=77 + f)
            gz.append(p)
        procs = [subprocess.Popen(["gzip", "-6", "-f", p]) for p in gz]
        assert all(pr.wait() == 0 for pr in procs)
        gz = [p + ".gz" for p in gz]
        _lib.warm_up(gz=2)
    for what, ins in (("fastq text", [text]), (".fastq.gz pair", gz)):
        if not ins:
            continue
        outs = [os.path.join(base, "out_%d.fastq" % (i + 1)) for i in range(len(ins))]
        loads, writes = [], []
        c = None
        for _ in range(3):
            r2, ms = timed(lambda: _lib.ReadSet(ins))
            _lib.check(_lib.lib().ss_device_sync(), "sync")
            n_rec = r2.info()["n_records"]
            r2.close()
            loads.append(ms)
            c, ms = timed(lambda: _lib.extract_write(ins, keys, outs))
            writes.append(ms)
        print(json.dumps(dict(step="ss_extract_write", input=what, input_mb=round(sum(os.path.getsize(p) for p in ins) / 1e6, 1),
                              records=n_rec, counters=c, output_mb=round(sum(os.path.getsize(p) for p in outs) / 1e6, 1),
                              extract_write_ms=med(writes), extract_write_ms_all=writes, reads_load_ms=med(loads), reads_load_ms_all=loads,
                              host_cpus=int(_lib.lib().ss_host_cpus()))), flush=True)
        for p in outs:
            os.remove(p)
    for p in [text] + gz:
        os.remove(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--cluster-genome", type=int, default=5_000_000)
    ap.add_argument("--leaves", type=int, default=823)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["tree", "cluster"])
    ap.add_argument("--min-hits-tree", type=int, default=1)
    ap.add_argument("--min-hits-cluster", type=int, default=16)
    ap.add_argument("--no-select", action="store_true")
    ap.add_argument("--files", metavar="DIR")
    ap.add_argument("--gz-reads", type=int, default=1_000_000)
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
        print(json.dumps(measure(torch, "tree", db, rs, args.reps, args.reads, args.min_hits_tree, not args.no_select)), flush=True)
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
        print(json.dumps(measure(torch, "cluster", db, rs, args.reps, args.reads, args.min_hits_cluster, not args.no_select)), flush=True)
        if args.files and not args.no_select:
            measure_files(torch, _lib, bench, db, rs, reads, args.reads, args.min_hits_cluster, args.files, args.gz_reads)
        rs.close()
        db.close()


if __name__ == "__main__":
    main()
