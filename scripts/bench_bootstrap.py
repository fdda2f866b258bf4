#!/usr/bin/env python3
"""What a `--bootstrap` replicate costs on the device, at the cluster shape of scripts/bench_read_support.py: a 10 M-row cluster
table (every 31-mer of a 5 Mb genome, both orientations; ss_db_expect_hits) and N reads of it.

  resample   ReadSet.resample alone (record index, spans, digest + weight, prefix sum, gather) from the packed resident set and
             from the same reads in file order (ASCII); device events around the synchronous call, the median of --reps after a
             warm-up, and the wall time.  A kernel-stats run of this script (scripts/gpu_kstats.sh) says how the call splits.
  replicate  one replicate as read_reports.collect_bootstrap runs it: resample -> order (ReadSet.order: the resampled records binned in
             place) -> reset -> scan -> sync -> counts to the host -> destroy; and the same without the binning, the resampled set
             scanned as it is (one ASCII slab, the records in the source's order) -- the alternative that was not kept.  Then the
             parts: the scan of a resampled set as it is, the binning, the scan of the binned set, the counts to the host.
    bench_bootstrap.py [--reads N] [--cluster-genome G] [--reps R]
-> one JSON line per step (profiles/r21_bootstrap.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.bench_extract_reads import events, med  # noqa: E402


def spread(v):
    return [round(min(v), 3), round(max(v), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--cluster-genome", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=5)
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
    sets = {"packed": _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=True),
            "file_order": _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=False)}
    del reads
    rep = [0]
    for name, rs in sets.items():
        got = {}

        def one():
            rep[0] += 1
            sub = rs.resample(1, rep[0])
            got["info"] = sub.info()
            sub.close()
        ms, wall = events(torch, one, args.reps)
        print(json.dumps(dict(step="resample", source=name, reads=args.reads, packed_slabs=rs.packed_slabs(), reps=args.reps,
                              resample_ms=med(ms), resample_ms_min_max=spread(ms), resample_wall_ms=med(wall),
                              drawn=got["info"]["n_records"], drawn_bases=got["info"]["n_bases"])), flush=True)
    rs = sets["packed"]
    sets["file_order"].close()

    def replicate(order):
        rep[0] += 1
        sub = rs.resample(1, rep[0])
        try:
            db.reset()
            (sub.order() if order else sub).scan_into(db)
            _lib.check(_lib.lib().ss_device_sync(), "sync")
            return int(db.counts_rows().astype(np.uint64).sum())
        finally:
            sub.close()
    for order in (True, False, True, False):
        hits = {}
        ms, wall = events(torch, lambda: hits.update(n=replicate(order)), args.reps)
        print(json.dumps(dict(step="replicate", scan="binned first" if order else "as it is", reads=args.reads, reps=args.reps,
                              replicate_ms=med(ms), replicate_ms_min_max=spread(ms), replicate_wall_ms=med(wall), hits=hits["n"])), flush=True)
    # the parts
    sub = rs.resample(1, 1)

    def scan_only(s):
        db.reset()
        s.scan_into(db)
        _lib.check(_lib.lib().ss_device_sync(), "sync")
    ms_scan, _ = events(torch, lambda: scan_only(sub), args.reps)
    ms_counts, _ = events(torch, lambda: db.counts_rows(), args.reps)
    ms_bin, s2 = [], None
    for _ in range(args.reps + 1):                           # (a set is binned once: a fresh one each time, the first a warm-up)
        if s2 is not None:
            s2.close()
        s2 = rs.resample(1, 1)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        s2.order()
        b.record()
        torch.cuda.synchronize()
        ms_bin.append(a.elapsed_time(b))
    ms_bin = ms_bin[1:]
    ms_scan_b, _ = events(torch, lambda: scan_only(s2), args.reps)
    print(json.dumps(dict(step="replicate parts", reads=args.reads, drawn=sub.info()["n_records"], reps=args.reps,
                          scan_as_it_is_ms=med(ms_scan), scan_as_it_is_ms_min_max=spread(ms_scan), counts_to_host_ms=med(ms_counts),
                          binning_ms=med(ms_bin), binning_ms_min_max=spread(ms_bin), binned_packed_slabs=s2.packed_slabs(),
                          scan_binned_ms=med(ms_scan_b), scan_binned_ms_min_max=spread(ms_scan_b),
                          binning_plus_scan_minus_scan_as_it_is_ms=round(med(ms_bin) + med(ms_scan_b) - med(ms_scan), 3))), flush=True)
    t0 = time.perf_counter()
    s2.close()
    sub.close()
    rs.close()
    db.close()
    print(json.dumps(dict(step="teardown", wall_ms=round((time.perf_counter() - t0) * 1e3, 1))), flush=True)


if __name__ == "__main__":
    main()
