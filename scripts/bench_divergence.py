#!/usr/bin/env python3
"""What `--divergence` costs on the device: one ss_reads_gaps call beside ss_reads_classify_strains (two called strains) and
ss_reads_support of the same (table, read set) pair in one process, at the cluster shape of bench_classify_strains.py --
    a 10 M-row cluster table (every 31-mer of a 5 Mb genome, both orientations; ss_db_expect_hits) and 20 M reads of 150 bases of
    it with 0.5 % substituted bases (bench.reads_of), as the binned (packed) resident set and in file order; row_called NULL
    (every row called), and with a fifth of the k-mers uncalled (both orientations of a k-mer alike)
Device events around each synchronous call, the median of `--reps` after a warm-up, the wall time beside it.  The calls upload
the row flags and fold the slots every time: that is part of what is measured.
    bench_divergence.py [--reads N] [--cluster-genome G] [--reps R] [--min-hits M]
-> one JSON line per layout (profiles/r31_divergence.md)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_classify_strains import events      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--cluster-genome", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-hits", type=int, default=4)
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
    rng = np.random.RandomState(1)
    called = np.repeat((rng.randint(0, 5, size=db.n_rows // 2 + 1) != 0).astype(np.uint8), 2)[:db.n_rows]
    masks = np.where(called != 0, 3, 1).astype(np.uint16)                       # two called strains; the uncalled k-mers are strain 1's alone
    m = args.min_hits
    for layout, order in (("packed", True), ("file_order", False)):
        rs = _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=order)
        out = dict(layout=layout, rows=db.n_rows, reads=args.reads, packed_slabs=rs.packed_slabs(), reps=args.reps, min_hits=m)
        got = {}
        out["support"] = events(torch, lambda: got.update(plain=rs.support(db)), args.reps)
        out["classify_strains"] = events(torch, lambda: rs.classify_strains(db, masks, 2, m, want_sets=False), args.reps)
        for name, rows in (("gaps_all_called", None), ("gaps_fifth_uncalled", called)):
            out[name] = events(torch, lambda: got.update(r=rs.gaps(db, rows, m)), args.reps)
            out[name]["totals"] = got["r"]
            out[name]["per_kb"] = round(1000.0 * got["r"]["sites"] / max(got["r"]["detectable"], 1), 3)
            out[name]["over_classify_strains"] = round(out[name]["ms"] / out["classify_strains"]["ms"], 2)
        out["gaps_with_records"] = events(torch, lambda: rs.gaps(db, None, m, want_records=True), args.reps)
        out["hits_all"] = got["plain"][1]
        print(json.dumps(out), flush=True)
        rs.close()
    db.close()


if __name__ == "__main__":
    main()
