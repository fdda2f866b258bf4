#!/usr/bin/env python3
"""What `--em_strains` costs on the device, at the cluster shape of bench_classify_strains.py (a 10 M-row cluster table, every 31-mer
of a 5 Mb genome in both orientations, and 20 M reads of 150 bases of it; a fifth of the rows have mask 0, every other row belongs
to all called strains but those it drops with probability 0.05 each):
  sets  one ss_reads_strain_sets_resampled call of 16 replicates at 3, 8 and 16 called strains, beside one ss_reads_classify_strains
        call of the same pair in the same process and beside sixteen times ss_reads_resample + ss_reads_classify_strains (the
        route that materialises every replicate), whose set counts are compared with the call's
  classify  ss_reads_classify_strains alone (runs on a build without the feature too: the parent commit's figure)
  em    ss_em_strain_sets at 1001 vectors x 100, 4000 and 60000 sets x 16 strains x 1000 iterations (tol = 0), the copies of the
        counts to the device and of the result back included
Device events around each synchronous call, the median of `--reps` after a warm-up, the wall time beside it.
    bench_em_strains.py [--parts sets,classify,em] [--reads N] [--cluster-genome G] [--reps R] [--strains 3,8,16] [--em-sets 100,4000,60000]
-> one JSON line per part (profiles/r30_em_strains.md)."""
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
    ts, walls = ts[1:], walls[1:]
    return dict(ms=round(float(np.median(ts)), 3), ms_min_max=[round(min(ts), 3), round(max(ts), 3)], wall_ms=round(float(np.median(walls)), 3))


def row_masks(db, n, rng):
    """both orientations of a k-mer (rows 2i, 2i + 1) share their mask"""
    half = db.n_rows // 2
    drop = np.zeros(half, np.uint16)
    for j in range(n):
        drop |= (rng.random_sample(half) < 0.05).astype(np.uint16) << np.uint16(j)
    masks = np.where(rng.randint(0, 5, size=half) == 0, 0, ((1 << n) - 1) & ~drop).astype(np.uint16)
    return np.repeat(masks, 2)[:db.n_rows]


def materialised(rs, db, masks, n, m, seed, n_rep):
    out = []
    for j in range(n_rep):
        sub = rs.resample(seed, j)
        try:
            out.append(sub.classify_strains(db, masks, n, m)["set_reads"])
        finally:
            sub.close()
    return np.stack(out)


def em_input(rng, n_vec, n_sets, n_strains):
    """distinct non-zero masks, the singletons first; counts of a sample and its replicates: one vector, Poisson noise around it"""
    space = (1 << n_strains) - 1
    masks = np.concatenate([1 << np.arange(n_strains), rng.permutation(space)[:n_sets] + 1])
    _, first = np.unique(masks, return_index=True)
    masks = masks[np.sort(first)][:n_sets].astype(np.uint16)
    base = rng.gamma(0.5, 400.0, size=masks.size)
    return rng.poisson(base[None, :], size=(n_vec, masks.size)).astype(np.uint64), masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="sets,em")
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--cluster-genome", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--strains", default="3,8,16")
    ap.add_argument("--em-sets", default="100,4000,60000")
    ap.add_argument("--min-score", type=int, default=1)
    args = ap.parse_args()
    parts = args.parts.split(",")
    import torch
    import bench
    from strainscan_amd import _lib
    dev = torch.device("cuda", 0)
    if "sets" in parts or "classify" in parts:
        G = args.cluster_genome
        g = torch.Generator(device=dev)
        g.manual_seed(3)
        genome = torch.randint(0, 4, (G + 200,), generator=g, device=dev, dtype=torch.uint8)
        key, rc, _, _ = bench._kmer_keys(torch, genome, torch.arange(0, G, device=dev), dev)
        keys = torch.stack([key, rc], 1).reshape(-1).cpu().numpy().view(np.uint64)
        reads = bench.reads_of(torch, dev, [genome], [args.reads], g)
        db = _lib.KmerDB(keys, np.ones(keys.size, np.uint8), bench.K, True).expect_hits()
        m = args.min_score
        rs = _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=True)
        out = dict(part="sets" if "sets" in parts else "classify", rows=db.n_rows, reads=args.reads, packed_slabs=rs.packed_slabs(), reps=args.reps,
                   min_score=m)
        rng = np.random.RandomState(1)
        got = {}
        for n in [int(x) for x in args.strains.split(",")]:
            masks = row_masks(db, n, rng)
            r = dict(classify_strains=events(torch, lambda: got.update(cs=rs.classify_strains(db, masks, n, m)), args.reps))
            r["distinct_sets"] = int((got["cs"]["set_reads"] > 0).sum())
            if "sets" in parts:
                r["sets_resampled_16"] = events(torch, lambda: got.update(rep=rs.strain_sets_resampled(db, masks, n, m, 1, 0, 16)), args.reps)
                r["sets_resampled_1"] = events(torch, lambda: rs.strain_sets_resampled(db, masks, n, m, 1, 0, 1), args.reps)
                r["sixteen_times_resample_and_classify"] = events(torch, lambda: got.update(mat=materialised(rs, db, masks, n, m, 1, 16)), 1)
                r["equal"] = bool((got["rep"] == got["mat"]).all())
                r["over_classify_strains"] = round(r["sets_resampled_16"]["ms"] / r["classify_strains"]["ms"], 2)
                r["weights_added"] = int(got["rep"].sum())
            out["strains_%d" % n] = r
        print(json.dumps(out), flush=True)
        rs.close()
        db.close()
    if "em" in parts:
        rng = np.random.RandomState(2)
        out = dict(part="em", vectors=1001, strains=16, max_iter=1000, tol=0.0, reps=args.reps)
        for n_sets in [int(x) for x in args.em_sets.split(",")]:
            counts, masks = em_input(rng, 1001, n_sets, 16)
            got = {}
            r = events(torch, lambda: got.update(res=_lib.em_strain_sets(counts, masks, 16, 1000, 0.0)), args.reps)
            r["one_iteration"] = events(torch, lambda: _lib.em_strain_sets(counts, masks, 16, 1, 0.0), args.reps)
            rho, iters = got["res"]
            r.update(sets=int(masks.size), in_lds=bool(masks.size <= _lib.EM_LDS_SETS), iters=[int(iters.min()), int(iters.max())],
                     rho_sums=[float(rho.sum(axis=1).min()), float(rho.sum(axis=1).max())])
            r["us_per_vector_iteration"] = round((r["ms"] - r["one_iteration"]["ms"]) * 1e3 / (1001 * 999), 4)
            out["sets_%d" % n_sets] = r
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
