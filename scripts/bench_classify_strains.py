#!/usr/bin/env python3
"""What `--classify_strains` costs on the device: one ss_reads_classify_strains call at 1, 3, 8 and 16 called strains beside
ss_reads_support_labeled (the call it generalises) of the same (table, read set) pair in one process, at the cluster shape of
bench_by_strain.py --
    a 10 M-row cluster table (every 31-mer of a 5 Mb genome, both orientations; ss_db_expect_hits) and 20 M reads of it, as the
    binned (packed) resident set and in file order; a fifth of the rows have mask 0, every other row belongs to all called strains
    but those it drops with probability 0.05 each (close strains: most k-mers shared) -- and, for the labelled call, to the lowest
    strain of its mask alone
and one ss_reads_select_strains entry (the reads assigned to strain 1 alone; those compatible with it) beside one clade of
ss_reads_select_class over the same rows (a forest of n roots, the lowest strain of a row as its node).
Device events around each synchronous call, the median of `--reps` after a warm-up, the wall time beside it.  The calls upload
the row masks and make the slot masks every time: that is part of what is measured.
    bench_classify_strains.py [--reads N] [--cluster-genome G] [--reps R] [--strains 1,3,8,16] [--min-score M]
-> one JSON line per layout (profiles/r29_classify_strains.md)."""
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


def close_all(sets):
    n = 0
    for s in sets:
        n += s.info()["n_records"]
        s.close()
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--cluster-genome", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--strains", default="1,3,8,16")
    ap.add_argument("--min-score", type=int, default=1)
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
    m = args.min_score
    for layout, order in (("packed", True), ("file_order", False)):
        rs = _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=order)
        out = dict(layout=layout, rows=db.n_rows, reads=args.reads, packed_slabs=rs.packed_slabs(), reps=args.reps, min_score=m)
        got = {}
        out["support"] = events(torch, lambda: got.update(plain=rs.support(db)), args.reps)
        rng = np.random.RandomState(1)
        for n in [int(x) for x in args.strains.split(",")]:
            # both orientations of a k-mer (rows 2i, 2i + 1) share their mask
            half = db.n_rows // 2
            drop = np.zeros(half, np.uint16)
            for j in range(n):
                drop |= (rng.random_sample(half) < 0.05).astype(np.uint16) << np.uint16(j)
            masks = np.where(rng.randint(0, 5, size=half) == 0, 0, ((1 << n) - 1) & ~drop).astype(np.uint16)
            masks = np.repeat(masks, 2)[:db.n_rows]
            low = (masks & (~masks + np.uint16(1))).astype(np.int64)
            lab = np.where(low > 0, np.log2(np.maximum(low, 1)).astype(np.int64) + 1, 0)
            r = dict(classify_strains=events(torch, lambda: got.update(cs=rs.classify_strains(db, masks, n, m)), args.reps))
            cs = got["cs"]
            r.update(records=int(cs["unique"].sum() + cs["tied"][0]), unique=int(cs["unique"][1:].sum()), tied=int(cs["tied"][0]),
                     unassigned=int(cs["unique"][0]), distinct_sets=int((cs["set_reads"] > 0).sum()), hits=int(cs["strain_hits"].sum()),
                     hits_all=got["plain"][1])
            r["classify_strains_without_set_reads"] = events(torch, lambda: rs.classify_strains(db, masks, n, m, want_sets=False), args.reps)
            if n <= _lib.LABELS_MAX:
                r["support_labeled"] = events(torch, lambda: got.update(lab=rs.support_labeled(db, lab.astype(np.uint8), n)), args.reps)
                r["over_support_labeled"] = round(r["classify_strains"]["ms"] / r["support_labeled"]["ms"], 2)
            par = np.zeros(n + 1, np.uint32)
            r["classify"] = events(torch, lambda: rs.classify(db, lab.astype(np.uint32), par, m), args.reps)
            for name, how in (("unique", 0), ("compatible", 1)):
                r["select_strains_" + name] = events(torch, lambda: got.update(n=close_all(rs.select_strains(db, masks, n, m, [1], [how]))), args.reps)
                r["select_strains_" + name]["selected"] = got["n"]
            r["select_class_one_clade"] = events(torch, lambda: got.update(n=close_all(rs.select_class(db, lab.astype(np.uint32), par, m, [1]))),
                                                 args.reps)
            r["select_class_one_clade"]["selected"] = got["n"]
            out["strains_%d" % n] = r
        print(json.dumps(out), flush=True)
        rs.close()
    db.close()


if __name__ == "__main__":
    main()
