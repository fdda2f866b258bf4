#!/usr/bin/env python3
"""The calls that write a slab of back-to-back records (the piece copy, strainscan_amd/csrc/ss_piece_copy.h), timed for ONE build of
the library so that two builds can be run alternately in fresh processes and compared (profiles/r26_piece_copy.md):
    bench_piece_copy.py sample DIR                    # CPU only: the 4 M-read paired BAM of bench_pairs_bam.py and a table of its reads
    SS_LIB=<library> bench_piece_copy.py run TAG DIR OUT [--reads N] [--reps R] [--digest]
    bench_piece_copy.py report OUT                    # TAGs beginning with "parent" against those beginning with "branch"
run: ss_reads_select and ss_reads_resample of N reads of 150 bases (a packed set and the same reads in file order, ASCII; the table
is every 31-mer of a 5 Mb genome, min_hits 1: everything is selected), ss_reads_join_pairs_dev of the two halves of the block,
ss_reads_load_pairs_bam and ss_bam_extract (min_hits 16) of the BAM -- a warm-up and R repeats each, the host clock around a call
that ends with the device synchronised; --digest: the sha1 of each result (the set read back; the written BAM).  -> OUT/TAG.json
report: per call the medians, the parent's spread (largest - smallest repeat) and whether the branch's median exceeds the parent's
by more than that; whether the digests agree.  Exit status 1 when a call is outside the margin or a digest differs."""
import glob
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def sample(d, n=4_000_000):
    import bench_pairs_bam as bpb
    from bench_extract_bam import sample_kmers
    os.makedirs(d, exist_ok=True)
    p = bpb.make_sample(d, n, min(16, os.cpu_count() or 1))
    for f in p["fq"]:
        os.remove(f)
    with open(os.path.join(d, "kmers.fa"), "wb") as f:
        f.write(sample_kmers(n, 7, None, 10000))
    print("sample: bam %.1f MB" % (os.path.getsize(p["bam"]) / 1e6), flush=True)


def run(tag, d, out_dir, n_reads, reps, digest):
    import torch
    import bench
    from strainscan_amd import _lib
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    out = dict(tag=tag, lib=_lib.LIB_PATH, reads=n_reads, reps=reps, calls={})

    def sync():
        _lib.check(_lib.lib().ss_device_sync(), "sync")

    def timed(name, fn, result=None, steps=None):
        """fn() -> a set (closed outside the clock) or None; result(x) -> the bytes to digest (default: the set read back)"""
        ts, st, dg, info = [], [], None, None
        for r in range(reps + 1):
            sync()
            t0 = time.perf_counter()
            x = fn()
            sync()
            dt = (time.perf_counter() - t0) * 1e3
            if r:
                ts.append(round(dt, 3))
                if steps:
                    st.append(steps())
            if r == reps:
                info = x.info() if x is not None else None
                if digest:
                    dg = hashlib.sha1(result(x) if result else x.read_back()).hexdigest()
            if x is not None:
                x.close()
        out["calls"][name] = dict(ms=ts, digest=dg, info=info, steps=st or None)
        print(tag, name, ts, dg, info, flush=True)

    G = 5_000_000
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    genome = torch.randint(0, 4, (G + 200,), generator=g, device=dev, dtype=torch.uint8)
    key, rc, _, _ = bench._kmer_keys(torch, genome, torch.arange(0, G, device=dev), dev)
    keys = torch.stack([key, rc], 1).reshape(-1).cpu().numpy().view(np.uint64)
    reads = bench.reads_of(torch, dev, [genome], [n_reads], g)
    db = _lib.KmerDB(keys, np.ones(keys.size, np.uint8), bench.K, True).expect_hits()
    packed = _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=True)
    ascii_ = _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=False)
    sync()
    out["packed_slabs"] = [packed.packed_slabs(), ascii_.packed_slabs()]
    timed("select_ascii", lambda: ascii_.select(db, 1))
    timed("select_packed", lambda: packed.select(db, 1))
    timed("resample_ascii", lambda: ascii_.resample(1, 1))
    timed("resample_packed", lambda: packed.resample(1, 1))
    for x in (packed, ascii_, db):
        x.close()
    half = (n_reads // 2) * (bench.READ_LEN + 1)
    timed("join_pairs_dev", lambda: _lib.ReadSet.join_pairs_dev(reads.data_ptr(), half, reads.data_ptr() + half, half, order=False))
    del reads
    torch.cuda.empty_cache()
    bam = os.path.join(d, "pairs.bam")
    _lib.warm_up(gz=1)
    timed("load_pairs_bam", lambda: _lib.ReadSet.load_pairs_bam(bam, order=False), steps=_lib.bam_pairs_timing)
    db = _lib.KmerDB.from_text(open(os.path.join(d, "kmers.fa"), "rb").read(), 31, True)
    o = os.path.join(d, "extract_%s.bam" % tag)
    cnt = {}
    timed("bam_extract", lambda: cnt.update(_lib.bam_extract(bam, db, 16, o)), result=lambda x: open(o, "rb").read(), steps=_lib.bam_extract_timing)
    out["calls"]["bam_extract"]["info"] = {k: int(v) for k, v in cnt.items()}
    os.remove(o)
    db.close()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, tag + ".json"), "w") as f:
        json.dump(out, f)


def report(out_dir):
    runs = [json.load(open(f)) for f in sorted(glob.glob(os.path.join(out_dir, "*.json")))]
    par = [r for r in runs if r["tag"].startswith("parent")]
    br = [r for r in runs if r["tag"].startswith("branch")]
    bad = 0
    print("| call | parent: median (min – max) ms | parent's spread | branch: median (min – max) ms | branch against parent + spread | digests |")
    print("|---|---|---|---|---|---|")
    for name in par[0]["calls"]:
        p = [t for r in par for t in r["calls"][name]["ms"]]
        b = [t for r in br for t in r["calls"][name]["ms"]]
        dig = {r["calls"][name]["digest"] for r in runs if r["calls"][name]["digest"]}
        spread = max(p) - min(p)
        ok, same = np.median(b) <= np.median(p) + spread, len(dig) == 1
        bad += (not ok) + (not same)
        print("| `%s` | %.3f (%.3f – %.3f) | %.3f | %.3f (%.3f – %.3f) | %s | %s |" % (name, np.median(p), min(p), max(p), spread, np.median(b), min(b),
              max(b), "within" if ok else "OUTSIDE", "equal" if same else "DIFFERENT"))
    for name in par[0]["calls"]:
        print("%s, median ms per process: %s" % (name, json.dumps({r["tag"]: round(float(np.median(r["calls"][name]["ms"])), 3) for r in runs})))
        for r in runs:
            st = r["calls"][name].get("steps")
            if st:
                print("%s, %s, steps (median ms): %s" % (name, r["tag"], json.dumps({k: round(float(np.median([s[k] for s in st])), 2) for k in st[0]})))
    print("results:", json.dumps({n: c["info"] for n, c in br[0]["calls"].items()}))
    return 1 if bad else 0


if __name__ == "__main__":
    a = sys.argv[1:]
    if a[:1] == ["sample"]:
        sample(a[1])
    elif a[:1] == ["run"]:
        opt = a[4:]
        run(a[1], a[2], a[3], int(opt[opt.index("--reads") + 1]) if "--reads" in opt else 20_000_000,
            int(opt[opt.index("--reps") + 1]) if "--reps" in opt else 5, "--digest" in opt)
    elif a[:1] == ["report"]:
        sys.exit(report(a[1]))
    else:
        sys.exit(__doc__)
