#!/usr/bin/env python3
"""What `--pairs` costs on a BAM sample: ss_reads_load_pairs_bam of the BAM shape of scripts/bench_bam.py (--reads reads of 150
bases, unaligned, htslib-style members) written as --reads / 2 PAIRS -- flags 0x41 / 0x81, one name per pair, the mates of a pair
125 000 records apart (a piece of 250 000 records holds its first mates, then its second mates) -- whole and split into the steps
ss_bam_pairs_timing reports (the library's host clock around steps that each end with the stream synchronised), the median of
--reps calls after a warm-up.  Beside it, same process: ss_reads_load of the same file; ss_reads_load_pairs of the same reads as
two plain FASTQ files; and one ss_bam_extract_pairs call beside ss_bam_extract at the same N against a table of every 31-mer of
--cluster-reads reads.
    bench_pairs_bam.py [--reads N] [--cluster-reads N] [--reps R]
-> one JSON line (profiles/r25_pairs_bam.md)."""
import argparse
import json
import os
import shutil
import struct
import sys
import tempfile
import time
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench_bam  # noqa: E402
from bench_extract_bam import med, sample_kmers  # noqa: E402
from tests import bamio  # noqa: E402

L = bench_bam.L_READ
PER = 250000                     # records per piece, as bench_bam.make_sample: the reads of piece i are bench_bam._reads(1000 + i, n)


def say(what):
    print("[bench_pairs_bam] " + what, file=sys.stderr, flush=True)


def _paired_records(args):
    """piece `seed` as BAM records: record j < n / 2 is the first mate of the piece's pair j, record n / 2 + j its second mate"""
    seed, first, n = args
    codes, q = bench_bam._reads(seed, n)
    bam_code = np.array([1, 2, 8, 4], np.uint8)[codes]
    size = 4 + 32 + 11 + L // 2 + L
    rec = np.zeros((n, size), np.uint8)
    rec[:, :36] = np.frombuffer(struct.pack("<iiiBBHHHIiii", size - 4, -1, -1, 11, 255, 4680, 0, 0x4D, L, -1, -1, 0), np.uint8)
    rec[n // 2:, 18] = 0x8D                                              # (0x1 | 0x4 | 0x8 and 0x40 / 0x80: an unaligned pair)
    rec[:, 36:46] = np.concatenate([bench_bam._names(first // 2, n // 2)] * 2)
    rec[:, 47:47 + L // 2] = (bam_code[:, 0::2] << 4) | bam_code[:, 1::2]
    rec[:, 47 + L // 2:] = q
    return rec.tobytes()


def _fastq_mates(args):
    seed, first, n = args
    text = bench_bam._fastq_text(args)
    size = len(text) // n
    return text[:size * (n // 2)], text[size * (n // 2):]


def make_sample(d, n_reads, procs):
    pieces = [(1000 + i, i * PER, min(PER, n_reads - i * PER)) for i in range((n_reads + PER - 1) // PER)]
    assert all(n % 2 == 0 for _, _, n in pieces)
    with Pool(procs) as pool:
        recs = pool.map(_paired_records, pieces)
        bam = bamio.member(bamio.header(0), 6) + bench_bam._bgzf_records(recs, pool) + bamio.EOF
        del recs
        mates = pool.map(_fastq_mates, pieces)
    paths = dict(bam=os.path.join(d, "pairs.bam"), fq=[os.path.join(d, "R%d.fq" % (m + 1)) for m in range(2)])
    with open(paths["bam"], "wb") as f:
        f.write(bam)
    for m in range(2):
        with open(paths["fq"][m], "wb") as f:
            for t in mates:
                f.write(t[m])
    return paths


def timed(fn, reps):
    """median wall (ms) of reps calls after a warm-up; fn() -> something with .close(), or None"""
    ts = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        x = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if r:
            ts.append(dt)
        if x is not None:
            x.close()
    return med(ts), [round(min(ts), 1), round(max(ts), 1)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--cluster-reads", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    from strainscan_amd import _lib
    _lib.require_gpu()
    d = tempfile.mkdtemp(prefix="ss_bench_pbam_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = dict(reads=a.reads, pairs=a.reads // 2, read_len=L, reps=a.reps)
    try:
        t0 = time.perf_counter()
        p = make_sample(d, a.reads, a.procs)
        out["generate_s"] = round(time.perf_counter() - t0, 1)
        out["bam_mb"] = round(os.path.getsize(p["bam"]) / 1e6, 1)
        say("sample written (%.0f s)" % out["generate_s"])
        _lib.warm_up(gz=1)
        for order in (1, 0):
            steps = {k: [] for k in _lib.BAM_PAIRS_STEPS}

            def load():
                js = _lib.ReadSet.load_pairs_bam(p["bam"], order=bool(order))
                _lib.check(_lib.lib().ss_device_sync(), "sync")
                for k, v in _lib.bam_pairs_timing().items():
                    steps[k].append(v)
                out["counters"] = js.pair_counters
                out["joined_bytes"] = js.info()["n_bases"] + js.info()["n_records"]
                return js
            wall, span = timed(load, a.reps)
            out["load_pairs_bam_order%d" % order] = dict(wall_ms=wall, wall_ms_min_max=span, steps_ms={k: med(v[1:]) for k, v in steps.items()})
            say("load_pairs_bam order=%d: %s" % (order, json.dumps(out["load_pairs_bam_order%d" % order])))
        assert out["counters"]["pairs"] == a.reads // 2 and not out["counters"]["orphans"]
        out["load_ms"], _ = timed(lambda: _lib.ReadSet([p["bam"]]), a.reps)
        out["load_pairs_fastq_ms"], _ = timed(lambda: _lib.ReadSet.load_pairs(p["fq"][0], p["fq"][1]), min(a.reps, 3))
        say("load %s, load_pairs of the FASTQ pair %s" % (out["load_ms"], out["load_pairs_fastq_ms"]))
        db = _lib.KmerDB.from_text(sample_kmers(a.reads, 7, None, a.cluster_reads), 31, True)
        try:
            for name, pairs in (("extract", False), ("extract_pairs", True)):
                o = os.path.join(d, name + ".bam")
                c = {}
                steps = {k: [] for k in _lib.BAM_EXTRACT_STEPS}

                def call():
                    c.update(_lib.bam_extract(p["bam"], db, 16, o, pairs=pairs))
                    for k, v in _lib.bam_extract_timing().items():
                        steps[k].append(v)
                wall, span = timed(call, min(a.reps, 3))
                out[name] = dict(min_hits=16, counters=c, wall_ms=wall, wall_ms_min_max=span, steps_ms={k: med(v[1:]) for k, v in steps.items()})
                say("%s: %s" % (name, json.dumps(out[name])))
        finally:
            db.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
