#!/usr/bin/env python3
"""BAM input against the same reads as a bgzip-style FASTQ: ss_reads_load of each (alternating, median of --reps) on the device
path, the BAM on the host path (SS_GZ_GPU=0) beside them, and a fresh `strainscan -i` process on each.  One JSON line.

The sample (not timed): --reads random reads of --read-len bases (150) with Phred-like qualities, written by several processes as an unaligned BAM
(htslib-style BGZF members, zlib level 6) and as a FASTQ .gz of 0xff00-byte members (bgzip's layout).  Kernel times: run it
again under `rocprofv3 --kernel-trace --stats -- python scripts/bench_bam.py --no-cli --reps 1` (kernels `bam_walk_kernel`,
`bam_list_kernel`, `bam_keep_kernel`, `bam_len_kernel`, `bam_decode_kernel` beside the inflater's)."""
import argparse
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import bamio  # noqa: E402

L_READ = 150


def _reads(seed, n):
    """n reads of L_READ bases (codes 0..3 = ACGT) and qualities (Phred, not +33)."""
    rs = np.random.RandomState(seed)
    codes = rs.randint(0, 4, size=(n, L_READ)).astype(np.uint8)
    q = 38 - np.abs(rs.normal(0, 4, size=(n, L_READ))).astype(np.int64) - (np.arange(L_READ) // 30)
    return codes, np.clip(q, 2, 40).astype(np.uint8)


def _names(first, n):
    return np.frombuffer("".join("r%09d" % i for i in range(first, first + n)).encode(), np.uint8).reshape(n, 10)


def _bam_records(args):
    """Piece `seed` of the sample as BAM records (unaligned: flag 4, refID -1), built as one array."""
    seed, first, n = args
    codes, q = _reads(seed, n)
    bam_code = np.array([1, 2, 8, 4], np.uint8)[codes]                  # codes 0..3 = A C T G (as _fastq_text) -> BAM's 4-bit codes
    size = 4 + 32 + 11 + L_READ // 2 + L_READ
    rec = np.zeros((n, size), np.uint8)
    fixed = struct.pack("<iiiBBHHHIiii", size - 4, -1, -1, 11, 255, 4680, 0, 4, L_READ, -1, -1, 0)
    rec[:, :36] = np.frombuffer(fixed, np.uint8)
    rec[:, 36:46] = _names(first, n)
    o = 47
    rec[:, o:o + L_READ // 2] = (bam_code[:, 0::2] << 4) | bam_code[:, 1::2]
    rec[:, o + L_READ // 2:] = q
    return rec.tobytes()


def _fastq_text(args):
    seed, first, n = args
    codes, q = _reads(seed, n)
    lut = np.frombuffer(b"ACTG", np.uint8)                              # the same letters as _bam_records' codes
    size = 12 + L_READ + 3 + L_READ + 1
    rec = np.empty((n, size), np.uint8)
    rec[:, 0] = ord("@")
    rec[:, 1:11] = _names(first, n)
    rec[:, 11] = 10
    rec[:, 12:12 + L_READ] = lut[codes]
    rec[:, 12 + L_READ:15 + L_READ] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 15 + L_READ:15 + 2 * L_READ] = q + 33
    rec[:, -1] = 10
    return rec.tobytes()


def _members(data):
    return b"".join(bamio.member(data[o:o + bamio.BLOCK], 6) for o in range(0, len(data), bamio.BLOCK))


def _bgzf_records(records, pool):
    """htslib's cut: a record starts a new member when it does not fit (the records here are of one size)."""
    rec = len(records[0]) if records else 1
    per = max(1, bamio.BLOCK // rec) * rec
    chunks = [blob[o:o + per] for blob in records for o in range(0, len(blob), per)]
    return b"".join(pool.map(_members, chunks, chunksize=64))


def make_sample(d, n_reads, procs):
    per = max(1, 250000 * 150 // L_READ)                                  # reads per piece: ~37 M bases
    pieces = [(1000 + i, i * per, min(per, n_reads - i * per)) for i in range((n_reads + per - 1) // per)]
    with Pool(procs) as pool:
        recs = pool.map(_bam_records, pieces)
        bam = bamio.member(bamio.header(0), 6) + _bgzf_records(recs, pool) + bamio.EOF
        del recs
        text = b"".join(pool.map(_fastq_text, pieces))
        blocks = [text[o:o + 64 * bamio.BLOCK] for o in range(0, len(text), 64 * bamio.BLOCK)]
        fq = b"".join(pool.map(_members, blocks)) + bamio.EOF
    paths = dict(bam=os.path.join(d, "sample.bam"), fq_gz=os.path.join(d, "sample.fq.gz"))
    with open(paths["bam"], "wb") as f:
        f.write(bam)
    with open(paths["fq_gz"], "wb") as f:
        f.write(fq)
    return paths


def load_ms(_lib, path, gz_gpu="1"):
    os.environ["SS_GZ_GPU"] = gz_gpu
    t0 = time.perf_counter()
    rs = _lib.ReadSet([path])
    _lib.check(_lib.lib().ss_device_sync(), "sync")
    dt = time.perf_counter() - t0
    info = rs.info()
    rs.close()
    return dt * 1e3, info


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--read-len", type=int, default=150, help="bases per read (even); e.g. --reads 40000 --read-len 20000 for long reads")
    ap.add_argument("--no-cli", action="store_true", help="no fresh strainscan processes")
    a = ap.parse_args()
    global L_READ
    if a.read_len < 2 or a.read_len % 2:
        ap.error("--read-len must be even")
    L_READ = a.read_len                                                  # (the pool's workers are forked after this)
    from strainscan_amd import _lib
    _lib.require_gpu()
    d = tempfile.mkdtemp(prefix="ss_bench_bam_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = dict(reads=a.reads, read_len=L_READ)
    try:
        t0 = time.perf_counter()
        p = make_sample(d, a.reads, a.procs)
        out["generate_s"] = round(time.perf_counter() - t0, 1)
        out["bam_mb"] = round(os.path.getsize(p["bam"]) / 1e6, 1)
        out["fq_gz_mb"] = round(os.path.getsize(p["fq_gz"]) / 1e6, 1)
        _lib.warm_up(gz=1)
        c0 = _lib.bam_counters()
        for key in ("bam", "fq_gz"):                    # one untimed load each: the device scratch, the pinned upload buffers
            load_ms(_lib, p[key])
        times = {"bam": [], "fq_gz": [], "bam_host": []}
        out["blocks"] = {}
        for _ in range(a.reps):
            for key in ("bam", "fq_gz"):
                ms, info = load_ms(_lib, p[key])
                assert info["n_records"] == a.reads and info["n_bases"] == a.reads * (L_READ + 1), (key, info)
                out["blocks"][key] = info["n_blocks"]
                times[key].append(round(ms, 1))
        for _ in range(a.reps):
            ms, info = load_ms(_lib, p["bam"], gz_gpu="0")
            assert info["n_records"] == a.reads and info["n_bases"] == a.reads * (L_READ + 1)
            times["bam_host"].append(round(ms, 1))
        os.environ.pop("SS_GZ_GPU", None)
        c1 = _lib.bam_counters()
        out["bam_counters"] = {k: c1[k] - c0[k] for k in c1}
        out["load_ms"] = {k: dict(median=round(float(np.median(v)), 1), all=v) for k, v in times.items()}
        out["bam_over_fq_gz"] = round(out["load_ms"]["bam"]["median"] / out["load_ms"]["fq_gz"]["median"], 3)
        # the same reads from both files (file order; as sorted records: a FASTQ that the host parses lands in parse chunks)
        os.environ["SS_READS_ORDER"] = "file"
        r1, r2 = _lib.ReadSet([p["bam"]]), _lib.ReadSet([p["fq_gz"]])
        out["same_reads"] = sorted(r1.read_back().split(b"\n")[:-1]) == sorted(r2.read_back().split(b"\n")[:-1])
        r1.close()
        r2.close()
        os.environ.pop("SS_READS_ORDER", None)
        if not a.no_cli:
            from tests import scenarios_mid as sm
            info = sm.build_mid(d)
            cli = {"bam": [], "fq_gz": []}
            env = dict(os.environ, SS_IMAGE_CACHE=os.path.join(d, "cache"))
            for _ in range(a.reps + 1):
                for key in ("bam", "fq_gz"):
                    o = os.path.join(d, "out_" + key)
                    t0 = time.perf_counter()
                    subprocess.run([sys.executable, "-m", "strainscan_amd.StrainScan", "-i", p[key], "-d", info["db_dir"], "-o", o],
                                   env=env, cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
                    cli[key].append(round(time.perf_counter() - t0, 3))
            out["cli_s"] = {k: dict(median=round(float(np.median(v[1:])), 3), all=v) for k, v in cli.items()}
            out["cli_note"] = ("fresh `python -m strainscan_amd.StrainScan -i FILE -d DB_M` processes (tests/scenarios_mid.py's database, "
                               "its image cached after the first run, which is not counted); random reads: the walk finds no cluster")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out["note"] = ("ss_reads_load of one file -> resident read set (binned), page cache warm, median of alternating runs; bam = "
                   "inflated on the device (ss_ginflate.hip, ss_gz_scratch.hip) + ss_bam_dev.hip, fq_gz = the same reads as a bgzip-style FASTQ through "
                   "ss_ginflate.hip + ss_fastq_dev.hip, bam_host = SS_GZ_GPU=0: host inflaters + the host decoder")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
