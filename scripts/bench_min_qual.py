#!/usr/bin/env python3
"""What the base-quality mask (-q / ss_set_min_base_qual) costs a load: ss_reads_load of (a) FASTQ text, (b) a .fastq.gz pair,
(c) a BAM, at threshold 0 and 20, and -- with --parent-tree DIR, a checkout of the commit before the feature with its library built
-- the same loads by that commit's library in the same run.  One JSON line.

Protocol.  The sample is made once (not timed; scripts/bench_bam.py's generator: random reads, Phred-like qualities that fall along
the read).  Every measurement runs in a child process of its own: one untimed load, then --reps timed loads per threshold, the
thresholds alternating load by load.  Per input the children alternate: this tree, the parent tree, this tree, the parent tree --
so each side is measured twice and `spread_ms` (the difference of its two medians) says what a difference between the sides is
worth.  `off_costs_ms` = median(this tree at 0) - median(parent); `on_costs_ms` = median(at 20) - median(at 0), this tree.
Kernel times: `rocprofv3 --kernel-trace --stats -- python scripts/bench_min_qual.py --child --kind gz|bam --qs 0|20 --reps 3
--paths ...` on the files of a run kept with --keep (kernels `fq_copy_kernel`, `bam_decode_kernel`)."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    tree = os.path.abspath(a.tree or ROOT)
    sys.path.insert(0, tree)
    from strainscan_amd import _lib
    _lib.require_gpu()
    qs = [int(q) for q in a.qs.split(",")]
    can_set = hasattr(_lib, "set_min_base_qual")
    assert can_set or qs == [0], "this tree has no threshold to set"

    def load(q):
        if can_set:
            _lib.set_min_base_qual(q)
        t0 = time.perf_counter()
        rs = _lib.ReadSet(a.paths)
        _lib.check(_lib.lib().ss_device_sync(), "sync")
        dt = (time.perf_counter() - t0) * 1e3
        info = rs.info()
        rs.close()
        return dt, info

    _lib.warm_up(ingest=a.kind == "text", gz=len(a.paths) if a.kind != "text" else 0)
    load(qs[0])
    times = {q: [] for q in qs}
    c0 = _lib.mask_counters() if can_set else None
    info = None
    for _ in range(a.reps):
        for q in qs:
            ms, info = load(q)
            times[q].append(round(ms, 1))
    out = dict(tree=os.path.relpath(tree, ROOT), kind=a.kind, times={str(q): v for q, v in times.items()}, n_records=info["n_records"], n_bases=info["n_bases"])
    if can_set:
        c1 = _lib.mask_counters()
        out["masked_per_load"] = (c1["masked"] - c0["masked"]) // max(1, a.reps) if any(qs) else 0
    print(json.dumps(out))


def run_child(tree, kind, paths, qs, reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--kind", kind, "--qs", ",".join(map(str, qs)), "--reps", str(reps),
           "--paths"] + list(paths)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, cwd=tree, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("child failed (%d): %s" % (r.returncode, " ".join(cmd)))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def make_inputs(d, a):
    sys.path.insert(0, ROOT)
    from scripts import bench_bam as bb
    from multiprocessing import Pool
    out = {}
    kinds = a.kinds.split(",")
    if "bam" in kinds:
        p = bb.make_sample(d, a.bam_reads, a.procs)                   # sample.bam (+ a bgzip-style .fq.gz that is not used here)
        os.unlink(p["fq_gz"])
        out["bam"] = [p["bam"]]
    per = 250000

    def text(first_seed, n, path):
        pieces = [(first_seed + i, i * per, min(per, n - i * per)) for i in range((n + per - 1) // per)]
        with Pool(a.procs) as pool, open(path, "wb") as f:
            for blob in pool.imap(bb._fastq_text, pieces):
                f.write(blob)
        return path

    if "text" in kinds:
        out["text"] = [text(5000, a.text_reads, os.path.join(d, "text.fq"))]
    if "gz" not in kinds:
        return out
    halves = [text(7000 + 500 * i, a.gz_reads // 2, os.path.join(d, "pair_%d.fq" % (i + 1))) for i in range(2)]
    for q in [subprocess.Popen(["gzip", "-1", h]) for h in halves]:
        assert q.wait() == 0
    out["gz"] = [h + ".gz" for h in halves]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree")
    ap.add_argument("--kind", choices=["text", "gz", "bam"])
    ap.add_argument("--qs", default="0,20")
    ap.add_argument("--paths", nargs="+")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-tree", help="a checkout of the commit before the feature, its library built")
    ap.add_argument("--text-reads", type=int, default=20_000_000)
    ap.add_argument("--gz-reads", type=int, default=2_000_000)
    ap.add_argument("--bam-reads", type=int, default=4_000_000)
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--keep", help="keep the sample in this directory")
    ap.add_argument("--kinds", default="text,gz,bam", help="the inputs to make and measure")
    a = ap.parse_args()
    if a.child:
        return child(a)
    d = a.keep or tempfile.mkdtemp(prefix="ss_bench_minq_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(d, exist_ok=True)
    out = dict(threshold=20, reps=a.reps, reads=dict(text=a.text_reads, gz=a.gz_reads, bam=a.bam_reads), inputs={})
    try:
        t0 = time.perf_counter()
        inputs = make_inputs(d, a)
        out["generate_s"] = round(time.perf_counter() - t0, 1)
        print("sample written in %.0f s" % out["generate_s"], file=sys.stderr, flush=True)
        med = lambda v: round(float(np.median(v)), 1)      # noqa: E731
        for kind in a.kinds.split(","):
            paths = inputs[kind]
            e = dict(mb=round(sum(os.path.getsize(p) for p in paths) / 1e6, 1), new=[], parent=[])
            for _ in range(2):
                e["new"].append(run_child(ROOT, kind, paths, [0, 20], a.reps))
                if a.parent_tree:
                    e["parent"].append(run_child(os.path.abspath(a.parent_tree), kind, paths, [0], a.reps))
            new0 = [t for c in e["new"] for t in c["times"]["0"]]
            new20 = [t for c in e["new"] for t in c["times"]["20"]]
            s = dict(new_q0_ms=med(new0), new_q20_ms=med(new20), on_costs_ms=round(med(new20) - med(new0), 1),
                     on_ratio=round(med(new20) / med(new0), 3),
                     new_spread_ms=round(abs(med(e["new"][0]["times"]["0"]) - med(e["new"][1]["times"]["0"])), 1),
                     masked_share=round(e["new"][0]["masked_per_load"] / max(1, e["new"][0]["n_bases"] - e["new"][0]["n_records"]), 4))
            if a.parent_tree:
                par = [t for c in e["parent"] for t in c["times"]["0"]]
                s.update(parent_ms=med(par), off_costs_ms=round(med(new0) - med(par), 1),
                         parent_spread_ms=round(abs(med(e["parent"][0]["times"]["0"]) - med(e["parent"][1]["times"]["0"])), 1),
                         on_over_parent=round(med(new20) / med(par), 3))
            e["summary"] = s
            print(kind, json.dumps(s), file=sys.stderr, flush=True)
            out["inputs"][kind] = e
    finally:
        if not a.keep:
            shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
