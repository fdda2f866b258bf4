"""What binning one slab of 20 M one-length reads costs (ss_reorder.hip order_flat_dev), on the product's path and on its
fallbacks, each beside ss_test_hook 6 = 1 (the count + atomic placement):

  packed    every byte A C G T: key pass, sort, packed gather
  lower     every base lower case: the packed gather finds a byte it cannot pack, the gather runs again with ASCII output
  newline   one newline in the middle of one record (the byte count still divides): the gather's check sends the slab
            through the general passes

Median of `--reps` calls each: wall time (allocation included) and ss_reads_order_timing.  One JSON line.
Usage: python scripts/bench_binning_fallbacks.py [--reads 20000000] [--length 150] [--reps 5]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_slab(torch, n, length, seed):
    """n records of `length` random bases + '\\n', flat on the device."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    c = torch.randint(0, 4, (n, length + 1), generator=g, device="cuda", dtype=torch.uint8)
    a = 65 + 2 * (c >= 1).to(torch.uint8) + 4 * (c >= 2).to(torch.uint8) + 13 * (c >= 3).to(torch.uint8)     # A C G T
    del c
    a[:, length] = 10
    return a.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from strainscan_amd import _lib as L
    L.require_gpu()
    base = make_slab(torch, args.reads, args.length, 11)
    out = dict(reads=args.reads, length=args.length, reps=args.reps, cases={})
    for case in ("packed", "lower", "newline"):
        slab = base.clone()
        if case == "lower":
            slab.bitwise_or_((slab != 10).to(torch.uint8) << 5)
        elif case == "newline":
            slab[(args.reads // 2) * (args.length + 1) + args.length // 2] = 10
        torch.cuda.synchronize()
        for hook in (0, 1):
            walls, parts, used, packed = [], [], None, None
            L.check(L.lib().ss_test_hook(6, hook), "ss_test_hook")
            try:
                for _ in range(args.reps):
                    c0 = (C.c_uint64 * 2)()
                    L.check(L.lib().ss_reads_order_counters(c0), "ss_reads_order_counters")
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    rs = L.ReadSet.from_flat_dev(slab.data_ptr(), slab.numel(), order=True)
                    torch.cuda.synchronize()
                    walls.append((time.perf_counter() - t) * 1e3)
                    p = np.zeros(3)
                    L.check(L.lib().ss_reads_order_timing(L.ptr(p)), "ss_reads_order_timing")
                    parts.append(p)
                    c1 = (C.c_uint64 * 2)()
                    L.check(L.lib().ss_reads_order_counters(c1), "ss_reads_order_counters")
                    used = "one_length" if c1[0] - c0[0] == 1 else "general"
                    packed = rs.packed_slabs()
                    rs.close()
            finally:
                L.lib().ss_test_hook(6, 0)
            pm = np.median(np.array(parts), axis=0)
            out["cases"]["%s%s" % (case, "_hook6" if hook else "")] = dict(
                passes=used, packed_slabs=packed, wall_ms=round(float(np.median(walls)), 3),
                timing_ms=[round(float(x), 3) for x in pm], kernels_ms=round(float(pm[0] + pm[2]), 3))
        del slab
    print(json.dumps(out))


if __name__ == "__main__":
    main()
