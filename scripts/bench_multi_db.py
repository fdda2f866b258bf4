#!/usr/bin/env python3
"""The fused tree pass of `strainscan-multi` (ss_scan_reads_multi, every tree table behind its own Bloom filter) against N
single-table scans of the same resident, binned read set.

Builds N tree tables of E. coli shape (bench.make_db: a 1645-node tree of sampled node sets, the tables bench.py measures)
from distinct seeds; the sample's reads come from the first database's strains (bench.make_reads), so table 0 has hits and
the others have (almost) none -- one sample against the databases of several species.  For N = 1, 2, 4, 8 it times, with
HIP events on the default stream, the N single-table scans (ss_scan_reads each) and the one fused call, after a warm-up, and
checks that the counts are equal.

    bench_multi_db.py [n_reads = 20000000] [Ns = 1,2,4,8] [steps = 5]

Prints one JSON line.  Run every GPU step under a time limit of its own (`timeout -k 10 ...`), chained with `&&`."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

C = 823                  # leaves: 1645 nodes, the E. coli tree's size


def main():
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000_000
    ns = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "1,2,4,8").split(",")]
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    import torch
    from strainscan_amd import _lib
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    specs = [bench.make_db(torch, dev, C, seed=20240101 + 17 * i, shape="sampled") for i in range(max(ns))]
    dbs = [_lib.KmerDB(s["keys"], np.ones(s["keys"].size, np.uint8), 31, True) for s in specs]
    reads = bench.make_reads(torch, dev, specs[0], n_reads, seed=5, hit_frac=0.05)
    rs = _lib.ReadSet.from_flat_dev(reads.data_ptr(), reads.numel(), order=True)
    del reads
    torch.cuda.synchronize()
    out = dict(n_reads=n_reads, tree_rows=[int(s["keys"].size) for s in specs],
               filter_bits=[db.info()["filter_bits"] for db in dbs], packed_slabs=rs.packed_slabs(),
               setup_s=round(time.perf_counter() - t0, 1), runs=[])

    def timed(fn):
        ts = []
        for i in range(steps + 1):                    # (the first call: the probe of each (read set, table) pair)
            for db in dbs:
                db.reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i:
                ts.append(a.elapsed_time(b))
        return round(float(np.median(ts)), 3), round(float(min(ts)), 3)

    for n in ns:
        tabs = dbs[:n]

        def single():
            for db in tabs:
                rs.scan_into(db)

        single_ms = timed(single)
        want = [db.counts_rows() for db in tabs]
        l0 = _lib.scan_multi_launches()
        fused_ms = timed(lambda: rs.scan_into_many(tabs))
        l1 = _lib.scan_multi_launches()
        equal = all(np.array_equal(db.counts_rows(), w) for db, w in zip(tabs, want))
        out["runs"].append(dict(n_tables=n, single_scans_ms_median_min=single_ms, fused_ms_median_min=fused_ms,
                                fused_over_one_table=round(fused_ms[0] / (single_ms[0] / n), 2) if n else None,
                                fused_over_n_single=round(fused_ms[0] / single_ms[0], 2), counts_equal=equal,
                                bloom_launches=l1["bloom"] - l0["bloom"], hits_table0=int(want[0].sum())))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
