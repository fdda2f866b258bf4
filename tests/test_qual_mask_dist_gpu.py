"""The base-quality mask under torch.distributed: two ranks on one MI355X (gloo), each with the threshold of its own command line,
load their shares of a .fastq.gz pair -- the ranks SHARE each file's inflation (range mode) and every rank masks the records of its
own pieces -- of a BAM, and of both together; the ranks' counts add up to the single-process counts under the same threshold
(which are the oracle's on the masked reads), and their masked-base counters to the definition's count."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import bamio
from tests import qualmask as qm
from tests import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 20

WORKER = r'''
import ctypes as C, json, os, sys
import numpy as np
sys.path.insert(0, %(repo)r)
import torch
import torch.distributed as dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", init_method="file://" + os.environ["SS_TEST_STORE"], rank=rank, world_size=world)
import strainscan_amd
from strainscan_amd import _lib, dist as sdist
strainscan_amd.set_min_base_qual(%(q)d)
kdb = _lib.KmerDB.from_text(open(%(kfa)r, "rb").read(), 31, True)
out = {}
for key, paths in %(cases)r:
    c0 = _lib.mask_counters()
    rf0, rp0 = C.c_uint64(), C.c_uint64()
    _lib.lib().ss_gz_range_counters(C.byref(rf0), C.byref(rp0))
    rs = sdist.load_agreed(paths, lambda use: _lib.ReadSet(use, rank, world), discard=lambda r: r.close())
    c1 = _lib.mask_counters()
    rf1, rp1 = C.c_uint64(), C.c_uint64()
    _lib.lib().ss_gz_range_counters(C.byref(rf1), C.byref(rp1))
    kdb.reset()
    rs.scan_into(kdb)
    _lib.lib().ss_device_sync()
    out[key] = dict(counts=kdb.counts_rows().tolist(), n_records=rs.info()["n_records"], masked=c1["masked"] - c0["masked"],
                    no_qual=c1["bam_no_qual"] - c0["bam_no_qual"], range_files=rf1.value - rf0.value)
    rs.close()
out["bam_counters"] = _lib.bam_counters()
out["chain_failures"] = len(sdist.CHAIN_FAILURES)
json.dump(out, open(os.path.join(%(out)r, "rank%%d.json" %% rank), "w"))
dist.barrier()
dist.destroy_process_group()
'''


def test_two_ranks_mask_their_shares(tmp_path):
    from strainscan_amd import _lib as L
    L.require_gpu()
    rs = np.random.RandomState(15)
    g = synth.rand_seq(rs, 80000)
    kfa = b"".join(b">1\n" + g[i:i + 31] + b"\n" for i in range(0, 80000 - 31, 3))
    reads = [g[s:s + 150] for s in rs.randint(0, 80000 - 150, size=50000)]
    fq = qm.FastqSample(16, reads)
    half = 25777
    p1, p2, kp, bam = tmp_path / "s_1.fq.gz", tmp_path / "s_2.fq.gz", tmp_path / "k.fa", tmp_path / "s.bam"
    p1.write_bytes(gzip.compress(fq.text(0, 0, half), 6))
    p2.write_bytes(gzip.compress(fq.text(0, half, None), 6))
    kp.write_bytes(kfa)
    bs = qm.BamSample(17, qm.FastqSample(18, reads[:16000]))
    bam.write_bytes(bamio.bgzf(bamio.header(), bs.records(0), level=6))
    assert min(os.path.getsize(p) for p in (p1, p2, bam)) > (1 << 20)
    cases = [("gz", [str(p1), str(p2)]), ("bam", [str(bam)]), ("mix", [str(bam), str(p1), str(p2)])]
    as_fasta = lambda rd: b"".join(b">r\n" + r + b"\n" for r in rd)      # noqa: E731
    want_gz, _ = orc.jellyfish_count(kfa, [as_fasta(fq.masked_reads(Q))], k=31, upper=True)
    want_bam, _ = orc.jellyfish_count(kfa, [as_fasta(bs.kept_reads(Q))], k=31, upper=True)
    plain_gz, _ = orc.jellyfish_count(kfa, [as_fasta(fq.reads)], k=31, upper=True)
    assert 0 < int(want_gz.sum()) < int(plain_gz.sum())
    want = {"gz": want_gz.astype(np.int64), "bam": want_bam.astype(np.int64), "mix": want_gz.astype(np.int64) + want_bam}
    masked = {"gz": fq.masked(Q), "bam": bs.masked(Q), "mix": fq.masked(Q) + bs.masked(Q)}
    # the single-process result under the same threshold
    L.set_min_base_qual(Q)
    kdb = L.KmerDB.from_text(kfa, 31, True)
    try:
        for key, paths in cases:
            kdb.reset()
            kdb.scan_files(paths)
            assert np.array_equal(kdb.counts_rows(), want[key]), key
    finally:
        kdb.close()
        L.set_min_base_qual(0)
    world = 2
    code = WORKER % dict(repo=REPO, kfa=str(kp), cases=cases, out=str(tmp_path), q=Q)
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   SS_TEST_STORE=str(tmp_path / "store"), SS_GZ_SLICE_KB="256", SS_GZ_CHUNK="4096")
        for name in ("SS_GZ_GPU", "SS_GZ_RANGE", "SS_READS_ORDER"):
            env.pop(name, None)
        procs.append(subprocess.Popen([sys.executable, "-c", code], env=env, stderr=subprocess.PIPE))
    errs = [p.communicate(timeout=600)[1].decode()[-3000:] for p in procs]
    assert all(p.returncode == 0 for p in procs), errs
    outs = [json.loads((tmp_path / ("rank%d.json" % r)).read_text()) for r in range(world)]
    assert all(o["chain_failures"] == 0 for o in outs)
    for key, paths in cases:
        got = sum(np.array(o[key]["counts"], np.int64) for o in outs)
        assert np.array_equal(got, want[key]), key
        assert sum(o[key]["masked"] for o in outs) == masked[key], key
        assert sum(o[key]["no_qual"] for o in outs) == (0 if key == "gz" else bs.no_qual()), key
        assert sum(o[key]["n_records"] for o in outs) == {"gz": 50000, "bam": 16000, "mix": 66000}[key]
        if key != "bam":        # both .gz files were inflated once, shared between the ranks, and both ranks got records of them
            assert all(o[key]["range_files"] == 2 for o in outs), (key, outs[0][key]["range_files"], errs)
            assert all(0 < o[key]["masked"] < masked[key] for o in outs)
    assert all(o["bam_counters"]["device"] >= 2 for o in outs)
