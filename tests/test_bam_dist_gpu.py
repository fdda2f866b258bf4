"""A BAM sharded over 2 and 3 ranks on one MI355X (torch.distributed, gloo): every rank loads its share through
dist.load_agreed -- alone and beside a .fastq.gz file in the same call, so that the range mode's chain of that file runs
while the BAM takes the whole-file device path -- and the ranks' counts add up to the counts of the whole sample."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bamio
from tests.test_bam_gpu import _genome_reads

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, %(repo)r)
import torch
import torch.distributed as dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", init_method="file://" + os.environ["SS_TEST_STORE"], rank=rank, world_size=world)
from strainscan_amd import _lib, dist as sdist
kdb = _lib.KmerDB.from_text(open(%(kfa)r, "rb").read(), 31, True)
out = {}
for key, paths in %(cases)r:
    rs = sdist.load_agreed(paths, lambda use: _lib.ReadSet(use, rank, world), discard=lambda r: r.close())
    kdb.reset()
    rs.scan_into(kdb)
    _lib.lib().ss_device_sync()
    out[key] = dict(counts=kdb.counts_rows().tolist(), n_records=rs.info()["n_records"])
    rs.close()
out["bam_counters"] = _lib.bam_counters()
json.dump(out, open(os.path.join(%(out)r, "rank%%d.json" %% rank), "w"))
dist.barrier()
dist.destroy_process_group()
'''


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    root = tmp_path_factory.mktemp("ss_bam_dist")
    reads, kfa = _genome_reads(8, 24000)
    recs = bamio.sample_records(5, reads, aligned=True, decoys=0.1, extras=True)
    bam = root / "s.bam"
    bam.write_bytes(bamio.bgzf(bamio.header(), recs, level=6))
    assert os.path.getsize(bam) >= 1 << 20
    other, _ = _genome_reads(9, 20000)
    fqgz = root / "o.fq.gz"
    fqgz.write_bytes(bamio.bgzip_text(bamio.fastq([s for _, s in other])))
    kp = root / "k.fa"
    kp.write_bytes(kfa)
    return str(bam), str(fqgz), str(kp), len(reads), len(other)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_bam_counts_add_up(world, sample, tmp_path):
    from strainscan_amd import _lib
    _lib.require_gpu()
    bam, fqgz, kfa, n_bam, n_fq = sample
    cases = [("bam", [bam]), ("mix", [bam, fqgz])]
    kdb = _lib.KmerDB.from_text(open(kfa, "rb").read(), 31, True)
    want = {}
    try:
        for key, paths in cases:
            kdb.reset()
            kdb.scan_files(paths)
            want[key] = kdb.counts_rows().astype(np.int64)
    finally:
        kdb.close()
    code = WORKER % dict(repo=REPO, kfa=kfa, cases=cases, out=str(tmp_path))
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   SS_TEST_STORE=str(tmp_path / "store"))
        procs.append(subprocess.Popen([sys.executable, "-c", code], env=env, stderr=subprocess.PIPE))
    errs = [p.communicate(timeout=600)[1].decode()[-3000:] for p in procs]
    assert all(p.returncode == 0 for p in procs), errs
    outs = [json.loads((tmp_path / ("rank%d.json" % r)).read_text()) for r in range(world)]
    for key, _ in cases:
        got = sum(np.array(o[key]["counts"], np.int64) for o in outs)
        assert np.array_equal(got, want[key]), (world, key)
        n = sum(o[key]["n_records"] for o in outs)
        assert n == n_bam + (n_fq if key == "mix" else 0), (world, key, n)
    assert all(o["bam_counters"]["device"] >= 1 for o in outs)          # the BAM took the device path on every rank
