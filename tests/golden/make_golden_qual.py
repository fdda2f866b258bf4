#!/opt/conda/bin/python3.9
"""Generate tests/golden/qual_mask.json by running the REAL jellyfish with -Q.

Runs only where the reference is mounted (like make_golden.py, whose setup_reference it borrows):

    python tests/golden/make_golden_qual.py            # ~1 min; the file regenerates byte-identically

Per case: the sha256 of kmer.fa and the inputs, Q, the sha256 of the counts over the rows of kmer.fa (rows as
identify.py:90-101 maps the dump to them), their sum, and the sum without -Q.  Inputs: scenarios_fuzz.fmt_case (uniform
qualities 33..73: Q in 1..3) and qualmask.real_case (the realistic profile: Q in 10, 20, 30); qualmask.qual_known_deviation
names what is left out and why.  tests/test_qual_mask_host.py holds the CPU oracle on qualmask.mask_fastx(inputs, Q) against
every entry: that pins the Python statement of the mask -- and so the product's definition -- to jellyfish's own."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, HERE]

from make_golden import setup_reference          # noqa: E402
from tests import qualmask as qm                 # noqa: E402
from tests import scenarios_fuzz as sf           # noqa: E402
from tests import synth                          # noqa: E402

FMT_SEEDS = range(0, 60)
REAL_SEEDS = range(0, 6)


def jellyfish_rows(jf, kfa_path, paths, q, n_rows, work):
    """identify.py:73-103 with -Q chr(33 + q) added to the count command (q = 0: the command as it is) -> counts per row."""
    out = os.path.join(work, "o.jf")
    qopt = ["-Q", chr(33 + q)] if q else []
    if any(p.endswith(".gz") for p in paths):
        zc = subprocess.Popen(["zcat"] + list(paths), stdout=subprocess.PIPE)
        subprocess.check_call([jf, "count", "/dev/fd/0", "-m", "31", "-s", "100M", "-t", "8"] + qopt + ["--if", kfa_path, "-o", out],
                              stdin=zc.stdout)
        zc.stdout.close()
        assert zc.wait() == 0
    else:
        subprocess.check_call([jf, "count", "-m", "31", "-s", "100M", "-t", "8"] + qopt + ["--if", kfa_path, "-o", out] + list(paths))
    dump = subprocess.check_output([jf, "dump", "-c", out]).decode()
    os.remove(out)
    index = {}
    with open(kfa_path) as f:
        lines = f.readlines()
    for i in range(len(lines) // 2):
        index[lines[2 * i + 1].rstrip().upper()] = i
    cnt = np.zeros(n_rows, np.int64)
    for ln in dump.splitlines():
        km, c = ln.rstrip().split(" ")
        cnt[index[km]] = int(c)
    return cnt.astype(np.uint32)


def one(jf, scratch, source, seed, q):
    root = tempfile.mkdtemp(prefix="%s_%d_" % (source, seed), dir=scratch)
    try:
        info, paths, blobs, kinds = (sf.fmt_case if source == "fmt" else qm.real_case)(seed, root)
        why = qm.qual_known_deviation(kinds)
        if why:
            return None, why
        kfa_path = os.path.join(info["db_dir"], "Tree_database", "kmer.fa")
        with open(kfa_path, "rb") as f:
            kfa = f.read()
        with_q = jellyfish_rows(jf, kfa_path, paths, q, info["n_rows"], root)
        without = jellyfish_rows(jf, kfa_path, paths, 0, info["n_rows"], root)
        return dict(source=source, seed=seed, kinds=kinds, q=q, sha256=synth.sha256_of(kfa, *blobs),
                    counts_sha256=synth.sha256_of(with_q.tobytes()), counts_sum=int(with_q.sum()), counts_sum_no_q=int(without.sum())), None
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    scratch = tempfile.mkdtemp(prefix="golden_qual_")
    try:
        _, jf = setup_reference(scratch)
        cases, skipped = [], {}
        for source, seeds, qs in (("fmt", FMT_SEEDS, (1, 2, 3)), ("real", REAL_SEEDS, (10, 20, 30))):
            for seed in seeds:
                g, why = one(jf, scratch, source, seed, qs[seed % 3])
                if g is None:
                    skipped[why] = skipped.get(why, 0) + 1
                    continue
                cases.append(g)
                print(source, seed, g["kinds"], "Q", g["q"], g["counts_sum_no_q"], "->", g["counts_sum"], flush=True)
        # the kept set cannot pass by counting nothing
        assert len(cases) >= 20, len(cases)
        shapes = {k.split("+")[0] for g in cases for k in g["kinds"]}
        assert {"fq4", "fq4_at", "fq_wrap", "fq4_crlf", "fq_plus_name"} <= shapes, shapes
        assert any(len(g["kinds"]) == 2 and {k[:2] for k in g["kinds"]} == {"fq", "fa"} for g in cases), "no FASTQ + FASTA pair"
        assert any(k.endswith("+gz") for g in cases for k in g["kinds"]), "no .gz"
        for g in cases:
            base = [k.split("+")[0] for k in g["kinds"]]
            if any(b.startswith("fq") and b != "fq4" or b == "real" for b in base):         # (fq4's quality is the constant 'I')
                assert 0 < g["counts_sum"] < g["counts_sum_no_q"], g
        with open(os.path.join(HERE, "qual_mask.json"), "w") as f:
            json.dump(dict(cases=cases, skipped=skipped), f, indent=1, sort_keys=True)
        print("wrote qual_mask.json: %d cases, skipped %s" % (len(cases), skipped))
    finally:
        shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
