"""`strainscan -i S.bam --pairs`: the FASTQ pair of tests/test_pairs_cli_gpu.py's sample written as ONE BAM -- the records shuffled
so that mates lie apart, a third of them 0x10, an empty mate as a record without bases, secondary and supplementary decoys under
the reads' names -- gives the per-read reports of `-i R1.fq -j R2.fq --pairs` on the same reads, as text; the names of
extracted/<table>_1.bam are those of the FASTQ run's <table>_1 file; stdout and the identification reports are those of the BAM run
without the flag, which joins nothing.  A BAM with a name that is not one first and one second mate says one line and writes no
per-read report; strainscan-multi joins once."""
import gzip
import os
import re

import numpy as np
import pytest

from tests import bamio
from tests.test_bam_select_gpu import HDR, walk
from tests.test_extract_cli_gpu import DIR, _files, _ok, _result_lines, _run, _with_cache, pair      # noqa: F401
from tests.test_pairs_cli_gpu import PER_READ, sample as fq_sample, tm      # noqa: F401

pytestmark = pytest.mark.gpu

M, N, B, SEED = 1, 2, 3, 5
FLAGS = ["--read_support", "--by_strain", "--classify_reads", str(M), "--bootstrap", str(B), "--bootstrap_seed", str(SEED), "-x", str(N)]


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _bam_records(seqs, seed, extra=()):
    """seqs = (mate 1 sequences, mate 2 sequences) -> the shuffled records of one BAM"""
    rs = np.random.RandomState(seed)
    recs = []
    for i, pair_ in enumerate(zip(*seqs)):
        for m, s in enumerate(pair_):
            rev = bool(s) and rs.random_sample() < 0.33
            recs.append(bamio.record("frag%d" % i, bamio.revcomp(s) if rev else s, flag=0x1 | (0x40, 0x80)[m] | (0x10 if rev else 0),
                                     qual=rs.randint(2, 41, size=len(s)).astype(np.uint8).tobytes()))
        if i % 40 == 0:
            other = "".join("ACGT"[j] for j in rs.randint(0, 4, size=120))
            recs.append(bamio.record("frag%d" % i, other, flag=(0x100 | 0x41) if i % 80 else (0x800 | 0x81 | 0x10)))
    recs += list(extra)
    return [recs[j] for j in rs.permutation(len(recs))]


@pytest.fixture(scope="module")
def sample(fq_sample, tmp_path_factory):      # noqa: F811
    """-> dict(bam=, fq=[R1, R2], stream=, n=the pairs): the same reads (upper case, as a BAM stores them) both ways"""
    root = tmp_path_factory.mktemp("bam_pairs_sample")
    seqs = [[s.decode().upper() for _, s in fq_sample["recs"][m]] for m in range(2)]
    assert all(set(s) <= set("ACGTN") for m in range(2) for s in seqs[m])
    fq = []
    for m in range(2):
        p = root / ("R%d.fq" % (m + 1))
        p.write_bytes(bamio.fastq(seqs[m], ["frag%d/%d" % (i, m + 1) for i in range(len(seqs[m]))]))
        fq.append(str(p))
    recs = _bam_records(seqs, 17)
    bam = root / "S.bam"
    bam.write_bytes(bamio.bgzf(HDR, recs, level=1))
    # mates lie apart: the sample is not collated
    names = [r[4] for r in walk(HDR + b"".join(recs))]
    assert sum(1 for a, b in zip(names, names[1:]) if a == b) < len(names) // 100
    return dict(bam=str(bam), fq=fq, stream=HDR + b"".join(recs), n=len(seqs[0]), seqs=seqs, root=root)


@pytest.fixture(scope="module")
def runs(L, mid_dbs, sample, tmp_path_factory):
    """name -> (err, stdout, stderr, out dir, joins made, bam extract calls made)"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("bam_pairs_cli")
    db = mid_dbs["DB_M"]["db_dir"]

    def go():
        out = {}
        for name, inp, extra in (("bam_off", ["-i", sample["bam"]], []), ("bam_on", ["-i", sample["bam"]], ["--pairs"]),
                                 ("fq_on", ["-i", sample["fq"][0], "-j", sample["fq"][1]], ["--pairs"])):
            j0, x0 = L.join_pairs_calls(), L.bam_extract_calls()
            od = str(root / name)
            err, _, text, errs = _run(StrainScan.main, inp + ["-d", db, "-o", od] + FLAGS + extra)
            out[name] = (err, text, errs, od, L.join_pairs_calls() - j0, L.bam_extract_calls() - x0)
        return out
    return _with_cache(root, go)


def test_per_read_reports_equal_those_of_the_fastq_pair(runs, sample):
    e_b, _, errs_b, d_b, joins_b, _ = runs["bam_on"]
    e_f, _, _, d_f, joins_f, _ = runs["fq_on"]
    assert _ok(e_b) and _ok(e_f) and joins_b == 1 and joins_f == 1
    for name in PER_READ:
        a, b = (open(os.path.join(d, name)).read() for d in (d_b, d_f))
        assert a == b and len(a.split("\n")) > 2, name
    reads = {ln.split("\t")[2] for ln in open(os.path.join(d_b, "read_support.tsv")).read().split("\n")[1:] if ln}
    assert reads == {str(sample["n"])}                               # `reads` counts fragments
    line = [ln for ln in errs_b.split("\n") if ln.startswith("pairs: ")]
    assert len(line) == 1, line
    m = re.fullmatch(r"pairs: (\d+) pairs joined\t(\d+) orphans\t(\d+) singles\t(\d+) bytes on the device", line[0])
    empty = sum(1 for a, b in zip(*sample["seqs"]) if not a or not b)
    assert m and int(m.group(1)) == sample["n"] - empty and int(m.group(2)) == empty > 0 and int(m.group(3)) == 0, line


def test_extracted_bam_names_are_those_of_the_fastq_run(runs):
    _, _, errs, d_b, _, calls = runs["bam_on"]
    d_f = runs["fq_on"][3]
    ex = os.path.join(d_b, DIR)
    files = sorted(os.listdir(ex))
    assert files and all(f.endswith("_1.bam") for f in files) and calls == len(files)
    assert any("." in f.split("_")[0] for f in files) and "tree_1.bam" in files          # --by_strain's files and the tables'
    seen = 0
    for f in files:
        t = f[:-len("_1.bam")]
        recs = walk(gzip.decompress(open(os.path.join(ex, f), "rb").read()))
        assert all(not r[2] & 0x900 and r[3] for r in recs)              # never a record that is not kept
        got = sorted({r[4] for r in recs})
        fq = open(os.path.join(d_f, DIR, "%s_1.fastq" % t), "rb").read().split(b"\n")
        want = sorted(ln[1:].rsplit(b"/", 1)[0] for ln in fq[0:-1:4])
        assert got == want, (t, len(got), len(want))
        seen += len(got)
    assert seen
    lines = [ln for ln in errs.split("\n") if ln.startswith("extract_reads:")]
    assert len(lines) == len(files) and all("\tfragments selected on the device " in ln for ln in lines)


def test_stdout_and_the_identification_do_not_depend_on_the_flag(runs):
    e0, t0, errs0, d0, joins0, calls0 = runs["bam_off"]
    e1, t1, _, d1, _, calls1 = runs["bam_on"]
    assert _ok(e0) and _ok(e1) and type(e0) is type(e1)
    # without the flag: no join, -x on a BAM as before (one call per file written, selected by record)
    assert joins0 == 0 and "pairs:" not in errs0 and calls0 == calls1 > 0
    assert "fragments selected" not in errs0 and "\tselected on the device " in errs0
    assert t0 == t1 or _result_lines(t0) == _result_lines(t1)
    assert _result_lines(t0)
    mine = lambda k: os.path.basename(k) in PER_READ or DIR in k.split(os.sep)      # noqa: E731
    a, b = ({k: v for k, v in _files(d).items() if not mine(k)} for d in (d0, d1))
    assert any(k.endswith("StrainVote.report") for k in a) and "final_report.txt" in a
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    for name in PER_READ:
        assert open(os.path.join(d0, name)).readline() == open(os.path.join(d1, name)).readline(), name
    assert any(open(os.path.join(d0, name)).read() != open(os.path.join(d1, name)).read() for name in PER_READ)


def test_a_violation_says_one_line_and_writes_no_per_read_report(L, mid_dbs, sample, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    third = bamio.record("frag7", "ACGT" * 30, flag=0x41)
    bam = tmp_path / "V.bam"
    bam.write_bytes(bamio.bgzf(HDR, _bam_records(sample["seqs"], 18, extra=[third]), level=1))
    base = ["-i", str(bam), "-d", mid_dbs["DB_M"]["db_dir"]]
    outs = {}
    for name, extra in (("plain", []), ("pairs", FLAGS + ["--pairs"])):
        x0 = L.bam_extract_calls()
        od = str(tmp_path / name)
        err, _, text, errs = _run(StrainScan.main, base + ["-o", od] + extra)
        assert _ok(err), err
        outs[name] = (type(err), _result_lines(text), errs, _files(od))
        assert L.bam_extract_calls() == x0
    lines = [ln for ln in outs["pairs"][2].split("\n") if ln.startswith(("pairs:", "read_support:", "extract_reads:", "classify_reads:", "bootstrap:"))]
    assert lines == ["pairs: has read names that are not one first and one second mate (3 records) and no per-read report was written"], lines
    assert outs["pairs"][0] is outs["plain"][0] and outs["pairs"][1] == outs["plain"][1] and outs["pairs"][3] == outs["plain"][3]


def test_two_bams_stay_refused(L, mid_dbs, sample, tmp_path, monkeypatch):
    from strainscan_amd import db as ssdb
    js, why = ssdb.resident_pairs((sample["bam"], sample["bam"]))
    assert js is None and why == ("takes FASTA/FASTQ inputs (the mates of a pair are not adjacent in a coordinate-sorted BAM; "
                                  "pairs from BAM are not built)")
    js, why = ssdb.resident_pairs((sample["bam"], sample["fq"][1]))
    assert js is None and "pairs from BAM are not built" in why
    js, why = ssdb.resident_pairs((sample["fq"][0], ""))
    assert js is None and why == "needs the two files of a paired sample (-i and -j)"


def test_multi_db_joins_once(L, runs, mid_dbs, sample, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbm, dbmem = mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]
    before = L.join_pairs_calls()
    err, rc, _, errs = _run(multi_db.main, ["-i", sample["bam"], "-d", dbm, "-d", "mem=" + dbmem, "-o", str(tmp_path / "out"),
                                            "--read_support", "--classify_reads", str(M), "--pairs"])
    assert err is None and rc == 0
    assert L.join_pairs_calls() == before + 1
    assert len([ln for ln in errs.split("\n") if ln.startswith("pairs: ")]) == 1
    for label in (os.path.basename(os.path.normpath(dbm)), "mem"):
        for name in ("read_support.tsv", "read_classes.tsv"):
            assert open(os.path.join(str(tmp_path / "out"), label, name)).read() == open(os.path.join(runs["bam_on"][3], name)).read(), (label, name)
