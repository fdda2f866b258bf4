"""The base-quality mask (-q / --min_base_qual) on the MI355X.  One property throughout: the product run with threshold Q on X
equals, byte for byte, the product run without a threshold on mask(X, Q) (tests/qualmask.py; pinned to the real
`jellyfish count -Q` by tests/test_qual_mask_host.py) -- resident flat blocks for every decoder, row counts of a tree table and of a
layer-2 cluster table (against the oracle on mask(X) too), and the files the commands write.  Every test that claims a decoder
asserts through the library's counters that it ran."""
import contextlib
import ctypes as C
import gzip
import io
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import bamio
from tests import qualmask as qm
from tests import scenarios as sc
from tests import scenarios_fuzz as sf
from tests import synth
from tests.test_bam_gpu import OPTIONS, _padded, records

pytestmark = pytest.mark.gpu

Q = 20


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    yield _lib
    _lib.set_min_base_qual(0)


@pytest.fixture(autouse=True)
def _threshold_off_again():
    yield
    from strainscan_amd import _lib
    _lib.set_min_base_qual(0)


def _gz_counters(L):
    a, b = C.c_uint64(), C.c_uint64()
    L.check(L.lib().ss_gz_gpu_counters(C.byref(a), C.byref(b)), "ss_gz_gpu_counters")
    return a.value, b.value


def _order_counters(L):
    out = (C.c_uint64 * 2)()
    L.check(L.lib().ss_reads_order_counters(out), "ss_reads_order_counters")
    return out[0], out[1]


def _load(L, paths, q, monkeypatch, order="file", gz_gpu=None, threads=None):
    """-> (read-back bytes, info, bases masked, BAM records without qualities, packed slabs) of one ss_reads_load under threshold q"""
    for name, val in (("SS_READS_ORDER", order), ("SS_GZ_GPU", gz_gpu), ("SS_INGEST_THREADS", threads)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    L.set_min_base_qual(q)
    c0 = L.mask_counters()
    rs = L.ReadSet(paths)
    try:
        c1 = L.mask_counters()
        return rs.read_back(), rs.info(), c1["masked"] - c0["masked"], c1["bam_no_qual"] - c0["bam_no_qual"], rs.packed_slabs()
    finally:
        rs.close()
        L.set_min_base_qual(0)


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """40 000 reads of 150 bases with the realistic quality profile: X and mask(X, Q) as plain text (12 MB: the threaded ingest),
    .fastq.gz (> 1 MB: the device path) and a small head of both; a k-mer table of the genome."""
    root = tmp_path_factory.mktemp("ss_qual")
    rs = np.random.RandomState(21)
    g = synth.rand_seq(rs, 60000)
    reads = []
    for s in rs.randint(0, 60000 - 150, size=40000):
        r = g[s:s + 150]
        if rs.random_sample() < 0.05:
            j = int(rs.randint(0, 150))
            r = r[:j] + b"N" + r[j + 1:]
        reads.append(synth.revcomp(r) if rs.random_sample() < 0.5 else r)
    fq = qm.FastqSample(22, reads)
    kfa = b"".join(b">1\n" + g[i:i + 31] + b"\n" for i in range(0, 60000 - 31, 3))
    out = dict(fq=fq, kfa=kfa, root=root)
    for q in (0, Q):
        text = fq.text(q)
        assert len(text) > (8 << 20)
        (root / ("x%d.fq" % q)).write_bytes(text)
        (root / ("x%d.fq.gz" % q)).write_bytes(gzip.compress(text, 1))
        assert os.path.getsize(root / ("x%d.fq.gz" % q)) > (1 << 20)
        (root / ("small%d.fq.gz" % q)).write_bytes(gzip.compress(fq.text(q, 0, 3000), 6))
        out[q] = {k: str(root / (k % q)) for k in ("x%d.fq", "x%d.fq.gz", "small%d.fq.gz")}
    head = fq.text(0, 0, 500)
    c = [0]
    assert qm.mask_fastx(head, Q, c) == fq.text(Q, 0, 500) and c[0] > 0          # the arrays' mask is the definition's
    assert 0 < fq.masked(Q) < sum(len(r) for r in reads) // 10
    return out


# ------------------------------------------------------------------------------------------------
# 1. read-back, decoder by decoder
# ------------------------------------------------------------------------------------------------
def test_device_fastq_gz(L, sample, monkeypatch):
    """ss_fastq_dev.hip's masked copy: the resident block of X.fastq.gz under Q is the block of mask(X).fastq.gz, the counter moves
    by the definition's count, and threshold 0 gives the unmasked bases."""
    fq = sample["fq"]
    h0 = _gz_counters(L)
    got, info, n_masked, _, _ = _load(L, [sample[0]["x%d.fq.gz"]], Q, monkeypatch)
    want, _, none_masked, _, _ = _load(L, [sample[Q]["x%d.fq.gz"]], 0, monkeypatch)
    plain, _, _, _, _ = _load(L, [sample[0]["x%d.fq.gz"]], 0, monkeypatch)
    h1 = _gz_counters(L)
    assert h1[0] == h0[0] + 3 and h1[1] == h0[1], "the device path must have taken all three loads"
    assert got == want == _padded(fq.flat(Q))
    assert plain == _padded(fq.flat(0)) and plain != got
    assert (n_masked, none_masked) == (fq.masked(Q), 0)
    assert info["n_records"] == len(fq.reads) and info["n_bases"] == len(fq.flat(0))
    # binned: a one-length sample with masked bases is still packed, and holds the same records
    o0 = _order_counters(L)
    got_b, _, _, _, packed = _load(L, [sample[0]["x%d.fq.gz"]], Q, monkeypatch, order=None)
    assert packed > 0 and _order_counters(L)[0] > o0[0]
    assert records(got_b) == records(want)


def test_device_fastq_gz_ragged_lengths(L, tmp_path, monkeypatch):
    """Reads of every length from 0 to 300 -- those whose line and '\\n' fill whole 16-byte groups (15, 31, 47, ...) among them,
    where the copy's last group carries the '\\n' that has no quality -- through the device path; the last record ends the text
    without a newline."""
    rs = np.random.RandomState(5)
    reads = [synth.rand_seq(rs, int(n)) for n in rs.permutation(np.repeat(np.arange(0, 301), 60))]
    reads.append(synth.rand_seq(rs, 47))
    fq = qm.FastqSample(6, reads)
    paths = {}
    for q in (0, Q):
        text = fq.text(q)[:-1]
        assert qm.mask_fastx(fq.text(0, 0, 400), q) == fq.text(q, 0, 400)
        paths[q] = tmp_path / ("ragged%d.fq.gz" % q)
        paths[q].write_bytes(gzip.compress(text, 1))
        assert os.path.getsize(paths[q]) > (1 << 20)
    h0 = _gz_counters(L)
    got, info, n_masked, _, _ = _load(L, [str(paths[0])], Q, monkeypatch)
    want, _, _, _, _ = _load(L, [str(paths[Q])], 0, monkeypatch)
    assert _gz_counters(L)[0] == h0[0] + 2
    assert got == want == _padded(fq.flat(Q)) and n_masked == fq.masked(Q)
    assert info["n_records"] == len(reads)


@pytest.mark.parametrize("what,gz_gpu,threads", [("x%d.fq.gz", "0", None), ("x%d.fq", None, None), ("x%d.fq", None, "1"), ("small%d.fq.gz", "0", None)])
def test_host_inflated_gz_and_threaded_text(L, sample, what, gz_gpu, threads, monkeypatch):
    """A .fastq.gz inflated on the host (SS_GZ_GPU=0) and plain text, both through the parse threads' in-memory grammar (a small
    file: through the streaming reader).  The parse chunks land in the slab in the order the threads finish: the same records;
    with one parse thread, or one chunk, the same bytes."""
    fq = sample["fq"]
    n = 3000 if what.startswith("small") else len(fq.reads)
    h0 = _gz_counters(L)
    got, info, n_masked, _, _ = _load(L, [sample[0][what]], Q, monkeypatch, gz_gpu=gz_gpu, threads=threads)
    want, _, none_masked, _, _ = _load(L, [sample[Q][what]], 0, monkeypatch, gz_gpu=gz_gpu, threads=threads)
    plain, _, _, _, _ = _load(L, [sample[0][what]], 0, monkeypatch, gz_gpu=gz_gpu, threads=threads)
    assert _gz_counters(L)[0] == h0[0], "the device path must not have run"
    assert records(got) == records(want) == sorted(fq.masked_reads(Q)[:n])
    assert records(plain) == sorted(fq.reads[:n])
    if threads == "1" or what.startswith("small"):
        assert got == want
    assert n_masked == int(sum(int((ql < Q).sum()) for ql in fq.quals[:n])) and none_masked == 0
    assert info["n_records"] == n


@pytest.fixture(scope="module")
def bams(tmp_path_factory, sample):
    """name -> (X.bam, mask(X).bam, BamSample) for the writer options of tests/test_bam_gpu.py (every BAM >= 1 MB), reverse-strand
    records, records without qualities and -- `long_reads` -- reads of 70-150 kb among them; and a small file for the host path."""
    root = tmp_path_factory.mktemp("ss_qual_bam")
    fq = sample["fq"]
    out = {}
    for i, (name, opt) in enumerate(OPTIONS.items()):
        reads, names = list(fq.reads[:14000]), list(fq.names[:14000])
        if opt.get("long"):
            rs = np.random.RandomState(77)
            longs = [synth.rand_seq(rs, int(rs.randint(70000, 150000))) for _ in range(12)]
            reads = reads[:2000] + longs + reads[2000:]
            names = names[:2000] + [b"long%d" % j for j in range(12)] + names[2000:]
        f = qm.FastqSample(40 + i, reads, names)
        bs = qm.BamSample(50 + i, f, reverse_share=0.5 if opt["aligned"] else 0.0, decoys=opt["decoys"], extras=opt["extras"])
        paths = []
        for q in (0, Q):
            data = bamio.bgzf(bamio.header(), bs.records(q), level=opt["level"], cuts=opt["cuts"], eof=opt["eof"], seed=i)
            assert len(data) >= 1 << 20
            p = root / ("%s_%d.bam" % (name, q))
            p.write_bytes(data)
            paths.append(str(p))
        assert bs.no_qual() > 0 and bs.masked(Q) > 0
        out[name] = (paths[0], paths[1], bs)
    f = qm.FastqSample(60, fq.reads[:500], fq.names[:500])
    bs = qm.BamSample(61, f, decoys=0.2)
    paths = []
    for q in (0, Q):
        p = root / ("small_%d.bam" % q)
        p.write_bytes(bamio.bgzf(bamio.header(), bs.records(q), level=6))
        paths.append(str(p))
    out["small"] = (paths[0], paths[1], bs)
    return out


@pytest.mark.parametrize("name", list(OPTIONS))
def test_device_and_host_bam(L, bams, name, monkeypatch):
    """bam_decode_kernel's masked instantiation and the host decoder: X.bam under Q == mask(X).bam; records without qualities are
    left alone and counted once each; low qualities of skipped records count for nothing."""
    x, m, bs = bams[name]
    want_flat = b"".join(r + b"\n" for r in bs.kept_reads(Q))
    c0 = L.bam_counters()
    got, info, n_masked, n_noq, _ = _load(L, [x], Q, monkeypatch)
    want, _, none_masked, none_noq, _ = _load(L, [m], 0, monkeypatch)
    plain, _, _, _, _ = _load(L, [x], 0, monkeypatch)
    c1 = L.bam_counters()
    assert c1["device"] == c0["device"] + 3 and c1["host"] == c0["host"], (c0, c1)
    assert got == want == _padded(want_flat)
    assert plain == _padded(b"".join(r + b"\n" for r in bs.kept_reads(0)))
    assert (n_masked, n_noq, none_masked, none_noq) == (bs.masked(Q), bs.no_qual(), 0, 0)
    assert info["n_records"] == len(bs.fq.reads)
    got_h, _, h_masked, h_noq, _ = _load(L, [x], Q, monkeypatch, gz_gpu="0")
    assert L.bam_counters()["host"] == c1["host"] + 1
    assert got_h == got and (h_masked, h_noq) == (bs.masked(Q), bs.no_qual())


def test_small_bam_on_the_host(L, bams, monkeypatch):
    x, m, bs = bams["small"]
    c0 = L.bam_counters()
    got, _, n_masked, n_noq, _ = _load(L, [x], Q, monkeypatch)
    want, _, _, _, _ = _load(L, [m], 0, monkeypatch)
    c1 = L.bam_counters()
    assert c1["host"] == c0["host"] + 2 and c1["device"] == c0["device"]
    assert got == want == _padded(b"".join(r + b"\n" for r in bs.kept_reads(Q)))
    assert (n_masked, n_noq) == (bs.masked(Q), bs.no_qual())


GENERAL = [("fq_wrap", None), ("fq4_crlf", None), ("fq4_at", "fa_wrap"), ("fq_plus_name", "fa1"), ("fq_blank_tail", None)]


@pytest.mark.parametrize("kind,kind2", GENERAL)
def test_general_grammar_and_streaming(L, sample, kind, kind2, tmp_path, monkeypatch):
    """Wrapped records, CRLF, a FASTQ + FASTA pair (the FASTA untouched), a blank tail -- with a record of 6000 bases among them:
    the resident set (small files: the streaming reader inside ss_reads_load), the reader's own blocks with a buffer shorter than
    that record, and the streamed scan (SS_INGEST=sequential) against the oracle on mask(X)."""
    rs = np.random.RandomState(len(kind) + 7)
    fq = sample["fq"]
    recs = [(b"r%d" % i, r) for i, r in enumerate(fq.reads[:600])]
    recs.insert(100, (b"long", b"".join(fq.reads[1000:1040])))
    recs.insert(200, (b"empty", b""))
    parts = [recs] if kind2 is None else [recs[0::2], recs[1::2]]
    q = 3                                            # (fmt_render's qualities are uniform in 33..73)
    paths, masked_paths, blobs, want_n = [], [], [], 0
    for i, (part, k) in enumerate(zip(parts, (kind, kind2))):
        blob = sf.fmt_render(part, k, rs)
        c = [0]
        m = qm.mask_fastx(blob, q, c)
        want_n += c[0]
        assert (m != blob) == k.startswith("fq")
        for name, data, lst in (("x%d.%s" % (i, k[:2]), blob, paths), ("m%d.%s" % (i, k[:2]), m, masked_paths)):
            (tmp_path / name).write_bytes(data)
            lst.append(str(tmp_path / name))
        blobs.append(blob)
    assert want_n > 0
    got, info, n_masked, _, _ = _load(L, paths, q, monkeypatch)
    want, _, _, _, _ = _load(L, masked_paths, 0, monkeypatch)
    assert records(got) == records(want) and n_masked == want_n
    if kind2 is None:
        assert got == want
    want_blocks = list(L.read_flat_blocks(masked_paths, cap=4096))
    assert max(len(b) for b, _ in want_blocks) <= 4096 and any(not b.endswith(b"\n") for b, _ in want_blocks)      # cut records
    L.set_min_base_qual(q)
    assert list(L.read_flat_blocks(paths, cap=4096)) == want_blocks
    monkeypatch.setenv("SS_INGEST", "sequential")
    db = L.KmerDB.from_text(sample["kfa"], 31, True)
    try:
        db.scan_files(paths)
        got_counts = db.counts_rows()
        L.set_min_base_qual(0)
        db.reset()
        db.scan_files(paths)
        plain_counts = db.counts_rows()
    finally:
        db.close()
    want_counts, _ = orc.jellyfish_count(sample["kfa"], [qm.mask_fastx(b, q) for b in blobs], k=31, upper=True)
    plain_want, _ = orc.jellyfish_count(sample["kfa"], blobs, k=31, upper=True)
    assert np.array_equal(got_counts, want_counts) and np.array_equal(plain_counts, plain_want)
    assert 0 < int(want_counts.sum()) < int(plain_want.sum())


# ------------------------------------------------------------------------------------------------
# 2. counts
# ------------------------------------------------------------------------------------------------
def test_counts_equal_the_oracle_on_masked_reads(L, sample, bams, monkeypatch):
    """Resident (binned, packed slabs) and streamed counts of X under Q -- text, .fastq.gz on the device, BAM -- equal the
    oracle's on mask(X, Q)."""
    fq = sample["fq"]
    want, _ = orc.jellyfish_count(sample["kfa"], [fq.text(Q)], k=31, upper=True)
    plain, _ = orc.jellyfish_count(sample["kfa"], [fq.text(0)], k=31, upper=True)
    assert 0 < int(want.sum()) < int(plain.sum())
    bam_x, _, bs = bams["plain_l6"]
    want_bam, _ = orc.jellyfish_count(sample["kfa"], [b"".join(b">r\n" + r + b"\n" for r in bs.kept_reads(Q))], k=31, upper=True)
    for name in ("SS_READS_ORDER", "SS_GZ_GPU", "SS_INGEST_THREADS", "SS_INGEST"):
        monkeypatch.delenv(name, raising=False)
    db = L.KmerDB.from_text(sample["kfa"], 31, True)
    try:
        for paths, w in (([sample[0]["x%d.fq"]], want), ([sample[0]["x%d.fq.gz"]], want), ([bam_x], want_bam)):
            L.set_min_base_qual(Q)
            db.reset()
            db.scan_files(paths)
            assert np.array_equal(db.counts_rows(), w), ("streamed", paths)
            db.reset()
            rs = L.ReadSet(paths)
            # (one block of one-length records -- a .fastq.gz or a BAM decoded on the device -- is what the binning packs; the parse
            #  threads' padded chunks of a text file never were)
            assert rs.packed_slabs() > 0 or paths[0].endswith(".fq"), "a one-length sample with masked bases stays packable"
            rs.scan_into(db)
            L.check(L.lib().ss_device_sync(), "sync")
            rs.close()
            assert np.array_equal(db.counts_rows(), w), ("resident", paths)
            L.set_min_base_qual(0)
        db.reset()
        db.scan_files([sample[0]["x%d.fq"]])
        assert np.array_equal(db.counts_rows(), plain)
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------
# 3. the whole command, 4. the caches
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid_sample(mid_dbs, tmp_path_factory):
    """M_mix of tests/scenarios_mid.py (two multi-strain clusters: layer 2 runs) with the realistic quality profile, as X and
    mask(X, Q): a text pair, a .gz pair, a BAM."""
    root = tmp_path_factory.mktemp("ss_qual_mid")
    fq = qm.requal_fastq(31, mid_dbs["reads"]["M_mix"][1])
    h = len(fq.reads) // 2
    # (a BAM stores upper-case letters, as `samtools import` writes them: the same reads, names and qualities in upper case)
    bs = qm.BamSample(32, qm.FastqSample(31, [r.upper() for r in fq.reads], fq.names), no_qual_share=0.0)
    assert all(np.array_equal(a, b) for a, b in zip(bs.fq.quals[:50], fq.quals[:50]))
    out = {"fq": fq, "root": root}
    for q in (0, Q):
        a, b = fq.text(q, 0, h), fq.text(q, h, None)
        d = {}
        for name, data in (("R1.fq", a), ("R2.fq", b), ("R1.fastq.gz", gzip.compress(a, 4)), ("R2.fastq.gz", gzip.compress(b, 4)),
                           ("s.bam", bamio.bgzf(bamio.header(), bs.records(q), level=6))):
            p = root / ("q%d_%s" % (q, name))
            p.write_bytes(data)
            d[name] = str(p)
        out[q] = d
    return out


def _files(d):
    out = {}
    for root, _, fs in os.walk(d):
        for f in fs:
            out[os.path.relpath(os.path.join(root, f), d)] = open(os.path.join(root, f), "rb").read()
    return out


def _run(main, argv):
    from strainscan_amd import db as ssdb
    ssdb.clear_cache()
    np.random.seed(sc.POISSON_SEED)
    out, err = io.StringIO(), io.StringIO()
    code = 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            code = main(argv) or 0
        except SystemExit as e:
            code = e.code or 0
    return code, out.getvalue(), err.getvalue()


INPUTS = {"text_pair": ("R1.fq", "R2.fq"), "gz_pair": ("R1.fastq.gz", "R2.fastq.gz"), "bam": ("s.bam", None)}


@pytest.mark.parametrize("kind", list(INPUTS))
def test_strainscan_q_writes_what_the_masked_sample_gives(L, kind, mid_dbs, mid_sample, tmp_path, monkeypatch):
    """`strainscan -q 20 -i X` writes the files `strainscan -i mask(X, 20)` writes, byte for byte (layer 2 included), differs from
    the run without -q, and says on stderr -- not on stdout -- what it masked."""
    from strainscan_amd import StrainScan
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    a, b = INPUTS[kind]
    db_dir = mid_dbs["DB_M"]["db_dir"]

    def argv(q, out, flag):
        d = mid_sample[q]
        return ["-i", d[a]] + (["-j", d[b]] if b else []) + ["-d", db_dir, "-o", str(tmp_path / out)] + flag

    rc_q, out_q, err_q = _run(StrainScan.main, argv(0, "with_q", ["-q", str(Q)]))
    assert L.get_min_base_qual() == Q
    rc_m, out_m, err_m = _run(StrainScan.main, argv(Q, "masked", []))
    assert L.get_min_base_qual() == 0, "a command line without -q runs unmasked"
    rc_0, out_0, _ = _run(StrainScan.main, argv(0, "plain", ["--min_base_qual", "0"]))
    assert (rc_q, rc_m, rc_0) == (0, 0, 0)
    got, want, plain = _files(tmp_path / "with_q"), _files(tmp_path / "masked"), _files(tmp_path / "plain")
    assert sorted(got) == sorted(want) and "final_report.txt" in got and any(k.endswith("StrainVote.report") for k in got)
    for rel in want:
        assert got[rel] == want[rel], (kind, rel)
    assert any(got.get(rel) != plain[rel] for rel in plain), "masking a fifth of the k-mers away must move some abundance"
    dicts = lambda t: [re.sub(r" at 0x[0-9a-f]+>", ">", ln) for ln in t.splitlines() if ln.startswith(("{", "defaultdict("))]      # noqa: E731
    assert dicts(out_q) == dicts(out_m) and dicts(out_q)
    fq = mid_sample["fq"]
    line = [ln for ln in err_q.splitlines() if ln.startswith("min_base_qual")]
    assert len(line) == 1 and "min_base_qual %d: %d bases masked of %d read" % (Q, fq.masked(Q), sum(map(len, fq.reads))) in line[0]
    assert "min_base_qual" not in err_m and "min_base_qual" not in out_q


def test_strainscan_multi_q(L, mid_dbs, mid_sample, tmp_path, monkeypatch):
    """The same for strainscan-multi with two databases."""
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbs = ["-d", mid_dbs["DB_M"]["db_dir"], "-d", "mem=" + mid_dbs["DB_Mmem"]["db_dir"]]
    rc_q, _, err_q = _run(multi_db.main, ["-i", mid_sample[0]["R1.fastq.gz"], "-j", mid_sample[0]["R2.fastq.gz"], "-o", str(tmp_path / "with_q"), "-q", str(Q)] + dbs)
    rc_m, _, _ = _run(multi_db.main, ["-i", mid_sample[Q]["R1.fastq.gz"], "-j", mid_sample[Q]["R2.fastq.gz"], "-o", str(tmp_path / "masked")] + dbs)
    rc_0, _, _ = _run(multi_db.main, ["-i", mid_sample[0]["R1.fastq.gz"], "-j", mid_sample[0]["R2.fastq.gz"], "-o", str(tmp_path / "plain")] + dbs)
    assert (rc_q, rc_m, rc_0) == (0, 0, 0)
    got, want, plain = _files(tmp_path / "with_q"), _files(tmp_path / "masked"), _files(tmp_path / "plain")
    assert sorted(got) == sorted(want) and {"DB_M/final_report.txt", "mem/final_report.txt", "databases.tsv"} <= set(got)
    for rel in want:
        assert got[rel] == want[rel], rel
    assert got["DB_M/final_report.txt"] != plain["DB_M/final_report.txt"]
    assert sum(ln.startswith("min_base_qual %d:" % Q) for ln in err_q.splitlines()) == 1


def test_caches_know_the_threshold(L, mid_dbs, mid_sample, monkeypatch):
    """One process, the same files: threshold 0, then 30, then 0 -- the tree table's counts, a layer-2 cluster table's counts and
    the identified clusters are each time those of the sample masked at that threshold (not the memoised ones of the call before)."""
    import strainscan_amd
    from strainscan_amd import Vote_Strain_L2_Lasso_new_sp as vote
    from strainscan_amd import db as ssdb
    from strainscan_amd import identify
    monkeypatch.delenv("SS_READS_ORDER", raising=False)
    fq = mid_sample["fq"]
    tdb = mid_dbs["DB_M"]["db_dir"] + "/Tree_database"
    cdir = mid_dbs["DB_M"]["db_dir"] + "/Kmer_Sets_L2/Kmer_Sets/C7"
    kfa = open(tdb + "/kmer.fa", "rb").read()
    x = (mid_sample[0]["R1.fq"], mid_sample[0]["R2.fq"])
    ssdb.clear_cache()
    seen = []
    for q in (0, 30, 0):
        strainscan_amd.set_min_base_qual(q)
        assert strainscan_amd.get_min_base_qual() == q
        mr = identify.jellyfish_count(x, tdb)
        want, valid = orc.jellyfish_count(kfa, [fq.text(q)], k=31, upper=identify._UPPER_KEYS)
        assert np.array_equal(mr.counts, want), q
        cl = vote.cluster_counts(x[0], x[1], cdir, 31)
        np.random.seed(sc.POISSON_SEED)
        with contextlib.redirect_stdout(io.StringIO()):
            res = identify.identify_cluster(x, tdb, [0.1, 0.4, 1])
        seen.append((int(want.sum()), cl.copy(), dict(res)))
    strainscan_amd.set_min_base_qual(0)
    # the cluster table against the masked FILES without a threshold
    m, h = fq, len(fq.reads) // 2
    ssdb.clear_cache()
    for q, idx in ((30, 1), (0, 0)):
        p1, p2 = mid_sample["root"] / ("c%d_1.fq" % q), mid_sample["root"] / ("c%d_2.fq" % q)
        p1.write_bytes(m.text(q, 0, h))
        p2.write_bytes(m.text(q, h, None))
        assert np.array_equal(vote.cluster_counts(str(p1), str(p2), cdir, 31), seen[idx][1]), q
    assert seen[0][0] > seen[1][0] > 0 and seen[2][0] == seen[0][0]
    assert np.array_equal(seen[0][1], seen[2][1]) and not np.array_equal(seen[0][1], seen[1][1])
    assert seen[0][2] == seen[2][2]
