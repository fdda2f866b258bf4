"""Every rung of the input ladder, through both entry points that climb it.

ss_scan_files_shard streams the base blocks of a list of inputs into a table; ss_reads_load keeps them as a resident read
set.  Both send an input down the same ladder: BAM (BGZF on the device, raw on the host), .gz on the device, .gz inflated on
the host and parsed as text, the chunked parse of a plain file of 4 MB and more, the sequential reader for everything else.
For every rung the counts through `scan_files` equal the counts through `ReadSet(...).scan_into`, and both equal
`db.scan_flat` over the sequences themselves, which knows nothing of files; the record and base totals agree; a CRAM and a
NULL path are refused by both with SS_EINVAL.  The calls go to the C ABI directly so that "" and NULL reach the library."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from tests import bamio
from tests import synth

pytestmark = pytest.mark.gpu

K = 31
# The base totals may differ by the k - 1 bases the reader re-emits for every record it cuts (tests/test_scan_gpu.py allows
# the same).  It cuts a record only where the record is longer than a 32 MB block; no record here is, so the allowance is 0.
CUT_SLACK = 0


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _genome_and_table(seed, n_sites=60000):
    rs = np.random.RandomState(seed)
    g = synth.rand_seq(rs, n_sites + 5000)
    kms = [g[i:i + K] for i in range(0, n_sites, 2)]
    return g, b"".join(b">1\n" + km + b"\n>1\n" + synth.revcomp(km) + b"\n" for km in kms)


def _reads(g, seed, n, ragged=True):
    """n reads of the genome: both strands, a few substitutions, a few 'N'; ragged lengths (some below k) or 150."""
    rs = np.random.RandomState(seed)
    ga = np.frombuffer(g, np.uint8)
    lut = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for s in rs.randint(0, len(g) - 150, size=n):
        r = ga[s:s + (rs.randint(20, 151) if ragged else 150)].copy()
        m = rs.random_sample(r.size) < 0.01
        r[m] = lut[rs.randint(0, 4, size=int(m.sum()))]
        b = r.tobytes()
        if rs.random_sample() < 0.5:
            b = synth.revcomp(b)
        if rs.random_sample() < 0.03:
            b = b[:len(b) // 2] + b"N" + b[len(b) // 2 + 1:]
        out.append(b)
    return out


def _fastq(seqs, tag=b"r"):
    return b"".join(b"@%s%d x\n%s\n+\n%s\n" % (tag, i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def _fasta_multiline(seqs, width=60):
    return b"".join(b">s%d\n" % i + b"".join(s[o:o + width] + b"\n" for o in range(0, len(s), width)) for i, s in enumerate(seqs))


def _bam_records(seqs):
    rs = np.random.RandomState(3)
    return [bamio.record("q%d" % i, s.decode(), qual=rs.randint(2, 41, size=len(s)).astype(np.uint8).tobytes())
            for i, s in enumerate(seqs)]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """name -> (paths as handed to the library, the sequences they hold); "kfa": the table's k-mers."""
    root = tmp_path_factory.mktemp("ss_ladder")
    g, kfa = _genome_and_table(29)
    text_seqs = _reads(g, 1, 30000) * 3                 # ~16 MB of FASTQ: several parse chunks
    small_seqs = _reads(g, 2, 3000)
    fasta_seqs = _reads(g, 3, 8000, ragged=False)
    gz_seqs = _reads(g, 4, 40000)
    bam_seqs = _reads(g, 5, 30000)
    raw_seqs = _reads(g, 6, 20000)

    def put(name, blob):
        p = root / name
        p.write_bytes(blob)
        return str(p)

    big = put("big.fq", _fastq(text_seqs))
    small = put("small.fq", _fastq(small_seqs))
    fasta = put("multi.fa", _fasta_multiline(fasta_seqs))
    gz = put("reads.fastq.gz", gzip.compress(_fastq(gz_seqs, b"g"), 6))
    bam = put("reads.bam", bamio.bgzf(bamio.header(), _bam_records(bam_seqs), level=6))
    raw = put("raw.bam", bamio.header() + b"".join(_bam_records(raw_seqs)))
    cram = put("s.cram", b"CRAM\3\0" + b"\0" * 64)
    assert os.path.getsize(big) >= 4 << 20 and os.path.getsize(small) < 4 << 20 and os.path.getsize(fasta) < 4 << 20
    assert os.path.getsize(gz) >= 1 << 20 and os.path.getsize(bam) >= 1 << 20      # what the device decoders take
    return {
        "kfa": kfa, "cram": cram, "small_path": small,
        "chunked_fastq": ([big], text_seqs),
        "small_fastq": ([small], small_seqs),
        "multiline_fasta": ([fasta], fasta_seqs),
        "gz": ([gz], gz_seqs),
        "bgzf_bam": ([bam], bam_seqs),
        "raw_bam": ([raw], raw_seqs),
        "pair_with_empty_mate": ([big, ""], text_seqs),
        "mixed": ([bam, gz, big], bam_seqs + gz_seqs + text_seqs),
    }


def _c_paths(paths):
    return (C.c_char_p * len(paths))(*[None if p is None else os.fsencode(p) for p in paths])


def _scan_files(L, db, paths, rank=0, world=1):
    """ss_scan_files_shard -> (code, n_records, n_bases)"""
    nrec, nb = C.c_uint64(), C.c_uint64()
    rc = L.lib().ss_scan_files_shard(db.handle, _c_paths(paths), len(paths), rank, world, C.byref(nrec), C.byref(nb))
    return rc, nrec.value, nb.value


def _load_and_scan(L, db, paths, rank=0, world=1):
    """ss_reads_load, then ss_scan_reads of the set into db -> (code, n_records, n_bases)"""
    h = C.c_void_p()
    rc = L.lib().ss_reads_load(_c_paths(paths), len(paths), rank, world, C.byref(h))
    if rc != L.SS_OK:
        return rc, 0, 0
    try:
        nrec, nb = C.c_uint64(), C.c_uint64()
        L.check(L.lib().ss_reads_info(h, C.byref(nrec), C.byref(nb), None, None), "ss_reads_info")
        L.check(L.lib().ss_scan_reads(db.handle, h, None), "ss_scan_reads")
        L.check(L.lib().ss_device_sync(), "ss_device_sync")
    finally:
        L.lib().ss_reads_destroy(h)
    return rc, nrec.value, nb.value


def _launches(L, db):
    return int(L.lib().ss_scan_kernel_launches(db.handle))


def _gz_device_files(L):
    a, b = C.c_uint64(), C.c_uint64()
    L.check(L.lib().ss_gz_gpu_counters(C.byref(a), C.byref(b)), "ss_gz_gpu_counters")
    return int(a.value)


def _both_entry_points(L, db, paths, world=1):
    """Counts and totals of `paths` through each entry point, the ranks of a sharded run added up."""
    out = {}
    for name, fn in (("scan_files", _scan_files), ("read_set", _load_and_scan)):
        counts, nrec, nb, launches = np.zeros(db.n_rows, np.uint64), 0, 0, 0
        for rank in range(world):
            db.reset()
            l0 = _launches(L, db)
            rc, r, b = fn(L, db, paths, rank, world)
            assert rc == L.SS_OK, (name, paths, rank, rc)
            launches += _launches(L, db) - l0
            counts += db.counts_rows()
            nrec += r
            nb += b
        out[name] = (counts, nrec, nb, launches)
    return out


CASES = [("chunked_fastq", 0, 1), ("small_fastq", 0, 1), ("multiline_fasta", 0, 1), ("gz", 0, 1), ("gz", 2, 1),
         ("bgzf_bam", 0, 1), ("raw_bam", 0, 1), ("pair_with_empty_mate", 0, 1), ("mixed", 0, 1), ("mixed", 0, 3)]


@pytest.mark.parametrize("name,policy,world", CASES, ids=["%s-policy%d-world%d" % c for c in CASES])
def test_counts_and_totals_equal_through_both_entry_points(L, inputs, name, policy, world, monkeypatch):
    for v in ("SS_GZ_GPU", "SS_INGEST", "SS_READS_ORDER"):
        monkeypatch.delenv(v, raising=False)
    paths, seqs = inputs[name]
    flat = b"".join(s + b"\n" for s in seqs)
    db = L.KmerDB.from_text(inputs["kfa"], K, True)
    try:
        db.scan_flat(flat)                       # the expectation: no file, no ladder
        want = db.counts_rows().astype(np.uint64)
        assert int(want.sum()) > 1000
        gz0, bam0 = _gz_device_files(L), L.bam_counters()
        with L.gz_policy(policy):
            got = _both_entry_points(L, db, paths, world)
        gz1, bam1 = _gz_device_files(L), L.bam_counters()
        # the rung the case is here for was the one taken, by both entry points and every rank
        if name in ("chunked_fastq", "pair_with_empty_mate"):
            # the chunked parse scans every 8 MB chunk of the text on its own; the reader would have made one 32 MB block of it
            assert got["scan_files"][3] >= 2, got["scan_files"][3]
        if name == "small_fastq":
            assert got["scan_files"][3] == 1, got["scan_files"][3]
        if name == "gz":
            assert gz1 - gz0 == (0 if policy == 2 else 2), (gz0, gz1)
        if name == "bgzf_bam":
            assert (bam1["device"] - bam0["device"], bam1["host"] - bam0["host"]) == (2, 0), (bam0, bam1)
        if name == "raw_bam":
            assert (bam1["device"] - bam0["device"], bam1["host"] - bam0["host"]) == (0, 2), (bam0, bam1)
        if name == "mixed":
            assert (bam1["device"] - bam0["device"], bam1["host"] - bam0["host"]) == (2 * world, 0), (bam0, bam1)
        for entry, (counts, nrec, nb, _) in got.items():
            print("%s %s policy %d world %d: %d records, %d bases (the sequences: %d, %d), %d hits (%d)"
                  % (name, entry, policy, world, nrec, nb, len(seqs), len(flat), int(counts.sum()), int(want.sum())))
            assert np.array_equal(counts, want), (name, entry)
            assert nrec == len(seqs), (name, entry)
            assert abs(nb - len(flat)) <= CUT_SLACK, (name, entry, nb, len(flat))
        assert np.array_equal(got["scan_files"][0], got["read_set"][0])
        assert got["scan_files"][1] == got["read_set"][1]
        assert abs(got["scan_files"][2] - got["read_set"][2]) <= CUT_SLACK
    finally:
        db.close()


@pytest.mark.parametrize("bad", ["cram", "null"])
def test_cram_and_null_path_are_refused_by_both_entry_points(L, inputs, bad, monkeypatch):
    for v in ("SS_GZ_GPU", "SS_INGEST"):
        monkeypatch.delenv(v, raising=False)
    good = inputs["small_path"]
    db = L.KmerDB.from_text(inputs["kfa"], K, True)
    try:
        for paths in ([inputs["cram"]], [good, inputs["cram"]]) if bad == "cram" else ([None], [good, None], [None, good]):
            assert _scan_files(L, db, paths)[0] == L.SS_EINVAL, paths
            assert _load_and_scan(L, db, paths)[0] == L.SS_EINVAL, paths
        # ... and the process goes on: the good file alone still counts
        db.reset()
        rc, nrec, _ = _scan_files(L, db, [good])
        assert rc == L.SS_OK and nrec == len(inputs["small_fastq"][1])
    finally:
        db.close()
