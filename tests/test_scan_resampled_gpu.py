"""ss_scan_reads_resampled (ss_scan_resampled.hip, scan_minik_kernel's WeightSink): the counts of several bootstrap replicates from
one pass over a resident set.  Every vector is held, with np.array_equal, to two things: the counts of the existing route on a
second handle of the same table (resample -> reset -> scan_into -> counts_rows) and the model -- the CPU oracle counting the reads
that tests/boot_model.py's weights repeat, as tests/test_resample_gpu.py::test_scan_of_the_resampled_set builds them.  The blocks
are that file's: every length from 1 to 400, records over 1024 bytes that straddle tiles, lower case, N, '\\r', empty lines; 1, 63,
64, 65 and 4099 one-length records in file order, binned as ASCII and packed; and a set of two slabs.

Not covered here: the SS_EINVAL of a table and a set on different devices (one device)."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from tests import boot_model
from tests.test_resample_gpu import _one_length_block, _ragged_block, _rand

pytestmark = pytest.mark.gpu

SEEDS = (20, (1 << 63) - 1)
FIRSTS = (0, 5)
NS = (1, 3, 16)
KS = (31, 25)
SIZES = (1, 63, 64, 65, 4099)
LAYOUTS = ("file", "binned", "packed")
SETS = ["%s_%d" % (lay, n) for n in SIZES for lay in LAYOUTS] + ["ragged_file", "ragged_binned", "two_slabs"]


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def genome():
    return _rand(np.random.RandomState(77), 60000)


def _kfa(genome, k):
    """a few thousand k-mers, one of them listed twice (the last row owns the count) and one in lower case"""
    kmers = list(dict.fromkeys(genome[i:i + k] for i in range(0, 18000, 3)))
    kmers.insert(1000, kmers[500])
    kmers[2000] = kmers[2000].lower()
    return b"".join(b">1\n" + km + b"\n" for km in kmers)


def _build(L, kfa, k, bloom):
    old = os.environ.get("SS_BLOOM_BITS")
    os.environ["SS_BLOOM_BITS"] = "16" if bloom else "0"
    try:
        db = L.KmerDB.from_text(kfa, k, True)
    finally:
        if old is None:
            del os.environ["SS_BLOOM_BITS"]
        else:
            os.environ["SS_BLOOM_BITS"] = old
    assert db.info()["layout"] == 1 and (db.info()["filter_bits"] > 0) == bloom
    return db


@pytest.fixture(scope="module")
def tables(L, genome):
    """(k, kind) -> (table, a second handle of the same table); kind: plain, bloom (behind its filter), expect (flagged)"""
    out = {}
    for k in KS:
        kfa = _kfa(genome, k)
        for kind in ("plain", "bloom", "expect"):
            pair = tuple(_build(L, kfa, k, kind == "bloom") for _ in range(2))
            if kind == "expect":
                for db in pair:
                    db.expect_hits()
            out[(k, kind)] = pair
    yield out
    for pair in out.values():
        for db in pair:
            db.close()


def _fastq_gz(path, reads, seed):
    rs = np.random.RandomState(seed)
    qa = np.arange(33, 74, dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(gzip.compress(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, qa[rs.randint(0, qa.size, size=len(r))].tobytes())
                                       for i, r in enumerate(reads)), 1))
    assert os.path.getsize(path) >= 1 << 20
    return path


@pytest.fixture(scope="module")
def read_sets(L, genome, tmp_path_factory):
    """name -> (ReadSet, the flat bytes whose records it holds)"""
    import torch
    keep, out = [], {}

    def flat(block, order, ascii_slabs=False):
        d = torch.frombuffer(bytearray(block if block else b"\n"), dtype=torch.uint8).cuda()
        keep.append(d)
        L.check(L.lib().ss_test_hook(5, 1 if ascii_slabs else 0), "ss_test_hook")
        try:
            rset = L.ReadSet.from_flat_dev(d.data_ptr(), len(block), order=order)
        finally:
            L.lib().ss_test_hook(5, 0)
        L.check(L.lib().ss_device_sync(), "sync")
        return rset

    for n in SIZES:
        block = _one_length_block(genome, n, 100 + n)
        out["file_%d" % n] = (flat(block, False), block)
        out["binned_%d" % n] = (flat(block, True, ascii_slabs=True), block)
        out["packed_%d" % n] = (flat(block, True), block)
        assert out["packed_%d" % n][0].packed_slabs() >= 1 and out["binned_%d" % n][0].packed_slabs() == 0
    ragged = _ragged_block(genome)
    out["ragged_file"] = (flat(ragged, False), ragged)
    out["ragged_binned"] = (flat(ragged, True), ragged)
    # two .fastq.gz files of 1 MB and more: the device path gives each a slab of its own, and record indices run on across slabs
    rs = np.random.RandomState(13)
    root = str(tmp_path_factory.mktemp("rsmp_gz"))
    reads = [[genome[s:s + 1000] for s in rs.randint(0, 20000, size=1250)] for _ in range(2)]
    two = L.ReadSet([_fastq_gz(os.path.join(root, "r%d.fastq.gz" % (m + 1)), reads[m], 100 + m) for m in range(2)])
    assert two.info()["n_blocks"] >= 2
    out["two_slabs"] = (two, b"".join(r + b"\n" for m in range(2) for r in reads[m]))
    out["flat"] = flat
    yield out
    for name, v in out.items():
        if name != "flat":
            v[0].close()


_ROUTE, _MODEL = {}, {}


def _existing_route(L, db2, rset, key, seed, rep):
    """resample -> reset -> scan_into -> counts_rows on the second handle (once per table, set, seed and replicate)"""
    if key + (seed, rep) not in _ROUTE:
        sub = rset.resample(seed, rep)
        try:
            db2.reset()
            sub.scan_into(db2)
            L.check(L.lib().ss_device_sync(), "sync")
            _ROUTE[key + (seed, rep)] = db2.counts_rows().copy()
        finally:
            sub.close()
    return _ROUTE[key + (seed, rep)]


def _model(L, genome, k, sname, block, seed, rep):
    """the CPU oracle's counts of the block's records, each as often as the model's weight says"""
    from oracle import oracle as orc
    if (k, sname, seed, rep) not in _MODEL:
        recs, w = boot_model.weights(L, block, seed, rep)
        fq = b"".join((b"@r\n" + r + b"\n+\n" + b"I" * len(r) + b"\n") * int(n) for r, n in zip(recs, w.tolist()))
        _MODEL[(k, sname, seed, rep)] = orc.jellyfish_count(_kfa(genome, k), [fq], k=k, upper=True)[0]
    return _MODEL[(k, sname, seed, rep)]


def _hold_to_definition(L, genome, tables, read_sets, k, kind, sname):
    db, db2 = tables[(k, kind)]
    rset, block = read_sets[sname]
    total = 0
    for seed in SEEDS:
        for first in FIRSTS:
            for n in NS:
                calls = L.scan_resampled_calls()
                out = rset.scan_resampled(db, seed, first, n)
                try:
                    assert L.scan_resampled_calls() == calls + 1
                    assert (out.n, out.n_rows) == (n, db.n_rows)
                    for j in range(n):
                        got = out.row_vector(j)
                        assert np.array_equal(got, _existing_route(L, db2, rset, (k, kind, sname), seed, first + j)), (seed, first, n, j)
                        assert np.array_equal(got, _model(L, genome, k, sname, block, seed, first + j)), (seed, first, n, j)
                        total += int(got.sum())
                finally:
                    out.close()
    return total


@pytest.mark.parametrize("sname", SETS)
@pytest.mark.parametrize("k", KS)
def test_definition(L, genome, tables, read_sets, k, sname):
    total = _hold_to_definition(L, genome, tables, read_sets, k, "plain", sname)
    if not sname.endswith("_1"):
        assert total > 1000                                 # (the sets do hit the table)


@pytest.mark.parametrize("sname", ["packed_4099", "binned_65", "ragged_file", "two_slabs"])
@pytest.mark.parametrize("kind", ["bloom", "expect"])
@pytest.mark.parametrize("k", KS)
def test_both_filter_kinds(L, genome, tables, read_sets, k, kind, sname):
    assert _hold_to_definition(L, genome, tables, read_sets, k, kind, sname) > 1000


def test_the_duplicate_and_the_lower_case_row(L, genome, tables, read_sets):
    """the conditions on the table: the k-mer listed twice counts on its last row only, the lower-case row counts"""
    db, _ = tables[(31, "plain")]
    out = read_sets["packed_4099"][0].scan_resampled(db, 20, 0, 16)
    try:
        v = sum(out.row_vector(j).astype(np.int64) for j in range(16))
    finally:
        out.close()
    assert db.row_valid[500] == 0 and v[500] == 0 and db.row_valid[1000] == 1 and v[1000] > 0 and v[2000] > 0


def test_counters_untouched(L, tables, read_sets):
    db, _ = tables[(31, "plain")]
    for sname in ("packed_4099", "ragged_file"):
        rset = read_sets[sname][0]
        text = rset.read_back()
        db.reset()
        rset.scan_into(db)
        L.check(L.lib().ss_device_sync(), "sync")
        before = db.counts_rows().copy()
        assert before.sum() > 1000
        rset.scan_resampled(db, 20, 0, 16).close()
        assert np.array_equal(db.counts_rows(), before)
        assert rset.read_back() == text
    db.reset()


def test_edge_sets(L, genome, tables, read_sets):
    db, _ = tables[(31, "plain")]
    flat = read_sets["flat"]
    short = b"".join(genome[i:i + 30] + b"\n" for i in range(0, 3000, 30))      # every record is shorter than k
    for block in (b"", b"\n" * 40, short):
        rset = flat(block, False)
        try:
            out = rset.scan_resampled(db, 20, 0, 16)
            try:
                assert all(not out.row_vector(j).any() for j in range(16))
            finally:
                out.close()
        finally:
            rset.close()
    # identical reads share a weight: every count is a multiple of it
    read = genome[300:450]
    rset = flat((read + b"\n") * 70, True)
    try:
        out = rset.scan_resampled(db, 20, 0, 16)
        try:
            ws = [int(boot_model.weights(L, read + b"\n", 20, j)[1][0]) for j in range(16)]
            assert any(w == 0 for w in ws) and any(w >= 2 for w in ws)
            for j, w in enumerate(ws):
                v = out.row_vector(j)
                assert set(np.unique(v).tolist()) == ({0, 70 * w} if w else {0}), (j, w)
        finally:
            out.close()
    finally:
        rset.close()


def test_refusals(L, genome, tables, read_sets, tmp_path, monkeypatch):
    db, _ = tables[(31, "plain")]
    rset = read_sets["file_65"][0]
    before = L.scan_resampled_calls()
    buf = L.ReplicateCounts(17, db.n_rows)
    try:
        call = L.lib().ss_scan_reads_resampled
        assert call(db.handle, rset._h, 1, 0, 0, buf.dptr) == L.SS_EINVAL
        assert call(db.handle, rset._h, 1, 0, 17, buf.dptr) == L.SS_EINVAL
        assert call(None, rset._h, 1, 0, 1, buf.dptr) == L.SS_EINVAL
        assert call(db.handle, None, 1, 0, 1, buf.dptr) == L.SS_EINVAL
        assert call(db.handle, rset._h, 1, 0, 1, None) == L.SS_EINVAL
        assert L.lib().ss_scan_reads_resampled_calls(None) == L.SS_EINVAL
        flat_db = L.KmerDB.from_text(b"".join(b">1\n" + genome[i:i + 15] + b"\n" for i in range(0, 300, 3)), 15, True)
        try:
            assert flat_db.info()["layout"] == 0
            assert call(flat_db.handle, rset._h, 1, 0, 1, buf.dptr) == L.SS_ERANGE
        finally:
            flat_db.close()
        # a record longer than a block of the sequential reader is cut: its pieces are no reads (ss_reads_resample refuses the same set)
        p = tmp_path / "long.fa"
        p.write_bytes(b">long\n" + genome[:50000] * 700 + b"\n>short\nACGTACGTAC\n")
        monkeypatch.setenv("SS_INGEST", "sequential")
        cut = L.ReadSet([str(p)])
        try:
            with pytest.raises(L.SSError) as e:
                cut.scan_resampled(db, 1, 0, 1)
            assert e.value.code == L.SS_ERANGE
        finally:
            cut.close()
        with pytest.raises(L.SSError) as e:
            rset.scan_resampled(db, 1, 0, 17)
        assert e.value.code == L.SS_EINVAL
    finally:
        buf.close()
    assert L.scan_resampled_calls() == before
