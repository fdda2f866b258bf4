"""Packed binned slabs (ss_reorder.hip place_fixed_packed_kernel, ss_scan_dev.h IN_PACKED): a read set of one-length records
whose every byte is A C G T or N is held as 2-bit codes + invalid flags, 3 bytes per 8 positions.  Every scan kernel reads it
as it is; the counts must equal, bit for bit, those over the same set kept ASCII (ss_test_hook 5 = 1) and those of the flat
scan of the block in file order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _bin(rec, bits, k=31, m=15):
    """Bin of a record (ss_reorder.hip record_bin): top `bits` bits of mix30 of the minimizer of its first 31 bases."""
    code = {65: 0, 67: 1, 84: 2, 71: 3}
    if len(rec) < k:
        return 1 << bits
    cs = [code.get(c & 0xDF, -1) for c in rec[:k]]
    if min(cs) < 0:
        return 1 << bits
    km = sum(c << (2 * j) for j, c in enumerate(cs))
    best, bx = None, 0
    for i in range(k - m + 1):
        x = (km >> (2 * i)) & 0x3FFFFFFF
        h = (((x & 0xFFFFFF) * (0x4F1BB << 5) + 0x7F4A7C00) & 0xFFFFFFFF) & ~31
        if best is None or h < best:
            best, bx = h, x
    M30 = 0x3FFFFFFF
    h = (bx * 0x9E3779B1) & M30
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & M30
    h ^= h >> 14
    return h >> (30 - bits)


def _order_bits(n_bytes):
    bits = 12
    while bits < 22 and (n_bytes // 152) >> (bits + 2):
        bits += 1
    return bits


def _kfa(g, k, step):
    return b"".join(b">1\n" + g[i:i + k] + b"\n" for i in range(0, len(g) - k, step))


def _reads(seed, length, n_rec, g):
    """n_rec reads of `length` bases cut from g; N inside some of them, and inside the first 31 bases of others."""
    rs = np.random.RandomState(seed)
    ga = np.frombuffer(g, np.uint8)
    starts = rs.randint(0, len(g) - length, size=n_rec)
    arr = ga[starts[:, None] + np.arange(length)[None, :]].copy()
    arr[::97, :][np.arange(len(arr[::97])), rs.randint(0, length, size=len(arr[::97]))] = ord("N")
    sub = arr[3::101]
    sub[np.arange(len(sub)), rs.randint(0, 31, size=len(sub))] = ord("N")
    arr[3::101] = sub
    return [a.tobytes() for a in arr]


def _read_set(L, block, ascii_slabs):
    import torch
    d = torch.frombuffer(bytearray(block), dtype=torch.uint8).cuda()
    L.check(L.lib().ss_test_hook(5, 1 if ascii_slabs else 0), "ss_test_hook")
    try:
        rset = L.ReadSet.from_flat_dev(d.data_ptr(), d.numel(), order=True)
    finally:
        L.lib().ss_test_hook(5, 0)
    L.check(L.lib().ss_device_sync(), "sync")
    return rset


def _tables(L, g):
    """name -> list of tables (one pass each; 'multi' goes through ss_scan_reads_multi)."""
    t = {}
    t["k31_sampled"] = [L.KmerDB.from_text(_kfa(g, 31, 7), 31, True)]
    dense = L.KmerDB.from_text(_kfa(g[:20000], 31, 1), 31, True)
    dense.expect_hits(True)                              # binned + a table that expects hits: the combining variant
    t["k31_dense_comb"] = [dense]
    multi = []
    for j in range(3):
        db = L.KmerDB.from_text(_kfa(g[j * 9000:j * 9000 + 14000], 31, 1 + j), 31, True)
        db.expect_hits(True)
        multi.append(db)
    t["multi3"] = multi
    t["k25"] = [L.KmerDB.from_text(_kfa(g, 25, 3), 25, True)]
    k19 = L.KmerDB.from_text(_kfa(g[:30000], 19, 1), 19, True)
    k19.expect_hits(True)                                # k <= 19 and expecting hits: scan_minik_kernel
    t["k19_flagged"] = [k19]
    t["k15_flat"] = [L.KmerDB.from_text(_kfa(g, 15, 5), 15, True)]
    return t


def _counts(L, name, dbs, scan):
    for db in dbs:
        db.reset()
    scan(dbs)
    L.check(L.lib().ss_device_sync(), "sync")
    return [db.counts_rows().copy() for db in dbs]


@pytest.fixture(scope="module")
def genome_tables(L):
    rs = np.random.RandomState(2024)
    g = np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, size=70000)].tobytes()
    t = _tables(L, g)
    yield g, t
    for dbs in t.values():
        for db in dbs:
            db.close()


@pytest.mark.parametrize("length,n_rec", [(150, 20001), (32, 5003), (100, 3), (151, 4097), (250, 2000), (1023, 300)])
def test_packed_set_counts_equal_ascii_and_file_order(L, genome_tables, length, n_rec):
    g, tables = genome_tables
    recs = _reads(length * 31 + n_rec, length, n_rec, g)
    block = b"\n".join(recs) + b"\n"
    packed = _read_set(L, block, ascii_slabs=False)
    plain = _read_set(L, block, ascii_slabs=True)
    assert packed.packed_slabs() == 1 and plain.packed_slabs() == 0
    assert packed.info()["n_records"] == plain.info()["n_records"]
    assert packed.info()["device_bytes"] < plain.info()["device_bytes"]
    for name, dbs in tables.items():
        want = _counts(L, name, dbs, lambda ds: [db.scan_flat(block) for db in ds])
        if name == "multi3":
            got_p = _counts(L, name, dbs, lambda ds: packed.scan_into_many(ds))
            got_a = _counts(L, name, dbs, lambda ds: plain.scan_into_many(ds))
        else:
            got_p = _counts(L, name, dbs, lambda ds: [packed.scan_into(db) for db in ds])
            got_a = _counts(L, name, dbs, lambda ds: [plain.scan_into(db) for db in ds])
        assert n_rec < 100 or sum(int(w.sum()) for w in want) > 0, name      # (a handful of reads may miss a table)
        for w, p, a in zip(want, got_p, got_a):
            assert np.array_equal(p, a), (name, length, n_rec)
            assert np.array_equal(p, w), (name, length, n_rec)
    # read-back: the bytes of the ASCII form -- same record multiset, bins ascending, padded to 16 with '\n'
    back_p, back_a = packed.read_back(), plain.read_back()
    assert len(back_p) == len(back_a) and len(back_p) % 16 == 0 and back_p.endswith(b"\n")
    recs_p = [r for r in back_p.split(b"\n") if r]
    assert sorted(recs_p) == sorted(recs)
    assert sorted(back_p.split(b"\n")) == sorted(back_a.split(b"\n"))      # the same slots, '\n' padding included
    bins = [_bin(r, _order_bits(len(block))) for r in recs_p]
    assert bins == sorted(bins)
    packed.close()
    plain.close()


def test_packed_set_past_the_probe(L, genome_tables):
    """A set large enough for the probe of an unflagged k = 31 table (its first 8192 tiles, then the rest of the slab from
    behind them: a packed pointer offset)."""
    g, tables = genome_tables
    recs = _reads(99, 150, 240000, g)
    block = b"\n".join(recs) + b"\n"
    packed = _read_set(L, block, ascii_slabs=False)
    plain = _read_set(L, block, ascii_slabs=True)
    assert packed.packed_slabs() == 1
    db = tables["k31_sampled"][0]
    want = _counts(L, "k31", [db], lambda ds: ds[0].scan_flat(block))[0]
    got_p = _counts(L, "k31", [db], lambda ds: packed.scan_into(ds[0]))[0]
    got_a = _counts(L, "k31", [db], lambda ds: plain.scan_into(ds[0]))[0]
    assert np.array_equal(got_p, got_a) and np.array_equal(got_p, want)
    packed.close()
    plain.close()


@pytest.mark.parametrize("odd", [b"a", b"R", b"c"])
def test_one_odd_base_keeps_the_slab_ascii(L, genome_tables, odd):
    """A one-length slab with a single lower-case or IUPAC base is binned by the one-length passes but stays ASCII, and
    reads back byte for byte."""
    g, tables = genome_tables
    recs = _reads(5, 150, 3001, g)
    recs[1777] = recs[1777][:60] + odd + recs[1777][61:]
    block = b"\n".join(recs) + b"\n"
    rset = _read_set(L, block, ascii_slabs=False)
    assert rset.packed_slabs() == 0
    back = rset.read_back()
    assert sorted(r for r in back.split(b"\n") if r) == sorted(recs)
    db = tables["k31_sampled"][0]
    want = _counts(L, "k31", [db], lambda ds: ds[0].scan_flat(block))[0]
    got = _counts(L, "k31", [db], lambda ds: rset.scan_into(ds[0]))[0]
    assert np.array_equal(got, want)
    rset.close()
