"""The GENERAL binning passes of ss_reorder.hip (count_kernel, place_kernel, place_again_kernel; tile_setup / tile_round /
copy_round under them) on the cases of tests/test_binning_general_host.py -- tile, halo and table edges, long records, several
record starts in a chunk, both placing kernels in one call, the buffer's edges, the 26-bit length field, wider bins -- against
tests/binmodel.py.

Every block is uploaded between 64 sentinel bytes of valid bases, at a pointer that is 16-byte aligned, odd, or 8- but not
16-byte aligned (cycled over the cases): a kernel that takes a byte at or behind n for anything but a newline lengthens the last
record into the sentinel, one that reads in front of the block merges the sentinel into the first.  The slab read back is walked
slot by slot (binmodel.parse_slab: a wrong prefix sum, slot size, piece address or a missing pad fails there), its records must
be in ascending bins and, bin by bin, the model's multiset; order inside a bin is left to the atomics and not compared.  Counts of
a table over the binned set, over the set in file order and over the flat block agree; for the wide-bin cases with the oracle
too.  Cases A, F and I are also binned in place (ReadSet.order) from a set in file order."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import binmodel as bm
from tests.test_binning_general_host import CASES, GENOME, LARGE, case

pytestmark = pytest.mark.gpu

OFFSETS = (0, 1, 8)
PARAMS = [(name, OFFSETS[i % 3]) for i, name in enumerate(CASES)]
IN_PLACE = ("A_", "F_", "I_")


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def table(L):
    """(the table, its k-mers as FASTA): every seventh 31-mer of the cases' genome"""
    kfa = b"".join(b">1\n" + GENOME[i:i + 31].tobytes() + b"\n" for i in range(0, len(GENOME) - 31, 7))
    db = L.KmerDB.from_text(kfa, 31, True)
    yield db, kfa
    db.close()


@functools.lru_cache(maxsize=4)
def _want(block):
    return bm.expected_slab(block)


def _order_counters(L):
    out = (C.c_uint64 * 2)()
    L.check(L.lib().ss_reads_order_counters(out), "ss_reads_order_counters")
    return int(out[0]), int(out[1])


def _upload(block, o):
    """-> (the device tensor, the block's address in it): 64 + o sentinel bases, the block, 64 sentinel bases"""
    import torch
    host = np.full(64 + o + len(block) + 64, ord("A"), np.uint8)
    host[64 + o:64 + o + len(block)] = np.frombuffer(block, np.uint8)
    d = torch.from_numpy(host).cuda()
    assert d.data_ptr() % 16 == 0
    return d, d.data_ptr() + 64 + o


def _binned(L, make):
    """make() with ss_test_hook 5 and 6 off -> (what it returned, (slabs through the one-length passes, through the general ones))"""
    L.check(L.lib().ss_test_hook(6, 0), "ss_test_hook")
    L.check(L.lib().ss_test_hook(5, 0), "ss_test_hook")
    try:
        f0, g0 = _order_counters(L)
        out = make()
        f1, g1 = _order_counters(L)
    finally:
        L.lib().ss_test_hook(6, 0)
        L.lib().ss_test_hook(5, 0)
    L.check(L.lib().ss_device_sync(), "sync")
    return out, (f1 - f0, g1 - g0)


def _check_slab(rset, block):
    """The binned set against the model of `block`, the bytes it was binned from."""
    want = _want(block)
    bits = bm.order_bits(len(block))
    assert rset.info()["n_records"] == want["n_records"]
    assert rset.packed_slabs() == 0
    slab = rset.read_back()
    assert len(slab) == want["slab_len"]
    recs = bm.parse_slab(slab, want["total"])
    assert len(recs) == want["n_records"]
    lengths = np.array([len(r) for r in recs], np.int64)
    starts = np.cumsum((lengths + 1 + 7) & ~7) - ((lengths + 1 + 7) & ~7)
    bins = bm.bins_at(np.frombuffer(slab, np.uint8), starts, lengths, bits)
    for r in want["by_rule"]:                                   # (start + 32 > n: in the last bin whatever its bases say)
        hit = [i for i in np.flatnonzero(lengths == len(r)).tolist() if recs[i] == r]
        assert hit, "the block's last record is not in the slab"
        bins[hit[-1]] = 1 << bits
    assert (np.diff(bins) >= 0).all(), "bins not ascending"
    got = {}
    for b, r in zip(bins.tolist(), recs):
        got.setdefault(b, []).append(r)
    assert got.keys() == want["per_bin"].keys()
    for b in got:
        assert sorted(got[b]) == want["per_bin"][b], b


def _counts(L, db, rset):
    db.reset()
    rset.scan_into(db)
    L.check(L.lib().ss_device_sync(), "sync")
    return db.counts_rows().copy()


@pytest.mark.parametrize("name,o", PARAMS)
def test_general_passes_against_the_model(L, table, name, o):
    db, kfa = table
    block, _ = case(name)
    n = len(block)
    d, ptr = _upload(block, o)
    rset, used = _binned(L, lambda: L.ReadSet.from_flat_dev(ptr, n, order=True))
    try:
        assert used == (0, 1)
        _check_slab(rset, block)
        if name not in LARGE:
            db.reset()
            db.scan_flat(block)
            flat = db.counts_rows().copy()
            assert np.array_equal(_counts(L, db, rset), flat)
            plain = L.ReadSet.from_flat_dev(ptr, n, order=False)
            try:
                assert np.array_equal(_counts(L, db, plain), flat)
            finally:
                plain.close()
            if name.startswith("I_"):
                from oracle import oracle as orc
                fq = b"".join(b"@r\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for r in block.split(b"\n") if r)
                assert np.array_equal(flat, orc.jellyfish_count(kfa, [fq], k=31, upper=True)[0]) and flat.sum() > 100000
    finally:
        rset.close()
    if name.startswith(IN_PLACE):
        # a set in file order holds the block padded with newlines to a multiple of 16 (one at least): that is what is binned
        padded = block + b"\n" * (((n + 1 + 15) & ~15) - n)
        plain = L.ReadSet.from_flat_dev(ptr, n, order=False)
        try:
            assert plain.read_back() == padded
            same, used = _binned(L, plain.order)
            assert same is plain and used == (0, 1)
            _check_slab(plain, padded)
            assert np.array_equal(_counts(L, db, plain), flat)
        finally:
            plain.close()
    del d
