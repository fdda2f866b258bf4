"""The sorted binning of records of one length through a packed file-order intermediate (ss_reorder.hip pack_key_fixed_kernel,
the radix sort, gather_packed_kernel): the pack pass reads the ASCII slab once -- checks, keys, encodes -- and leaves record i
packed at i x Rt (Rt = the packed record's R bytes rounded up to 16); the gather moves those records into bin order at stride R.
The binned slab is what the ASCII gather made before: the records stable-sorted by bin, byte for byte.

The model here is vectorised (numpy), so the slabs that take the intermediate through both of its homes -- the unused tail of
a large packed slab's block, and the call's scratch -- are checked in full as well."""
import ctypes as C

import numpy as np
import pytest

from tests.binmodel import order_bits as _order_bits, slot_of as _slot

pytestmark = pytest.mark.gpu

BIG_KEEP_MIN = 256 << 20          # ss_common.h


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def genome():
    return np.frombuffer(b"ACGT", np.uint8)[np.random.RandomState(2024).randint(0, 4, size=400000)]


@pytest.fixture(scope="module")
def db(L, genome):
    kfa = b"".join(b">1\n" + genome[i:i + 31].tobytes() + b"\n" for i in range(0, 60000, 5))
    d = L.KmerDB.from_text(kfa, 31, True)
    yield d
    d.close()


_CODE = np.full(256, 255, np.uint8)
for _c, _v in ((65, 0), (67, 1), (84, 2), (71, 3)):
    _CODE[_c] = _v
    _CODE[_c | 0x20] = _v


def _bins(arr, bits, k=31, m=15):
    """record_bin of every row of arr (n x length, ASCII): top `bits` bits of mix30 of the minimizer of the first 31 bases
    (leftmost on ties), 1 << bits for a row whose first k-mer holds anything but a base of either case."""
    n, length = arr.shape
    if length < k:
        return np.full(n, 1 << bits, np.int64)
    codes = _CODE[arr[:, :k]]
    bad = (codes == 255).any(axis=1)
    km = np.zeros(n, np.uint64)
    for j in range(k):
        km |= (codes[:, j] & 3).astype(np.uint64) << np.uint64(2 * j)
    best = np.full(n, np.iinfo(np.uint64).max, np.uint64)
    for i in range(k - m + 1):
        x = (km >> np.uint64(2 * i)) & np.uint64(0x3FFFFFFF)
        h = (((x & np.uint64(0xFFFFFF)) * np.uint64(0x4F1BB << 5) + np.uint64(0x7F4A7C00)) & np.uint64(0xFFFFFFFF)) & ~np.uint64(31)
        best = np.minimum(best, h | np.uint64(i))
    pos = best & np.uint64(31)
    M30 = np.uint64(0x3FFFFFFF)
    h = (((km >> (np.uint64(2) * pos)) & M30) * np.uint64(0x9E3779B1)) & M30
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & M30
    h ^= h >> np.uint64(14)
    out = (h >> np.uint64(30 - bits)).astype(np.int64)
    out[bad] = 1 << bits
    return out


def _reads(genome, seed, length, n_rec):
    """n_rec reads of `length` bases cut from the genome's head (so that the table's k-mers are hit), with repeats (several
    reads per bin) and an N in some."""
    rs = np.random.RandomState(seed)
    starts = rs.randint(0, 62000, size=n_rec)
    arr = np.lib.stride_tricks.sliding_window_view(genome, length)[starts].copy()
    arr[3::97, rs.randint(0, length)] = ord("N")
    arr[7::211, rs.randint(0, min(31, length))] = ord("N")
    return arr


def _block(arr, pad=0):
    """The flat block of the rows of arr: each followed by a newline, `pad` more behind the last (and up to the 64 bytes below
    which nothing is taken for records of one length)."""
    n, length = arr.shape
    flat = np.full((n, length + 1), 10, np.uint8)
    flat[:, :length] = arr
    out = np.concatenate([flat.reshape(-1), np.full(pad, 10, np.uint8)])
    if out.size < 64:
        out = np.concatenate([out, np.full(64 - out.size, 10, np.uint8)])
    assert out.size - n * (length + 1) < 64
    return out


def _model(arr, n_bytes):
    """The binned slab as read_back() gives it: the rows stable-sorted by bin, each in its slot, newlines up to a multiple of 16."""
    n, length = arr.shape
    order = np.argsort(_bins(arr, _order_bits(n_bytes)), kind="stable")
    slots = np.full((n, _slot(length)), 10, np.uint8)
    slots[:, :length] = arr[order]
    flat = slots.reshape(-1)
    cap = max((flat.size + 15) & ~15, 16)
    return np.concatenate([flat, np.full(cap - flat.size, 10, np.uint8)])


def _order_counters(L):
    out = (C.c_uint64 * 2)()
    L.check(L.lib().ss_reads_order_counters(out), "ss_reads_order_counters")
    return int(out[0]), int(out[1])


class _Binned:
    """One block on the device, binned: the read set, which passes ran, and the flat scan's counts of the same block."""
    def __init__(self, L, db, block, hook6=0, want_counts=True):
        import torch
        self.L, self.db = L, db
        self.d = torch.from_numpy(block).cuda()
        self.want = None
        if want_counts:
            db.reset()
            db.scan_flat_dev(self.d.data_ptr(), self.d.numel())
            L.check(L.lib().ss_device_sync(), "sync")
            self.want = db.counts_rows().copy()
        L.check(L.lib().ss_test_hook(6, hook6), "ss_test_hook")
        try:
            f0, g0 = _order_counters(L)
            self.rset = L.ReadSet.from_flat_dev(self.d.data_ptr(), self.d.numel(), order=True)
            f1, g1 = _order_counters(L)
        finally:
            L.lib().ss_test_hook(6, 0)
        L.check(L.lib().ss_device_sync(), "sync")
        self.used = (f1 - f0, g1 - g0)

    def counts(self):
        self.db.reset()
        self.rset.scan_into(self.db)
        self.L.check(self.L.lib().ss_device_sync(), "sync")
        return self.db.counts_rows().copy()

    def back(self):
        return np.frombuffer(self.rset.read_back(), np.uint8)

    def close(self):
        self.rset.close()
        del self.d


def _check_packed(L, db, arr, pad=0, what=None):
    """The product's path on the rows of arr: one-length passes, a packed slab, read_back() = the model, counts = scan_flat's."""
    block = _block(arr, pad)
    b = _Binned(L, db, block)
    try:
        assert b.used == (1, 0), (what, b.used)
        assert b.rset.packed_slabs() == 1, what
        got, want = b.back(), _model(arr, block.size)
        assert got.size == want.size and np.array_equal(got, want), (what, int(np.argmax(got != want)) if got.size == want.size else got.size)
        assert np.array_equal(b.counts(), b.want), what
    finally:
        b.close()


LENGTHS = [32, 33, 40, 47, 150, 151, 250, 1023]      # R = 15 15 18 18 57 57 96 384: 96 and 384 are multiples of 16;
                                                     # slots of 8 x odd positions: 32 33 150 151, 8 x even: 40 47 250 1023


@pytest.mark.parametrize("length", LENGTHS)
def test_pack_layout_at_every_record_count(L, db, genome, length):
    """Record counts of 1, 63, 64, 65, 129 (a last wave of one record behind two full ones), 257 (one record in a second
    workgroup) and 1300 (several rounds per wave at 1023 bases, a partial last wave)."""
    for n_rec in (1, 63, 64, 65, 129, 257, 1300):
        _check_packed(L, db, _reads(genome, length * 7 + n_rec, length, n_rec), what=(length, n_rec))


@pytest.mark.parametrize("length,n_rec", [(150, 65), (33, 129)])
def test_newline_padding_behind_the_last_record(L, db, genome, length, n_rec):
    """0 to 63 newline bytes behind the last record (fewer than a record's L + 1 bytes: from there on the byte count says one
    record more): the slab is of one length with every one of them."""
    arr = _reads(genome, 5 + length, length, n_rec)
    for pad in range(min(64, length + 1)):
        _check_packed(L, db, arr, pad=pad, what=(length, pad))


@pytest.mark.parametrize("length", [150, 33, 40])
def test_an_n_at_the_edges_of_pieces_and_of_the_first_kmer(L, db, genome, length):
    """An N at position 0, 7, 8, 15, 16, at the last position of the first k-mer (30), behind it (31) and at L - 1, each in records
    of its own, first and last record among them."""
    arr = _reads(genome, 11 + length, length, 700)
    arr[arr == ord("N")] = ord("A")
    for j, pos in enumerate((0, 7, 8, 15, 16, 30, 31, length - 1)):
        arr[j::41, pos] = ord("N")
    arr[-1, length - 1] = ord("N")
    assert arr[0, 0] == ord("N")
    _check_packed(L, db, arr, what=length)


def _check_ascii(L, db, arr, what):
    block = _block(arr)
    b = _Binned(L, db, block)
    try:
        assert b.used == (1, 0), (what, b.used)
        assert b.rset.packed_slabs() == 0, what
        assert np.array_equal(b.back(), _model(arr, block.size)), what
        assert np.array_equal(b.counts(), b.want), what
    finally:
        b.close()


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("byte", ["a", "\r"])
def test_a_byte_outside_the_alphabet_in_one_record_only(L, db, genome, where, byte):
    """One lower-case base, or one carriage return, in the first record only / in the last record only (a last wave of 40 records,
    the last workgroup): an ASCII slab in the model's order."""
    arr = _reads(genome, 19, 150, 9000 + 40)
    row, col = (0, 77) if where == "first" else (arr.shape[0] - 1, 149)
    arr[row, col] = ord(byte) if byte != "a" else (arr[row, col] | 0x20 if arr[row, col] != ord("N") else ord("a"))
    _check_ascii(L, db, arr, (where, byte))


def test_a_lower_case_base_inside_the_first_kmer(L, db, genome):
    """The key is case-insensitive (the record keeps its bin) and the slab stays ASCII."""
    arr = _reads(genome, 23, 150, 5000)
    arr[2500, :31] = genome[100:131]
    arr[2500, 12] |= 0x20
    bits = _order_bits(5000 * 151)
    upper = arr[2500:2501].copy()
    upper[0, 12] &= 0xDF
    assert _bins(arr[2500:2501], bits)[0] == _bins(upper, bits)[0] != 1 << bits
    _check_ascii(L, db, arr, "lower case in the first k-mer")


@pytest.mark.parametrize("variant", ["inner_newline", "last_newline_missing", "one_base_short"])
def test_not_of_one_length_is_seen_by_the_pack_pass(L, db, genome, variant):
    """One newline inside a middle record (the byte count still divides), a base where the last record's newline belongs, and one
    record a base short (a later one a base long): the general passes run -- ss_reads_order_counters says so -- and the counts
    are the flat scan's."""
    arr = _reads(genome, 29, 150, 9000)
    flat = _block(arr).copy()
    if variant == "inner_newline":
        flat[4000 * 151 + 75] = 10
    elif variant == "last_newline_missing":
        flat[-1] = ord("A")
    else:
        rows = [r.tobytes() for r in arr]
        rows[2500] = rows[2500][:-1]
        rows[6000] = rows[6000] + b"A"
        flat = np.frombuffer(b"\n".join(rows) + b"\n", np.uint8).copy()
    assert flat.size == 9000 * 151 and flat[150] == 10
    b = _Binned(L, db, flat)
    try:
        assert b.used == (0, 1), (variant, b.used)
        assert b.rset.packed_slabs() == 0
        assert np.array_equal(b.counts(), b.want)
        recs = sorted(r for r in flat.tobytes().split(b"\n") if r)
        assert sorted(r for r in b.back().tobytes().split(b"\n") if r) == recs
    finally:
        b.close()


def _plan_in_slab(length, n_rec):
    """PackPlan of ss_reorder.hip: whether the intermediate lies in the new slab's block."""
    slot = _slot(length)
    cap = max((n_rec * slot + 15) & ~15, 16)
    rt = (slot // 8 * 3 + 15) & ~15
    used = (cap >> 4) * 6 + 8
    block = max(used, cap if cap >= BIG_KEEP_MIN else 0)
    return ((used + 255) & ~255) + n_rec * rt <= block, cap >= BIG_KEEP_MIN


@pytest.mark.parametrize("length,n_rec,home", [(150, 1_800_000, "tail"), (150, 3000, "scratch"), (44, 5_700_000, "scratch_large")])
def test_both_homes_of_the_intermediate(L, db, genome, length, n_rec, home):
    """A slab just above BIG_KEEP_MIN (1.8 M x 150 bases, 272 MB): the intermediate lies behind the packed slab in its block;
    one far below: in the scratch; 5.7 M x 44 bases (slot 48: R = 18, Rt = 32, and 18 + 32 > 48): the block is large and the
    intermediate does not fit, the scratch holds it.  Then a small slab in the same process, with the scratch kept from this."""
    in_slab, large = _plan_in_slab(length, n_rec)
    assert (in_slab, large) == {"tail": (True, True), "scratch": (False, False), "scratch_large": (False, True)}[home]
    rs = np.random.RandomState(n_rec)
    starts = rs.randint(0, len(genome) - length, size=n_rec)
    arr = np.lib.stride_tricks.sliding_window_view(genome, length)[starts]
    arr[5::1001, 40] = ord("N")
    _check_packed(L, db, arr, what=home)
    _check_packed(L, db, _reads(genome, 3, 150, 2000), what=(home, "small slab afterwards"))


def _rows_by_bin(back, length, n_rec, bits):
    """The records of a binned slab as rows, their bins, and the order that sorts them by (bin, a hash of the row)."""
    rows = back[:n_rec * _slot(length)].reshape(n_rec, _slot(length))
    bins = _bins(rows[:, :length], bits)
    words = np.ascontiguousarray(rows).view(np.uint64)              # (slots are multiples of 8 bytes)
    w = np.random.RandomState(1).randint(1, 1 << 62, size=words.shape[1]).astype(np.uint64) | np.uint64(1)
    hsh = (words * w[None, :]).sum(axis=1, dtype=np.uint64)
    return rows, bins, np.lexsort((hsh, bins))


@pytest.mark.parametrize("length,n_rec", [(32, 65), (33, 64), (40, 257), (47, 1300), (150, 1), (150, 63), (150, 30001), (151, 4097),
                                          (250, 1300), (1023, 700), (150, 1_800_000)])
def test_the_count_and_atomic_placement_agrees(L, db, genome, length, n_rec):
    """ss_test_hook 6 = 1 (count_fixed + place_fixed_packed, untouched) against 0: the same records in every bin, the same counts."""
    rs = np.random.RandomState(length + n_rec)
    arr = np.lib.stride_tricks.sliding_window_view(genome, length)[rs.randint(0, 62000, size=n_rec)].copy()
    arr[3::97, length // 2] = ord("N")
    block = _block(arr)
    bits = _order_bits(block.size)
    got = {}
    for hook in (1, 0):
        b = _Binned(L, db, block, hook6=hook, want_counts=False)
        try:
            assert b.used == (1, 0) and b.rset.packed_slabs() == 1, (hook, b.used)
            got[hook] = (b.counts(), b.back())
        finally:
            b.close()
    assert np.array_equal(got[0][0], got[1][0])
    assert got[0][1].size == got[1][1].size
    r0, b0, o0 = _rows_by_bin(got[0][1], length, n_rec, bits)
    r1, b1, o1 = _rows_by_bin(got[1][1], length, n_rec, bits)
    assert np.all(np.diff(b0) >= 0) and np.all(np.diff(b1) >= 0)
    assert np.array_equal(b0, b1)
    assert np.array_equal(r0[o0], r1[o1])
