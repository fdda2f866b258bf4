"""Binning of records of one length by sorting (ss_reorder.hip key_fixed_kernel, a stable radix sort, gather_fixed_kernel): the
binned slab holds the records in bin order and, inside a bin, in FILE order -- so two binnings of one input read back byte for
byte the same.  ss_test_hook 6 = 1 bins through the count + atomic placement instead: the same records per bin, the same counts.
Bytes other than A C G T N keep the slab ASCII; a slab that is not of one length after all takes the general passes -- from
either one-length path.  The scratch block is one allocation that each path lays out its own way and that is kept from call to
call: one process takes it through every layout."""
import ctypes as C

import numpy as np
import pytest

from tests.binmodel import bin_of as _bin, one_length_candidate as _one_length_candidate, order_bits as _order_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _order_counters(L):
    out = (C.c_uint64 * 2)()
    L.check(L.lib().ss_reads_order_counters(out), "ss_reads_order_counters")
    return int(out[0]), int(out[1])


def _genome(seed, n):
    rs = np.random.RandomState(seed)
    return np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, size=n)]


def _records(seed, length, n_rec, g, lower_first=False, mid=None):
    """n_rec reads of `length` bases cut from g (with repeats: several reads per bin); N in the first k-mer of some, N elsewhere
    in others; lower_first: lower case in the first k-mer of some; mid: a byte put in the middle of some."""
    rs = np.random.RandomState(seed)
    starts = rs.randint(0, len(g) - length, size=n_rec)
    arr = g[starts[:, None] + np.arange(length)[None, :]].copy()
    arr[7::211, rs.randint(0, min(31, length))] = ord("N")
    arr[3::97, rs.randint(0, length)] = ord("N")
    if lower_first:
        arr[5::503, :31] |= 0x20
    if mid is not None:
        arr[11::301, length // 2] = ord(mid)
    return [a.tobytes() for a in arr]


def _kdb(L, g):
    kfa = b"".join(b">1\n" + g[i:i + 31].tobytes() + b"\n" for i in range(0, len(g) - 31, 7))
    return L.KmerDB.from_text(kfa, 31, True)


def _ragged_block(seed, n_rec, g):
    """n_rec reads of 100..200 bases cut from g, some with an N: no one-length candidate (checked)."""
    rs = np.random.RandomState(seed)
    lens = rs.randint(100, 201, size=n_rec)
    starts = rs.randint(0, len(g) - 200, size=n_rec)
    recs = [g[s:s + n].tobytes() for s, n in zip(starts, lens)]
    for i in range(3, n_rec, 97):
        recs[i] = recs[i][:40] + b"N" + recs[i][41:]
    block = b"\n".join(recs) + b"\n"
    assert _one_length_candidate(block) is None
    return recs, block


def _bin_once(L, block, hook6=0, hook5=0):
    import torch
    d = torch.frombuffer(bytearray(block), dtype=torch.uint8).cuda()
    L.check(L.lib().ss_test_hook(6, hook6), "ss_test_hook")
    L.check(L.lib().ss_test_hook(5, hook5), "ss_test_hook")
    try:
        f0, g0 = _order_counters(L)
        rset = L.ReadSet.from_flat_dev(d.data_ptr(), d.numel(), order=True)
        f1, g1 = _order_counters(L)
    finally:
        L.lib().ss_test_hook(6, 0)
        L.lib().ss_test_hook(5, 0)
    L.check(L.lib().ss_device_sync(), "sync")
    return rset, (f1 - f0, g1 - g0)


def _counts(L, db, rset):
    db.reset()
    rset.scan_into(db)
    L.check(L.lib().ss_device_sync(), "sync")
    return db.counts_rows().copy()


@pytest.mark.parametrize("length,n_rec,pad,lower", [(150, 20001, 0, False), (150, 20001, 0, True), (151, 4097, 9, False), (32, 70000, 0, False),
                                                    (33, 64, 0, True), (100, 1, 0, False), (250, 12345, 3, False), (1023, 3000, 0, False),
                                                    (1023, 700, 5, True), (160, 999, 0, False), (47, 130, 0, False)])
def test_sorted_binning_keeps_file_order_inside_a_bin(L, length, n_rec, pad, lower):
    """read_back() equals the records stable-sorted by bin; a second binning reads back the same bytes; the counts equal the
    flat scan's.  Lengths 32..1023, record counts that are not multiples of 64, one record, newline padding, N / lower case in
    the first k-mer (lower case: an ASCII slab), slots of 8 x odd and 8 x even positions."""
    g = _genome(length * 3 + n_rec, 60000 + length)
    recs = _records(length + n_rec, length, n_rec, g, lower_first=lower)
    block = b"\n".join(recs) + b"\n" * (1 + pad)
    assert len(block) >= 64 or n_rec == 1
    if len(block) < 64:                                         # (one short record: below what the one-length passes take)
        block += b"\n" * (64 - len(block))
    db = _kdb(L, g)
    db.reset()
    db.scan_flat(block)
    want = db.counts_rows().copy()
    bits = _order_bits(len(block))
    bins = [_bin(r, bits) for r in recs]
    order = sorted(range(n_rec), key=lambda i: bins[i])         # (stable)
    first = None
    for rep in range(2):
        rset, used = _bin_once(L, block)
        assert used == (1, 0), (length, n_rec, used)
        assert rset.packed_slabs() == (0 if lower else 1)
        assert np.array_equal(_counts(L, db, rset), want)
        slots = rset.read_back()
        assert len(slots) % 16 == 0 and slots.endswith(b"\n")
        back = [r for r in slots.split(b"\n") if r]
        assert back == [recs[i] for i in order]
        if first is None:
            first = slots
        else:
            assert slots == first
        rset.close()
    timing = np.zeros(3)
    L.check(L.lib().ss_reads_order_timing(L.ptr(timing)), "ss_reads_order_timing")
    assert timing[0] > 0 and timing[1] >= 0 and timing[2] > 0
    db.close()


@pytest.mark.parametrize("length,n_rec,lower", [(150, 30000, False), (150, 30000, True), (77, 5001, False), (151, 4097, False),
                                                (151, 4097, True), (1023, 700, False), (1023, 700, True), (33, 64, False),
                                                (33, 64, True), (32, 65, False), (32, 65, True), (100, 1, False)])
def test_hook6_atomic_placement_agrees_with_the_sort(L, length, n_rec, lower):
    """ss_test_hook 6 = 1 (count + atomic placement) and 0 (key + sort + gather) on one input: the same records in every bin,
    the same layout, bit-identical counters after a scan.  Slots of 8 x odd positions with a partial last wave (151 x 4097),
    several LDS rounds per wave (1023), the shortest lengths with one wave and one record more, a single record; packed
    (place_fixed_packed_kernel) and, lower case in some first k-mers, ASCII (place_fixed_kernel)."""
    g = _genome(91 + length, 40000 + length)
    recs = _records(17 + n_rec, length, n_rec, g, lower_first=lower)
    block = b"\n".join(recs) + b"\n"
    assert _one_length_candidate(block) == (length, n_rec)
    assert not lower or n_rec > 5                               # (_records puts the lower case into record 5, 508, ...)
    bits = _order_bits(len(block))
    db = _kdb(L, g)
    got = {}
    for hook in (1, 0):
        rset, used = _bin_once(L, block, hook6=hook)
        assert used == (1, 0), hook
        got[hook] = (rset.packed_slabs(), _counts(L, db, rset), [r for r in rset.read_back().split(b"\n") if r])
        rset.close()
    assert got[0][0] == got[1][0] == (0 if lower else 1)
    assert np.array_equal(got[0][1], got[1][1])
    per_bin = [{}, {}]
    for h in (0, 1):
        bins = [_bin(r, bits) for r in got[h][2]]
        assert bins == sorted(bins)
        for b_, r in zip(bins, got[h][2]):
            per_bin[h].setdefault(b_, []).append(r)
    assert per_bin[0].keys() == per_bin[1].keys()
    for b_ in per_bin[0]:
        assert sorted(per_bin[0][b_]) == sorted(per_bin[1][b_]), b_
    db.close()


@pytest.mark.parametrize("letter", ["a", "R", "Y", "\r"])
def test_bytes_outside_the_alphabet_give_an_ascii_slab(L, letter):
    """A lower-case or IUPAC letter (or a carriage return) in the middle of some records: the gather's alphabet check sends the
    slab through the ASCII gather (same order), with correct counts."""
    g = _genome(5, 50150)
    recs = _records(23, 150, 9000, g, mid=letter)
    block = b"\n".join(recs) + b"\n"
    db = _kdb(L, g)
    db.reset()
    db.scan_flat(block)
    want = db.counts_rows().copy()
    rset, used = _bin_once(L, block)
    assert used == (1, 0)
    assert rset.packed_slabs() == 0
    assert np.array_equal(_counts(L, db, rset), want)
    bits = _order_bits(len(block))
    bins = [_bin(r, bits) for r in recs]
    back = [r for r in rset.read_back().split(b"\n") if r]
    assert back == [recs[i] for i in sorted(range(len(recs)), key=lambda i: bins[i])]
    rset.close()
    db.close()


def _broken_block(variant, g):
    """9 000 x 150 bases that the probe takes for records of one length and that are not."""
    recs = _records(31, 150, 9000, g)
    if variant == "inner_newline":
        recs[4000] = recs[4000][:75] + b"\n" + recs[4000][76:]
    elif variant == "inner_newline_last":
        recs[-1] = recs[-1][:140] + b"\n" + recs[-1][141:]
    else:                                                       # (and one a base longer: the byte count still divides)
        recs[2500] = recs[2500][:-1]
        recs[6000] = recs[6000] + b"A"
    block = b"\n".join(recs) + b"\n"
    assert _one_length_candidate(block) == (150, 9000)
    return recs, block


def _check_fallback(L, variant, hook6):
    g = _genome(9, 50150)
    recs, block = _broken_block(variant, g)
    db = _kdb(L, g)
    db.reset()
    db.scan_flat(block)
    want = db.counts_rows().copy()
    rset, used = _bin_once(L, block, hook6=hook6)
    assert used == (0, 1), variant
    assert np.array_equal(_counts(L, db, rset), want)
    back = [r for r in rset.read_back().split(b"\n") if r]
    assert sorted(back) == sorted(r for chunk in recs for r in chunk.split(b"\n") if r)
    rset.close()
    db.close()


@pytest.mark.parametrize("variant", ["inner_newline", "one_base_short", "inner_newline_last"])
def test_not_one_length_takes_the_general_passes(L, variant):
    """An internal newline (the byte count still divides: only the gather's check sees it) and a record one base short (the
    records behind it shifted: the key pass sees it) each go through the general passes, with the same counts as the flat scan."""
    _check_fallback(L, variant, 0)


@pytest.mark.parametrize("variant", ["inner_newline", "one_base_short"])
def test_not_one_length_under_hook6_takes_the_general_passes(L, variant):
    """The same from the count + atomic placement (ss_test_hook 6 = 1): count_fixed_kernel sees the newline in the middle of a
    record, and the record a base short (a later one a base long), and the general passes bin the slab."""
    _check_fallback(L, variant, 1)


@pytest.mark.parametrize("hook6", [0, 1])
def test_timing_after_a_fallback(L, hook6):
    """ss_reads_order_timing after a one-length attempt that fell back: count + prefix (the failed attempt in it), allocation,
    place."""
    recs, block = _broken_block("inner_newline", _genome(9, 50150))
    rset, used = _bin_once(L, block, hook6=hook6)
    assert used == (0, 1)
    timing = np.zeros(3)
    L.check(L.lib().ss_reads_order_timing(L.ptr(timing)), "ss_reads_order_timing")
    assert timing[0] > 0 and timing[1] >= 0 and timing[2] > 0
    rset.close()


def test_hooks_5_and_6_together(L):
    """The count + atomic placement with ASCII slabs asked for: an all-ACGT slab of one length stays ASCII, with correct counts;
    packed again once hook 5 is back at 0."""
    g = _genome(41, 30150)
    starts = np.random.RandomState(43).randint(0, len(g) - 150, size=6000)
    recs = [a.tobytes() for a in g[starts[:, None] + np.arange(150)[None, :]]]
    block = b"\n".join(recs) + b"\n"
    assert _one_length_candidate(block) == (150, 6000) and set(block) <= set(b"ACGT\n")
    db = _kdb(L, g)
    db.reset()
    db.scan_flat(block)
    want = db.counts_rows().copy()
    for hook5, packed in ((1, 0), (0, 1)):
        rset, used = _bin_once(L, block, hook6=1, hook5=hook5)
        assert used == (1, 0)
        assert rset.packed_slabs() == packed
        assert np.array_equal(_counts(L, db, rset), want)
        assert sorted(r for r in rset.read_back().split(b"\n") if r) == sorted(recs)
        rset.close()
    db.close()


def test_one_scratch_block_through_every_layout(L):
    """One process, one kept scratch block: the record table of the general passes (a ragged slab of ~2 MB), the sort's arrays
    (one length, ~0.3 MB, in the larger kept block), the per-record bins (the same under hook 6), a larger record table (~6 MB
    ragged: the kept block is replaced), the sort's arrays again; then the kept block is released and a slab binned afresh."""
    g = _genome(77, 60000)
    db = _kdb(L, g)
    ragged_2mb, ragged_6mb = _ragged_block(1, 13000, g), _ragged_block(2, 40000, g)
    fixed = _records(5, 150, 2000, g)
    one_len = (fixed, b"\n".join(fixed) + b"\n")
    assert _one_length_candidate(one_len[1]) == (150, 2000)
    assert 1.8e6 < len(ragged_2mb[1]) < 2.2e6 and 5.5e6 < len(ragged_6mb[1]) < 6.5e6 and 0.28e6 < len(one_len[1]) < 0.32e6
    want = {}
    for recs, block in (ragged_2mb, ragged_6mb, one_len):
        db.reset()
        db.scan_flat(block)
        want[id(block)] = db.counts_rows().copy()

    def step(what, hook6, expect):
        recs, block = what
        rset, used = _bin_once(L, block, hook6=hook6)
        assert used == expect
        assert np.array_equal(_counts(L, db, rset), want[id(block)])
        assert sorted(r for r in rset.read_back().split(b"\n") if r) == sorted(recs)
        rset.close()

    step(ragged_2mb, 0, (0, 1))
    step(one_len, 0, (1, 0))
    step(one_len, 1, (1, 0))
    step(ragged_6mb, 0, (0, 1))
    step(one_len, 0, (1, 0))
    release = getattr(L.lib(), "ss_gz_gpu_release", None)
    if release is not None:
        L.check(release(), "ss_gz_gpu_release")
        step(one_len, 0, (1, 0))
    db.close()
