"""ss_reads_resample (ss_resample.hip): a resident set resampled with replacement.  The device is held to tests/boot_model.py: the
multiset of records read back is every record as often as the model's weight says (the order is unspecified), n_records and n_bases
are exact, the weight depends on a record's bytes only (file order, binned ASCII and packed give one multiset), a call repeats
itself, replicates differ, the resampled set scans like any other (its counts are those of the CPU oracle on the model's
resampled reads, at k = 31 and k = 25), and the refusals are those the header states."""
import ctypes as C

import numpy as np
import pytest

from tests import boot_model

pytestmark = pytest.mark.gpu

SEED = 20


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _rand(rs, n):
    return np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, size=n)].tobytes()


@pytest.fixture(scope="module")
def genome():
    return _rand(np.random.RandomState(77), 60000)


def _ragged_block(genome):
    """Every length 1..400 (so records begin and end at every offset modulo 16 and straddle the 1024-byte tiles), one record of
    2 600 bytes and one of 1 025, lower case, N, '\\r' at a record's end, empty lines"""
    rs = np.random.RandomState(3)
    recs = []
    for ln in rs.permutation(np.arange(1, 401)).tolist():
        s = int(rs.randint(0, len(genome) - ln))
        r = bytearray(genome[s:s + ln])
        if ln % 7 == 0:
            r[ln // 2:] = bytes(r[ln // 2:]).lower()
        if ln % 11 == 0:
            r[int(rs.randint(0, ln))] = ord("N")
        if ln % 13 == 0:
            r[-1] = ord("\r")
        recs.append(bytes(r))
    recs.insert(100, genome[2000:4600])
    recs.insert(300, genome[9000:10025].lower())
    block = b"\n".join(recs[:150]) + b"\n\n\n" + b"\n".join(recs[150:]) + b"\n"
    assert max(map(len, recs)) > 1024
    return block


def _one_length_block(genome, n, seed):
    """n distinct-looking 150-base reads, A C G T and a few N: a slab that binning packs"""
    rs = np.random.RandomState(seed)
    g = np.frombuffer(genome, np.uint8)
    starts = rs.randint(0, g.size - 150, size=n)
    arr = g[starts[:, None] + np.arange(150)[None, :]].copy()
    arr[::9, 75] = ord("N")
    arr[4::31, 0] = ord("N")
    arr[5::37, 149] = ord("N")
    return b"".join(a.tobytes() + b"\n" for a in arr)


@pytest.fixture(scope="module")
def loader(L):
    import torch
    keep, made = [], []

    def flat(block, order, ascii_slabs=False):
        d = torch.frombuffer(bytearray(block if block else b"\n"), dtype=torch.uint8).cuda()
        keep.append(d)
        L.check(L.lib().ss_test_hook(5, 1 if ascii_slabs else 0), "ss_test_hook")
        try:
            rset = L.ReadSet.from_flat_dev(d.data_ptr(), len(block), order=order)
        finally:
            L.lib().ss_test_hook(5, 0)
        L.check(L.lib().ss_device_sync(), "sync")
        made.append(rset)
        return rset

    yield flat
    for r in made:
        r.close()


def _records(text):
    return sorted(p for p in text.split(b"\n") if p)


def _check(L, rset, flat, seed, replicate):
    """resample `rset`, whose records are those of `flat`, and hold the result to the model; -> the sorted records"""
    want = boot_model.resampled(L, flat, seed, replicate)
    calls = L.resample_calls()
    sub = rset.resample(seed, replicate)
    try:
        assert L.resample_calls() == calls + 1
        text = sub.read_back()
        info = sub.info()
        got = _records(text)
        print("records", len(boot_model.records_of(flat)), "seed", seed, "replicate", replicate, "drawn", len(want), "device", info["n_records"],
              info["n_bases"])
        assert len(text) % 16 == 0 and (not text or text.endswith(b"\n"))
        assert got == want
        assert info["n_records"] == len(want) and info["n_bases"] == sum(map(len, want))
        assert sub.packed_slabs() == 0
        if not want:
            assert text.replace(b"\n", b"") == b""
    finally:
        sub.close()
    return got


@pytest.mark.parametrize("order", [False, True])
def test_ragged_ascii(L, loader, genome, order):
    block = _ragged_block(genome)
    rset = loader(block, order)
    assert rset.packed_slabs() == 0
    before = rset.read_back()
    for rep in (0, 1, 5):
        got = _check(L, rset, block, SEED, rep)
        assert len(got) > 300
    assert rset.read_back() == before                       # the source set is left alone
    recs, w = boot_model.weights(L, block, SEED, 0)
    assert w.max() >= 3 and (w == 0).sum() > 100            # the model itself draws nothing, one and several
    long_rec = max(recs, key=len)
    assert any(w[recs.index(long_rec)] > 0 for w in (boot_model.weights(L, block, SEED, r)[1] for r in (0, 1, 5)))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
def test_one_length_packed(L, loader, genome, n):
    block = _one_length_block(genome, n, 100 + n)
    rset = loader(block, True)
    assert rset.packed_slabs() >= 1
    for rep in (0, 3):
        _check(L, rset, block, SEED, rep)


def test_three_layouts_one_multiset(L, loader, genome):
    """the weight depends on the record's bytes only: the same reads in file order, binned as ASCII and packed"""
    block = _one_length_block(genome, 1500, 9)
    sets = {"file": loader(block, False), "binned": loader(block, True, ascii_slabs=True), "packed": loader(block, True)}
    assert sets["file"].packed_slabs() == 0 and sets["binned"].packed_slabs() == 0 and sets["packed"].packed_slabs() >= 1
    assert sets["binned"].read_back() != sets["file"].read_back()      # (binning did permute them)
    got = {name: _check(L, r, block, 7, 2) for name, r in sets.items()}
    assert got["file"] == got["binned"] == got["packed"]
    # identical reads share a weight: every record of the doubled block is drawn an even number of times
    twice = loader(block + block, False)
    sub = twice.resample(7, 2)
    try:
        assert _records(sub.read_back()) == sorted(got["file"] + got["file"])
    finally:
        sub.close()


def test_repeats_itself_and_replicates_differ(L, loader, genome):
    block = _one_length_block(genome, 1200, 10)
    rset = loader(block, True)
    subs = [rset.resample(5, 0), rset.resample(5, 0), rset.resample(5, 1), rset.resample(6, 0)]
    try:
        texts = [s.read_back() for s in subs]
    finally:
        for s in subs:
            s.close()
    assert texts[0] == texts[1]                             # byte for byte, not only as a multiset
    assert _records(texts[0]) != _records(texts[2]) and _records(texts[0]) != _records(texts[3])
    assert _records(texts[2]) == boot_model.resampled(L, block, 5, 1) and _records(texts[3]) == boot_model.resampled(L, block, 6, 0)


def test_no_records(L, loader):
    for block in (b"", b"\n" * 40):
        rset = loader(block, False)
        sub = rset.resample(1, 0)
        try:
            assert sub.info()["n_records"] == 0 and sub.info()["n_bases"] == 0
            assert sub.read_back().replace(b"\n", b"") == b""
            again = sub.resample(1, 1)                      # a valid set: it resamples in turn
            assert again.info()["n_records"] == 0
            again.close()
        finally:
            sub.close()


def test_one_record_nothing_and_several(L, loader, genome):
    rec = genome[500:650]
    block = rec + b"\n"
    w = np.array([int(boot_model.weights(L, block, SEED, r)[1][0]) for r in range(200)])
    zero, many = int(np.nonzero(w == 0)[0][0]), int(np.nonzero(w >= 2)[0][0])
    for order in (False, True):
        rset = loader(block, order)
        assert _check(L, rset, block, SEED, zero) == []
        assert _check(L, rset, block, SEED, many) == [rec] * int(w[many])


@pytest.mark.parametrize("k", [31, 25])
def test_scan_of_the_resampled_set(L, loader, genome, k):
    """counts of the resampled set = sum over records of weight x the record's hits per row: the CPU oracle counts the model's
    resampled reads"""
    from oracle import oracle as orc
    kmers = list(dict.fromkeys(genome[i:i + k] for i in range(0, 30000, 3)))
    kfa = b"".join(b">1\n" + km + b"\n" for km in kmers)
    block = _one_length_block(genome, 2000, 40 + k) + _ragged_block(genome)
    db = L.KmerDB.from_text(kfa, k, True)
    try:
        for order in (False, True):
            rset = loader(block, order)
            sub = rset.resample(SEED, 4)
            try:
                db.reset()
                sub.scan_into(db)
                L.check(L.lib().ss_device_sync(), "sync")
                got = db.counts_rows().copy()
            finally:
                sub.close()
            recs, w = boot_model.weights(L, block, SEED, 4)
            fq = b"".join((b"@r\n" + r + b"\n+\n" + b"I" * len(r) + b"\n") * int(n) for r, n in zip(recs, w.tolist()))
            want, _ = orc.jellyfish_count(kfa, [fq], k=k, upper=True)
            assert want.sum() > 10000
            assert np.array_equal(got, want), (k, order)
    finally:
        db.close()


def test_order_bins_a_resampled_set_in_place(L, loader, genome):
    """ReadSet.order (ss_reads_order), what --bootstrap does to a replicate before its scan: the same records, the same counts;
    one-length records end up packed, ragged ones binned as ASCII; a second call and a set of no records are left alone"""
    from oracle import oracle as orc
    kmers = list(dict.fromkeys(genome[i:i + 31] for i in range(0, 30000, 3)))
    kfa = b"".join(b">1\n" + km + b"\n" for km in kmers)
    db = L.KmerDB.from_text(kfa, 31, True)
    try:
        for block, packed in ((_one_length_block(genome, 3000, 77), True), (_ragged_block(genome), False)):
            sub = loader(block, False).resample(SEED, 2)
            try:
                want = boot_model.resampled(L, block, SEED, 2)
                info = sub.info()
                db.reset()
                sub.scan_into(db)
                L.check(L.lib().ss_device_sync(), "sync")
                before = db.counts_rows().copy()
                assert sub.order() is sub
                assert (sub.packed_slabs() >= 1) == packed
                text = sub.read_back()
                assert _records(text) == want and sub.info()["n_records"] == info["n_records"] and sub.info()["n_bases"] == info["n_bases"]
                db.reset()
                sub.scan_into(db)
                L.check(L.lib().ss_device_sync(), "sync")
                assert before.sum() > 1000 and np.array_equal(db.counts_rows(), before)
                fq = b"".join(b"@r\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for r in want)
                assert np.array_equal(before, orc.jellyfish_count(kfa, [fq], k=31, upper=True)[0])
                sub.order()                                         # binned already: nothing to do
                assert sub.read_back() == text
                again = sub.resample(SEED, 3)                       # a binned (packed) set resamples like any other
                try:
                    assert _records(again.read_back()) == boot_model.resampled(L, b"\n".join(want) + b"\n", SEED, 3)
                finally:
                    again.close()
            finally:
                sub.close()
    finally:
        db.close()
    empty = loader(b"\n" * 40, False).resample(1, 0)
    try:
        empty.order()
        assert empty.info()["n_records"] == 0
    finally:
        empty.close()
    assert L.lib().ss_reads_order(None) == L.SS_EINVAL


def test_refusals(L, loader, genome, tmp_path, monkeypatch):
    rset = loader(_one_length_block(genome, 10, 1), False)
    before = L.resample_calls()
    h = C.c_void_p()
    assert L.lib().ss_reads_resample(None, 1, 0, C.byref(h)) == L.SS_EINVAL
    assert L.lib().ss_reads_resample(rset._h, 1, 0, None) == L.SS_EINVAL
    assert L.lib().ss_reads_resample_calls(None) == L.SS_EINVAL
    # a record longer than a block of the sequential reader is cut: its pieces are no reads (ss_reads_select refuses the same set)
    p = tmp_path / "long.fa"
    p.write_bytes(b">long\n" + genome[:50000] * 700 + b"\n>short\nACGTACGTAC\n")
    monkeypatch.setenv("SS_INGEST", "sequential")
    cut = L.ReadSet([str(p)])
    try:
        with pytest.raises(L.SSError) as e:
            cut.resample(1, 0)
        assert e.value.code == L.SS_ERANGE
        db = L.KmerDB.from_text(b">1\n" + genome[:31] + b"\n", 31, True)
        try:
            with pytest.raises(L.SSError) as e:
                cut.select(db, 1)
            assert e.value.code == L.SS_ERANGE
        finally:
            db.close()
    finally:
        cut.close()
    assert L.resample_calls() == before
