"""ss_bam_select (ss_bam_extract.hip) on hand-built BAM streams: the bytes it returns and its four counters equal those of the
model below -- walk the records, keep what the loader keeps, count the hits of each kept record's decoded read with
tests/rs_model.py, take the names of the records with at least N hits, concatenate every kept record that bears one of them."""
import struct

import numpy as np
import pytest

from tests import bamio, label_model, rs_model
from tests.test_support_labeled_gpu import _all_kmers, _distinct, _kfa, _labels, _rand

pytestmark = pytest.mark.gpu

HDR = bamio.header()
K = 31


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
def walk(stream):
    """[(offset, bytes, flag, l_seq, name, packed bases, qualities)] of the records behind the header"""
    p, out = len(HDR), []
    while p < len(stream):
        bs = struct.unpack_from("<i", stream, p)[0]
        lrn = stream[p + 12]
        ncig, flag, lseq = struct.unpack_from("<HHI", stream, p + 16)
        s0 = p + 36 + lrn + 4 * ncig
        q0 = s0 + (lseq + 1) // 2
        out.append((p, 4 + bs, flag, lseq, stream[p + 36:p + 36 + lrn - 1].split(b"\0")[0], stream[s0:q0], stream[q0:q0 + lseq]))
        p += 4 + bs
    assert p == len(stream)
    return out


def read_of(flag, lseq, packed, qual, min_qual=0):
    """the flat form the loader makes of a kept record"""
    seq = "".join(bamio.CODES[b >> 4] + bamio.CODES[b & 15] for b in packed)[:lseq]
    if min_qual and qual[0] != 0xFF:
        seq = "".join("N" if q < min_qual else c for c, q in zip(seq, qual))
    return bamio.revcomp(seq) if flag & 0x10 else seq


def model(stream, keys, k, n, min_qual=0):
    """-> (the written records' bytes, [records, kept, selected, written])"""
    recs = walk(stream)
    kept = [r for r in recs if not r[2] & 0x900 and r[3]]
    text = "".join(read_of(r[2], r[3], r[5], r[6], min_qual) + "\n" for r in kept).encode()
    hits = rs_model.hits_per_record(text, keys, k)
    assert hits.size == len(kept)
    sel = [r for r, h in zip(kept, hits.tolist()) if h >= n]
    names = {r[4] for r in sel}
    out = [stream[r[0]:r[0] + r[1]] for r in kept if r[4] in names]
    return b"".join(out), [len(recs), len(kept), len(sel), len(out)]


def check(L, db, keys, stream, n, k=K, min_qual=0, labels=None, n_labels=0, label=0, say=""):
    want, wc = model(stream, keys, k, n, min_qual)
    calls = L.bam_extract_calls()
    got, c = L.bam_select(stream, db, n, labels, n_labels, label)
    assert L.bam_extract_calls() == calls + 1
    gc = [c[x] for x in L.BAM_SELECT_COUNTERS]
    print(say, "N", n, "counters", gc, "model", wc, "bytes", len(got), len(want))
    assert gc == wc
    assert got == want
    return wc


# ------------------------------------------------------------------------------------------------
# material: a genome, a k = 31 table over its first part, records
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genome():
    return _rand(np.random.RandomState(2025), 70000)


@pytest.fixture(scope="module")
def table(L, genome):
    kmers = _distinct(_all_kmers(genome[:40000], K, 2))
    db = L.KmerDB.from_text(_kfa(kmers), K, True)
    yield db, kmers, rs_model.encode_kmers(kmers, K)
    db.close()


def hot(genome, rs, n=150):
    """a read from the part of the genome the table covers (about n / 2 hits)"""
    s = int(rs.randint(0, 40000 - n))
    return genome[s:s + n].decode()


def cold(rs, n=150):
    return _rand(rs, n).decode()


def qual_of(rs, n):
    return rs.randint(2, 41, size=n).astype(np.uint8).tobytes()


def seeded_records(genome, seed, n):
    """n templates in a seeded mix: single records, mates (adjacent at first), a third kept record, decoys, records without
    bases, 0x10 records, IUPAC codes and N, no qualities, aux data of 0..40 bytes; then the whole list is shuffled, so mates lie
    anywhere"""
    rs = np.random.RandomState(seed)
    out = []
    for t in range(n):
        name = "t%d" % t
        mates = 1 + int(rs.randint(0, 2)) + (1 if rs.random_sample() < 0.02 else 0)
        for m in range(mates):
            ln = int(rs.randint(20, 260))
            r = rs.random_sample()
            seq = hot(genome, rs, ln) if r < 0.25 else cold(rs, ln) if r < 0.8 else genome[39900:39900 + ln].decode()
            if rs.random_sample() < 0.1:
                j = int(rs.randint(0, ln))
                seq = seq[:j] + "NMRWY="[int(rs.randint(0, 6))] + seq[j + 1:]
            flag = (0x1 | (0x40 if m == 0 else 0x80)) if mates > 1 else 4
            if rs.random_sample() < 0.3:
                flag |= 0x10
            q = b"\xff" * ln if rs.random_sample() < 0.03 else qual_of(rs, ln)
            out.append(bamio.record(name, seq, flag=flag, qual=q, aux=rs.bytes(int(rs.randint(0, 41))),
                                    cigar=((ln << 4),) if rs.random_sample() < 0.5 else ()))
        if rs.random_sample() < 0.1:
            out.append(bamio.record(name, hot(genome, rs, 100), flag=0x100 if rs.random_sample() < 0.5 else 0x800 | 0x10))
        if rs.random_sample() < 0.03:
            out.append(bamio.record(name, "", flag=4))
    order = rs.permutation(len(out))
    return [out[i] for i in order]


@pytest.fixture(scope="module")
def big_stream(genome):
    recs = seeded_records(genome, 7, 1900)
    assert 2900 <= len(recs) <= 3600
    return HDR + b"".join(recs)


# ------------------------------------------------------------------------------------------------
# hand-built streams
# ------------------------------------------------------------------------------------------------
def _streams(genome):
    rs = np.random.RandomState(11)
    H, C = (lambda n=150: hot(genome, rs, n)), (lambda n=150: cold(rs, n))
    R = bamio.record
    s = {}
    s["header_only"] = []
    s["one_record_selected"] = [R("only", H())]
    s["one_record_not_selected"] = [R("only", C())]
    s["first_record_alone"] = [R("first", H())] + [R("c%d" % i, C(80)) for i in range(40)]
    s["mates_adjacent"] = [R("a", C(), flag=0x41), R("a", H(), flag=0x81), R("b", C(), flag=0x41), R("b", C(), flag=0x81),
                           R("c", H(), flag=0x41), R("c", C(), flag=0x81)]
    far = [R("f%d" % i, C(80)) for i in range(520)]
    far.insert(3, R("mate", H(), flag=0x41))
    far.insert(504, R("mate", C(), flag=0x81))
    far.insert(200, R("other", C(), flag=0x41))
    far.insert(519, R("other", C(), flag=0x81))
    s["mates_500_apart"] = far
    s["three_of_one_name"] = [R("x", C()), R("y", C()), R("x", H()), R("z", C()), R("x", C(33)), R("y", C())]
    # names that are prefixes of one another, a 1-byte name, the longest name; a name field with a NUL inside is the name before it
    long_a, long_b = "n" * 254, "n" * 253 + "m"
    s["names"] = [R("r1", H()), R("r10", C()), R("r100", C()), R("r", C()), R("r1\0x", C()), R("r2", C()), R("r20", H()), R("r2\0", C()),
                  R("a", C()), R("b", H()), R("b", C()), R(long_a, H()), R(long_b, C()), R(long_a, C()), R("r1", C()), R("r", C())]
    s["decoys_share_a_selected_name"] = [R("d", H()), R("d", H(), flag=0x100), R("d", H(), flag=0x800 | 0x10), R("d", C(), flag=0x900),
                                         R("e", C()), R("e", H(), flag=0x100), R("d", C(), flag=0x81)]
    s["no_bases"] = [R("g", ""), R("g", H()), R("h", ""), R("g", "", flag=0x81), R("i", C())]
    rc = [R("rc%d" % i, bamio.revcomp(H()), flag=0x10) for i in range(3)] + [R("fw_of_rc", bamio.revcomp(H())), R("rc_cold", C(), flag=0x10)]
    s["reverse_strand"] = rc
    iu = H(150)
    s["iupac_and_n"] = [R("n_mid", iu[:75] + "N" + iu[76:]), R("iupac", "".join("MRWSYKVHDB="[i % 11] if i % 20 == 7 else c for i, c in enumerate(H()))),
                        R("all_n", "N" * 100), R("clean", H())]
    edge = []
    for ln in (30, 31, 32, 33, 34, 61, 62):
        for a in range(0, 41, 5):
            edge.append(R("e%d_%d" % (ln, a), H(ln), aux=rs.bytes(a)))
    for a in range(41):                                   # record starts at every residue mod 16
        edge.append(R("aux%d" % a, H(64 + a % 3), aux=rs.bytes(a)))
    s["lengths_around_k_and_aux"] = edge
    long_ = [R("s%d" % i, C() if i % 3 else H()) for i in range(12)]
    long_.insert(4, R("long70k", genome[:35000].decode() + cold(rs, 35000)))
    long_.insert(9, R("long150k", cold(rs, 150000), aux=b"XYZabc\0"))
    long_.insert(11, R("long150k", H(), flag=0x81))
    s["long_records"] = long_
    s["all_from_the_table"] = [R("q%d" % (i // 2), H(int(rs.randint(40, 200))), flag=0x41 if i % 2 == 0 else 0x81) for i in range(300)]
    return {k: HDR + b"".join(v) for k, v in s.items()}


@pytest.fixture(scope="module")
def streams(genome):
    return _streams(genome)


NAMES = ["header_only", "one_record_selected", "one_record_not_selected", "first_record_alone", "mates_adjacent", "mates_500_apart", "three_of_one_name", "names",
         "decoys_share_a_selected_name", "no_bases", "reverse_strand", "iupac_and_n", "lengths_around_k_and_aux", "long_records",
         "all_from_the_table"]


@pytest.mark.parametrize("n", [1, 16])
@pytest.mark.parametrize("name", NAMES)
def test_hand_built_streams_equal_the_model(L, table, streams, name, n):
    db, _, keys = table
    before = db.counts_rows().copy()
    wc = check(L, db, keys, streams[name], n, say=name)
    assert (db.counts_rows() == before).all()              # the table's counters are not touched
    if name == "header_only":
        assert wc == [0, 0, 0, 0]
    if name == "one_record_selected":
        assert wc == [1, 1, 1, 1]
    if name == "first_record_alone":
        assert wc == [41, 41, 1, 1]                        # the copy's first piece begins with the stream's first record
    if name == "mates_500_apart":
        assert wc[2] == 1 and wc[3] == 2
    if name == "three_of_one_name":
        assert wc[2] == 1 and wc[3] == 3
    if name == "decoys_share_a_selected_name":
        assert wc == [7, 3, 1, 2]
    if name == "long_records":
        assert wc[2] >= 5 and wc[3] > wc[2]
    if name == "all_from_the_table" and n == 1:
        assert wc[1] == wc[2] == wc[3] == 300
    if name == "lengths_around_k_and_aux" and n == 1:
        assert 0 < wc[2] < wc[1]                           # l_seq 30 has no window, 31 has one


@pytest.mark.parametrize("n", [1, 16, 100000])
def test_seeded_records_equal_the_model(L, table, big_stream, n):
    db, _, keys = table
    wc = check(L, db, keys, big_stream, n, say="seeded")
    assert wc[0] > wc[1] >= 2700
    if n == 100000:
        assert wc[2] == wc[3] == 0
    else:
        assert 0 < wc[2] < wc[3] < wc[1]                   # mates ride along; not everything is written


def test_last_record_ends_exactly_at_n_and_a_truncated_stream(L, table, streams):
    db, _, keys = table
    s = streams["mates_adjacent"]
    for cut in (1, 7, 40):
        with pytest.raises(L.SSError) as e:
            L.bam_select(s[:-cut], db, 1)
        assert e.value.code == L.SS_EIO
    with pytest.raises(L.SSError) as e:
        L.bam_select(s[:len(HDR) - 3], db, 1)
    assert e.value.code == L.SS_EIO
    with pytest.raises(L.SSError) as e:
        L.bam_select(b"BAX\1" + s[4:], db, 1)
    assert e.value.code == L.SS_EIO
    check(L, db, keys, s, 1, say="after the damaged ones")


def test_host_walk_serves_a_stream_the_device_walk_declines(L, table, big_stream, streams):
    db, _, keys = table
    L.check(L.lib().ss_test_hook(7, 1), "hook")
    try:
        check(L, db, keys, big_stream, 16, say="host walk")
        check(L, db, keys, streams["long_records"], 1, say="host walk, long")
        with pytest.raises(L.SSError) as e:
            L.bam_select(big_stream[:-5], db, 1)
        assert e.value.code == L.SS_EIO
    finally:
        L.check(L.lib().ss_test_hook(7, 0), "hook")


def test_k25_table(L, genome, streams, big_stream):
    kmers = _distinct(_all_kmers(genome[:40000], 25, 3))
    db = L.KmerDB.from_text(_kfa(kmers), 25, True)
    try:
        keys = rs_model.encode_kmers(kmers, 25)
        wc = check(L, db, keys, big_stream, 16, k=25, say="k25 seeded")
        assert 0 < wc[2] < wc[1]
        check(L, db, keys, streams["lengths_around_k_and_aux"], 1, k=25, say="k25 lengths")
    finally:
        db.close()


def test_refusals(L, table, genome, streams):
    import ctypes as C
    db, _, keys = table
    s = streams["mates_adjacent"]
    flat = L.KmerDB.from_text(_kfa(_distinct(_all_kmers(genome[:3000], 15, 1))), 15, True)
    try:
        with pytest.raises(L.SSError) as e:
            L.bam_select(s, flat, 1)
        assert e.value.code == L.SS_ERANGE
    finally:
        flat.close()
    with pytest.raises(L.SSError) as e:
        L.bam_select(s, db, 0)
    assert e.value.code == L.SS_EINVAL
    lab = np.ones(db.n_rows, np.uint8)
    for nl, j in ((0, 1), (16, 1), (2, 0), (2, 3)):
        with pytest.raises(L.SSError) as e:
            L.bam_select(s, db, 1, lab, nl, j)
        assert e.value.code == L.SS_EINVAL, (nl, j)
    with pytest.raises(L.SSError) as e:
        L.bam_select(s, db, 1, lab + 2, 2, 1)              # a row label above n_labels
    assert e.value.code == L.SS_EINVAL
    # cap too small: SS_ERANGE, *out_len exact, the counters set
    want, wc = model(s, keys, K, 1)
    assert len(want) > 100
    out = np.zeros(len(want), np.uint8)
    n, c = C.c_uint64(), (C.c_uint64 * 4)()
    for cap in (0, len(want) - 1):
        rc = L.lib().ss_bam_select(s, len(s), db.handle, None, 0, 0, 1, L.ptr(out), cap, C.byref(n), c)
        assert rc == L.SS_ERANGE and n.value == len(want) and list(c) == wc
        assert not out.any()
    rc = L.lib().ss_bam_select(s, len(s), db.handle, None, 0, 0, 1, L.ptr(out), len(want), C.byref(n), c)
    assert rc == 0 and out.tobytes() == want


def test_base_quality_mask(L, table, genome):
    db, _, keys = table
    rs = np.random.RandomState(3)
    good = bytes([35] * 150)
    holes = bytes([5 if i % 20 == 10 else 35 for i in range(150)])      # no window of 31 bases survives the mask
    recs = [bamio.record("clean", hot(genome, rs), qual=good), bamio.record("holes", hot(genome, rs), qual=holes),
            bamio.record("holes_rc", bamio.revcomp(hot(genome, rs)), flag=0x10, qual=holes),
            bamio.record("no_qual", hot(genome, rs), qual=b"\xff" * 150), bamio.record("cold", cold(rs), qual=good),
            bamio.record("low_tail", hot(genome, rs), qual=bytes([35] * 100 + [3] * 50))]
    s = HDR + b"".join(recs)
    assert check(L, db, keys, s, 16, say="mask off")[2] == 5
    L.set_min_base_qual(20)
    try:
        wc = check(L, db, keys, s, 16, min_qual=20, say="mask 20")
        assert wc[2] == 3                                              # clean, no_qual, low_tail
        assert check(L, db, keys, s, 40, min_qual=20, say="mask 20, N 40")[2] == 2
    finally:
        L.set_min_base_qual(0)
    assert check(L, db, keys, s, 16, say="mask off again")[2] == 5


def test_labelled_equals_the_model_on_each_labels_kmers(L, table, big_stream, streams):
    db, kmers, keys = table
    lab = _labels(len(kmers), 2, 77)
    sizes = []
    for j in (1, 2):
        own = label_model.label_keys(keys, lab, j)
        for n in (1, 8):
            sizes.append(check(L, db, own, big_stream, n, labels=lab, n_labels=2, label=j, say="label %d" % j)[2])
        check(L, db, own, streams["mates_500_apart"], 4, labels=lab, n_labels=2, label=j, say="label %d far" % j)
    assert all(sizes), sizes
    plain = model(big_stream, keys, K, 8)[1][2]
    assert all(x <= plain for x in sizes[1::2])


def test_selected_equals_the_resident_sets_select(L, table, big_stream, tmp_path):
    """counters[2] = the records ss_reads_select takes from the same BAM loaded as a sample"""
    db, _, keys = table
    p = tmp_path / "s.bam"
    p.write_bytes(bamio.bgzf(HDR, [big_stream[r[0]:r[0] + r[1]] for r in walk(big_stream)], level=1))
    rset = L.ReadSet([str(p)])
    try:
        for n in (1, 16):
            sub = rset.select(db, n)
            try:
                _, c = L.bam_select(big_stream, db, n)
                assert c["selected"] == sub.info()["n_records"] > 0
                assert c["kept"] == rset.info()["n_records"]
            finally:
                sub.close()
    finally:
        rset.close()
