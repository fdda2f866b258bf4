"""ss_bam_mates, ss_reads_join_pairs_bam and ss_bam_select_pairs (ss_bam_pairs.hip) against tests/bam_pairs_model.py on the streams
of tests/bam_pairs_cases.py: the mate link element for element, the joined set read back byte for byte (order = 0) and as a
multiset of records (order = 1), each violating shape refused with the model's counters, the device walk-decline route, the
base-quality mask, the hits of the fragments adding up to those of the reads, and the selection by fragment."""
import collections

import numpy as np
import pytest

from tests import bam_pairs_cases as cases, bam_pairs_model as bpm, bamio, rs_model
from tests.test_bam_select_gpu import K, cold, genome, hot, table      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def streams():
    return {n: cases.stream(n) for n in cases.SIZES}


def _counters(L, c):
    return [c[k] for k in L.BAM_PAIR_COUNTERS]


def check_mates(L, s):
    _, want, wc, _ = bpm.fragments(s)
    got, c = L.bam_mates(s)
    print("counters", _counters(L, c), "model", wc)
    assert _counters(L, c) == wc
    assert got.dtype == np.uint32 and got.shape == want.shape and (got == want).all(), np.nonzero(got != want)[0][:10]
    return wc


def check_join(L, s, min_qual=0):
    frags, _, wc, _ = bpm.fragments(s, min_qual)
    want = b"".join(f + b"\n" for f in frags)
    calls = L.join_pairs_calls()
    rset = L.ReadSet.join_pairs_bam(s, order=False)
    try:
        assert L.join_pairs_calls() == calls + 1
        assert _counters(L, rset.pair_counters) == wc
        text, info = rset.read_back(), rset.info()
        first = next((i for i in range(min(len(text), len(want))) if text[i] != want[i]), None)
        assert text[:len(want)] == want, ("first difference at byte", first)
        if want:
            assert len(text) % 16 == 0 and len(text) > len(want) and text[len(want):] == b"\n" * (len(text) - len(want))
        else:
            assert text == b""
        flat_len = len(bamio.flat(bamio.decode(s))[0])
        assert len(want) == (flat_len - wc[1]) + 2 * len(frags)
        assert info["n_records"] == len(frags) and info["n_bases"] == len(want) - len(frags)
        assert rset.packed_slabs() == 0
    finally:
        rset.close()
    ordered = L.ReadSet.join_pairs_bam(s, order=True)
    try:
        got = collections.Counter(r for r in ordered.read_back().split(b"\n") if r) if not ordered.packed_slabs() else None
        assert ordered.info()["n_records"] == len(frags)
        if got is not None:
            assert got == collections.Counter(frags)
        assert _counters(L, ordered.pair_counters) == wc
    finally:
        ordered.close()
    return frags, wc


@pytest.mark.parametrize("n", cases.SIZES)
def test_mates_equal_the_model(L, streams, n):
    wc = check_mates(L, streams[n])
    assert wc[0] == n and wc[5] == 0


@pytest.mark.parametrize("n", cases.SIZES)
def test_joined_set_equals_the_model(L, streams, n):
    frags, wc = check_join(L, streams[n])
    if n >= 255:
        assert wc[2] > 100 and wc[3] >= 6 and wc[4] >= 5


def test_ordered_set_is_the_same_multiset_of_records(L):
    """order = 1 on records the binning keeps as ASCII text (IUPAC codes: not packed), so the records can be read back"""
    rs = np.random.RandomState(5)
    recs = []
    for i in range(300):
        a, b = ("".join("ACGTRY"[j] for j in rs.randint(0, 6, size=n)) for n in (40 + i % 7, 33 + i % 5))
        recs += [bamio.record("m%d" % i, a, flag=0x41), bamio.record("m%d" % i, b, flag=0x81 | 0x10)]
    recs = [recs[j] for j in rs.permutation(len(recs))]
    s = cases.HDR + b"".join(recs)
    frags, _, wc, _ = bpm.fragments(s)
    rset = L.ReadSet.join_pairs_bam(s, order=True)
    try:
        assert rset.packed_slabs() == 0
        assert collections.Counter(r for r in rset.read_back().split(b"\n") if r) == collections.Counter(frags)
        assert rset.info()["n_records"] == 300 == wc[2]
    finally:
        rset.close()


@pytest.mark.parametrize("shape", ["three_of_one_name", "two_of_role_1", "role_0_shares_a_name", "one_name_257"])
def test_violations_are_refused_with_the_models_counters(L, shape):
    import ctypes as C
    s = cases.violating()[shape]
    _, want, wc, _ = bpm.fragments(s)
    assert wc[5]
    got, c = L.bam_mates(s)
    assert _counters(L, c) == wc and (got == want).all()
    for order in (0, 1):
        h, cc = C.c_void_p(), (C.c_uint64 * 6)()
        rc = L.lib().ss_reads_join_pairs_bam(s, len(s), order, C.byref(h), cc)
        assert rc == L.SS_EIO and not h.value and list(cc) == wc
    with pytest.raises(L.SSError) as e:
        L.ReadSet.join_pairs_bam(s)
    assert e.value.code == L.SS_EIO and e.value.pair_counters["violating"] == wc[5]


def test_device_walk_decline_route(L, streams):
    L.check(L.lib().ss_test_hook(7, 1), "hook")
    try:
        check_mates(L, streams[257])
        check_join(L, streams[257])
        check_join(L, streams[2])
        with pytest.raises(L.SSError) as e:
            L.ReadSet.join_pairs_bam(streams[257][:-5])
        assert e.value.code == L.SS_EIO and e.value.pair_counters["violating"] == 0
    finally:
        L.check(L.lib().ss_test_hook(7, 0), "hook")


def test_base_quality_mask(L, streams):
    plain, _ = check_join(L, streams[256])
    L.set_min_base_qual(20)
    try:
        masked, _ = check_join(L, streams[256], min_qual=20)
    finally:
        L.set_min_base_qual(0)
    assert masked != plain and sum(f.count(b"N") for f in masked) > sum(f.count(b"N") for f in plain)
    # the pair without qualities is not masked
    assert [f for f in masked if f.count(b"N") == 1 and len(f) == 150 + 1 + 16]


def test_damaged_streams_and_bad_arguments(L, streams):
    import ctypes as C
    s = streams[255]
    for bad in (s[:-3], b"BAX\1" + s[4:]):
        with pytest.raises(L.SSError) as e:
            L.bam_mates(bad)
        assert e.value.code == L.SS_EIO
        with pytest.raises(L.SSError) as e:
            L.ReadSet.join_pairs_bam(bad)
        assert e.value.code == L.SS_EIO
    c = (C.c_uint64 * 6)()
    small = np.zeros(10, np.uint32)
    assert L.lib().ss_bam_mates(s, len(s), L.ptr(small), 10, c) == L.SS_ERANGE and c[0] == 255
    assert L.lib().ss_bam_mates(s, len(s), None, 0, None) == L.SS_EINVAL
    assert L.lib().ss_reads_join_pairs_bam(s, len(s), 0, None, c) == L.SS_EINVAL


# ------------------------------------------------------------------------------------------------
# reads from a genome: hits, the file loader, the selection by fragment
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genome_records(genome):      # noqa: F811
    """pairs, orphans and singles of hot and cold reads, shuffled; decoys under pair names"""
    rs = np.random.RandomState(31)
    out = []
    for i in range(400):
        a = hot(genome, rs, 100) if i % 3 == 0 else cold(rs, 100)
        b = hot(genome, rs, 90) if i % 5 == 0 else cold(rs, 90)
        out.append(bamio.record("g%d" % i, a, flag=0x41))
        out.append(bamio.record("g%d" % i, bamio.revcomp(b), flag=0x81 | 0x10))
        if i % 50 == 0:
            out.append(bamio.record("g%d" % i, hot(genome, rs, 100), flag=0x100 | 0x41))
    out += [bamio.record("orph%d" % i, hot(genome, rs, 80), flag=0x81) for i in range(20)]
    out += [bamio.record("single%d" % (i % 4), hot(genome, rs, 70) if i % 2 else cold(rs, 70), flag=4) for i in range(20)]
    return [out[j] for j in rs.permutation(len(out))]


def test_hits_of_the_fragments_add_up_to_those_of_the_reads(L, table, genome_records, tmp_path):      # noqa: F811
    db, _, keys = table
    p = tmp_path / "s.bam"
    p.write_bytes(bamio.bgzf(cases.HDR, genome_records, level=1))
    s = cases.HDR + b"".join(genome_records)
    frags, _, wc, _ = bpm.fragments(s)
    plain = L.ReadSet([str(p)])
    calls = L.join_pairs_calls()
    joined = L.ReadSet.load_pairs_bam(str(p), order=False)
    ordered = L.ReadSet.load_pairs_bam(str(p))
    try:
        assert L.join_pairs_calls() == calls + 2
        assert _counters(L, joined.pair_counters) == wc and wc[2] == 400 and wc[3] == 20 and wc[4] == 20
        want = b"".join(f + b"\n" for f in frags)
        assert joined.read_back()[:len(want)] == want
        hits = [r.support(db)[1] for r in (plain, joined, ordered)]
        model = int(rs_model.hits_per_record(want, keys, K).sum())
        print("hits", hits, "model", model)
        assert hits[0] == hits[1] == hits[2] == model > 0
        assert joined.info()["n_records"] == ordered.info()["n_records"] == len(frags) == plain.info()["n_records"] - wc[2]
        t = L.bam_pairs_timing()
        assert t["total"] > 0 and all(v >= 0 for v in t.values())
    finally:
        for r in (plain, joined, ordered):
            r.close()
    with pytest.raises(L.SSError) as e:
        L.ReadSet.load_pairs_bam(str(tmp_path / "absent.bam"))
    assert e.value.code == L.SS_EINVAL                      # (not a BAM: nothing to look at)


def check_select(L, db, keys, s, n):
    want, wc = bpm.select(s, lambda text: rs_model.hits_per_record(text, keys, K), n)
    calls = L.bam_extract_calls()
    got, c = L.bam_select(s, db, n, pairs=True)
    assert L.bam_extract_calls() == calls + 1
    gc = [c[x] for x in L.BAM_SELECT_COUNTERS]
    print("N", n, "counters", gc, "model", wc)
    assert gc == wc and got == want
    return wc


def test_selection_by_fragment(L, table, genome, genome_records):      # noqa: F811
    db, _, keys = table
    s = cases.HDR + b"".join(genome_records)
    for n in (1, 40, 90, 100000):
        wc = check_select(L, db, keys, s, n)
        # (a pair's two records are written together, a decoy never: written = records of the selected fragments)
        assert wc[3] >= wc[2] and (n < 100000 or wc[2] == wc[3] == 0)
    rs = np.random.RandomState(9)
    R = bamio.record
    recs = [R("both_halves", genome[1000:1060].decode() + cold(rs, 30), flag=0x41), R("far", cold(rs, 50), flag=0x81),
            R("one_alone", hot(genome, rs, 100), flag=0x81), R("both_halves", "", flag=0x81),
            R("both_halves", genome[3000:3100].decode(), flag=0x81 | 0x100), R("orphan", hot(genome, rs, 100), flag=0x41),
            R("one_alone", cold(rs, 60), flag=0x41), R("far", cold(rs, 50), flag=0x41),
            R("both_halves", bamio.revcomp(genome[2000:2060].decode()), flag=0x81 | 0x10), R("one_alone", hot(genome, rs, 100), flag=0x800 | 0x41)]
    s = cases.HDR + b"".join(recs)
    forms = bpm.flat_forms(s, bpm.walk(s))
    h = {i: int(rs_model.hits_per_record(f + b"\n", keys, K)[0]) for i, f in forms.items()}
    n = max(h[0], h[8]) + 1
    assert sorted(h) == [0, 1, 2, 5, 6, 7, 8] and h[0] and h[8] and h[0] + h[8] >= n      # neither mate of both_halves reaches n alone
    assert h[2] >= n > h[6] and h[5] >= n > h[1] + h[7]                                     # one mate alone; the orphan; nothing
    wc = check_select(L, db, keys, s, n)
    assert wc == [10, 7, 3, 5]                              # both_halves (2 records), one_alone (2), orphan (1); never a record not kept
    plain, pc = L.bam_select(s, db, n)
    assert pc["selected"] == 2 and pc["written"] == 3       # by record: one_alone's hot mate and the orphan, one_alone's mate by name
    with pytest.raises(L.SSError) as e:
        L.bam_select(cases.violating()["two_of_role_1"], db, 1, pairs=True)
    assert e.value.code == L.SS_EIO
    L.bam_select(cases.violating()["two_of_role_1"], db, 1)      # the template join does not mind


def test_extract_pairs_writes_the_selected_fragments_and_leaves_no_file_on_a_violation(L, table, genome_records, tmp_path):      # noqa: F811
    db, _, keys = table
    p, out = tmp_path / "s.bam", tmp_path / "out.bam"
    p.write_bytes(bamio.bgzf(cases.HDR, genome_records, level=1))
    s = cases.HDR + b"".join(genome_records)
    want, wc = bpm.select(s, lambda text: rs_model.hits_per_record(text, keys, K), 40)
    c = L.bam_extract(str(p), db, 40, str(out), pairs=True)
    assert [c[x] for x in L.BAM_SELECT_COUNTERS] == wc and wc[2] > 0
    import gzip
    assert gzip.decompress(out.read_bytes()) == cases.HDR + want
    bad, out2 = tmp_path / "bad.bam", tmp_path / "out2.bam"
    bad.write_bytes(bamio.bgzf(cases.HDR, [cases.violating()["three_of_one_name"][len(cases.HDR):]], level=1))
    with pytest.raises(L.SSError) as e:
        L.bam_extract(str(bad), db, 1, str(out2), pairs=True)
    assert e.value.code == L.SS_EIO and not out2.exists() and not (tmp_path / "out2.bam.tmp").exists()
