"""ss_bam_tag_stream / ss_bam_tag_file (ss_bam_tag.hip) on hand-built BAM streams: the body they return, byte for byte, the six
counters, direct, node_hits and kmers equal those of tests/bam_tag_model.py.  The table is k = 31 over 40 kb of a random genome
(every second k-mer), as in tests/test_bam_select_gpu.py; the node sets are disjoint 4 kb stretches of it in a forest of two trees:

    1 -+- 2 -+- 4        7 -+- 8        stretch v - 1 (bases 4000 (v - 1) .. 4000 v) belongs to node v;
       |     +- 5           +- 9        bases 36000 .. 40000 are in the table and nobody's (node 0)
       +- 3 --- 6

Aux data is well-formed throughout (the call walks it field by field): streams taken from tests/bam_pairs_cases.py, whose records
carry random aux bytes, get fields of the same length in their place (lengths 1..3, which no field has, become 0)."""
import ctypes as C
import os
import struct
import types

import numpy as np
import pytest

from tests import bam_pairs_cases, bam_pairs_model, bam_tag_model, bamio, rs_model
from tests.test_support_labeled_gpu import _kfa, _rand

pytestmark = pytest.mark.gpu

HDR = bamio.header()
K = 31
STRETCH = 4000
PARENT = np.array([0, 0, 1, 1, 2, 2, 3, 0, 7, 7], np.uint32)
VALUE = np.array([-1, 101, 102, 103, 104, 105, 106, 2000000007, 108, 109], np.int32)
R = bamio.record


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def genome():
    return _rand(np.random.RandomState(2025), 70000)


@pytest.fixture(scope="module")
def T(L, genome):
    starts = list(range(0, 40000 - K + 1, 2))
    kmers = [genome[i:i + K] for i in starts]
    assert len(set(kmers)) == len(kmers)
    db = L.KmerDB.from_text(_kfa(kmers), K, True)
    stretch = np.array([i // STRETCH for i in starts])
    row_node = np.where(stretch < 9, stretch + 1, 0).astype(np.uint32)
    t = types.SimpleNamespace(db=db, keys=rs_model.encode_kmers(kmers, K), row_node=row_node, parent=PARENT, n=9, value=VALUE, stretch=stretch)
    yield t
    db.close()


def of_node(genome, v, off, n):
    """n bases of node v's stretch from an EVEN offset on: (n - 30) / 2 windows of it are rows of the table"""
    assert off % 2 == 0 and off + n <= STRETCH
    return genome[(v - 1) * STRETCH + off:(v - 1) * STRETCH + off + n].decode()


def cold(rs, n=150):
    return _rand(rs, n).decode()


def qual_of(rs, n):
    return rs.randint(2, 41, size=n).astype(np.uint8).tobytes()


def aux_exact(rs, n):
    """well-formed aux fields of exactly n bytes (n in 1..3: none), no tag of them sn, sc, Xa or Xb"""
    if n < 4:
        return b""
    pick = int(rs.randint(0, 6))
    if pick == 0 and n >= 8:
        f = b"XC" + b"C" + rs.bytes(1)
    elif pick == 1 and n >= 9:
        f = b"Xs" + b"S" + rs.bytes(2)
    elif pick == 2 and n >= 11:
        f = b"Xi" + b"i" + rs.bytes(4)
    elif pick == 3 and n >= 16:
        c = int(rs.randint(0, (n - 12) // 2 + 1))
        f = b"XB" + b"Bs" + struct.pack("<I", c) + rs.bytes(2 * c)
    else:
        return b"XZZ" + bytes(rs.randint(33, 127, size=n - 4).astype(np.uint8)) + b"\0"
    return f + (aux_exact(rs, n - len(f)) if n - len(f) >= 4 else b"XZZ" + b"z" * (n - len(f) - 4) + b"\0" if n - len(f) else b"")


def well_formed(stream, seed=5):
    """`stream` with every record's aux bytes replaced by well-formed fields of the same length (1..3 bytes: none)"""
    rs = np.random.RandomState(seed)
    out = [stream[:bam_pairs_model.header_end(stream)]]
    for r in bam_pairs_model.walk(stream):
        raw = stream[r["at"]:r["at"] + r["size"]]
        n_aux = len(bam_tag_model.aux_of(stream, r["at"], r["size"]))
        body = raw[4:len(raw) - n_aux] + aux_exact(rs, n_aux)
        out.append(struct.pack("<i", len(body)) + body)
    return b"".join(out)


def test_aux_exact_is_exact_and_well_formed():
    rs = np.random.RandomState(1)
    for n in list(range(0, 60)) * 8:
        a = aux_exact(rs, n)
        assert len(a) == (n if n >= 4 else 0)
        assert bam_tag_model.aux_walk(a, b"snsc") == 0 and bam_tag_model.aux_walk(a, b"XaXb") == 0


def check(L, T, stream, m=5, pairs=False, tags=b"snsc", min_qual=0, say=""):
    """the call against the model -> (body or None, the model's counters, the model's direct)"""
    want, wc, wd, wh, wk = bam_tag_model.model(stream, T.keys, T.row_node, T.parent, T.n, K, m, T.value, tags, pairs, min_qual)
    calls = L.bam_tag_calls()
    if want is None:
        with pytest.raises(L.BamTagError) as e:
            L.bam_tag(stream, T.db, T.row_node, T.parent, m, T.value, pairs, tags)
        print(say, "refused", e.value.code, e.value.counters, "model", wc)
        assert e.value.code == L.SS_EIO and e.value.counters["already_tagged"] == wc[3]
        assert L.bam_tag_calls() == calls + 1
        return None, wc, wd
    got, c, d, h, km = L.bam_tag(stream, T.db, T.row_node, T.parent, m, T.value, pairs, tags, want_counts=True)
    assert L.bam_tag_calls() == calls + 1
    gc = [c[x] for x in L.BAM_TAG_COUNTERS]
    print(say, "M", m, "pairs", pairs, "counters", gc, "model", wc, "bytes", len(got), len(want))
    assert gc == wc
    assert len(got) == len(want) == len(stream) - bam_pairs_model.header_end(stream) + 14 * wc[1]
    assert got == want
    assert (d == wd).all() and (h == wh).all() and (km == wk).all()
    assert int(d.sum()) == wc[4]
    return got, wc, wd


def tags_of(body, tags=b"snsc"):
    return bam_tag_model.read_tags(body, tags)


# ------------------------------------------------------------------------------------------------
# edge sizes, alignments
# ------------------------------------------------------------------------------------------------
def mixed(genome, n, seed):
    """n records: kept ones of the nodes and cold ones, secondary / supplementary records and records without bases mixed in"""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        ln = int(rs.randint(31, 120))
        seq = of_node(genome, 1 + (i // 2) % 9, 2 * int(rs.randint(0, 1900)), ln) if i % 3 else cold(rs, ln)
        flag = (4, 4, 0x10, 0x100, 4, 0x800 | 0x10, 4)[i % 7]
        if i % 11 == 5:
            seq = ""
        out.append(R("m%d" % i, bamio.revcomp(seq) if flag & 0x10 else seq, flag=flag, qual=qual_of(rs, len(seq)), aux=aux_exact(rs, int(rs.randint(0, 41)))))
    return HDR + b"".join(out)


def test_edge_sizes(L, T, genome):
    rs = np.random.RandomState(3)
    assert check(L, T, HDR, say="header only")[1] == [0, 0, 0, 0, 0, 0]
    got, wc, _ = check(L, T, HDR + R("only", of_node(genome, 4, 100, 150)), say="one kept record")
    assert wc == [1, 1, 1, 0, 1, 0] and tags_of(got) == [(4, b"only", 104, 60)]
    got, wc, _ = check(L, T, HDR + R("only", of_node(genome, 4, 100, 150), flag=0x100, aux=b"snA!"), say="one record that is not kept")
    assert wc == [1, 0, 0, 0, 0, 0] and got == R("only", of_node(genome, 4, 100, 150), flag=0x100, aux=b"snA!")
    got, wc, _ = check(L, T, HDR + R("cold", cold(rs)), say="one cold record")
    assert wc == [1, 1, 0, 0, 1, 0] and tags_of(got) == [(4, b"cold", -1, 0)]
    for n in (255, 256, 257):
        _, wc, wd = check(L, T, mixed(genome, n, n), say="%d records" % n)
        assert wc[0] == n and 0 < wc[2] < wc[1] < n and wd[1:].all()


def test_every_alignment_of_a_record_and_of_its_end(L, T, genome):
    """name lengths 1..40 x aux lengths 0..40: every D mod 16 and every E mod 16, for tagged and for untagged records"""
    rs = np.random.RandomState(9)
    recs = []
    for i in range(41 * 8):
        name = "n" * (1 + i % 40)
        seq = of_node(genome, 1 + i % 9, 2 * (i % 1000), 60 + i % 2) if i % 2 else cold(rs, 33 + i % 5)
        recs.append(R(name, seq, flag=0x100 if i % 5 == 3 else 4, aux=aux_exact(rs, i % 41)))
    s = HDR + b"".join(recs)
    off = bam_tag_model.offsets(s)
    for kept in (True, False):
        assert {d % 16 for d, e, k in off if k == kept} == set(range(16)), kept
        assert {e % 16 for d, e, k in off if k == kept} == set(range(16)), kept
    check(L, T, s, say="alignments")


# ------------------------------------------------------------------------------------------------
# classification
# ------------------------------------------------------------------------------------------------
def class_stream(genome):
    rs = np.random.RandomState(21)
    g = lambda v, off, n: of_node(genome, v, off, n)      # noqa: E731
    recs = [
        R("leaf4", g(4, 0, 150)),                                             # 0
        R("tie_in_tree", g(4, 200, 40) + "N" + g(5, 200, 40)),                # 1: 5 hits each -> their parent 2
        R("tie_across", g(4, 400, 40) + "N" + g(8, 400, 40)),                 # 2: -> 0, from a tie
        R("path", g(1, 0, 60) + "N" + g(2, 0, 50) + "N" + g(5, 0, 40)),       # 3: 15 + 10 + 5 on one path -> 5, score 30
        R("below_m", g(6, 600, 38)),                                          # 4: 4 hits < 5 -> -1, sc 4
        R("rc", bamio.revcomp(g(9, 800, 150)), flag=0x10),                    # 5
        R("rc_stored_forward", g(9, 1000, 150), flag=0x10),                   # 6: the flat form is the reverse complement: no hit
        R("iupac", "".join("MRWSYKVHDB="[i % 11] if i % 50 == 40 else c for i, c in enumerate(g(3, 0, 150)))),      # 7
        R("n_mid", g(7, 0, 75) + "N" + g(7, 76, 74)),                         # 8
        R("nobody", genome[36100:36250].decode()),                            # 9: hits, none with a node -> -1, sc 0
        R("cold", cold(rs)),                                                  # 10
        R("short", g(2, 100, 30)),                                            # 11: no window
    ]
    return HDR + b"".join(recs)


def test_classification_cases(L, T, genome):
    s = class_stream(genome)
    got, wc, wd = check(L, T, s, m=5, say="classes")
    t = {name: (sn, sc) for _, name, sn, sc in tags_of(got)}
    assert t[b"leaf4"] == (104, 60)
    assert t[b"tie_in_tree"] == (102, 5)
    assert t[b"tie_across"] == (-1, 5)
    assert t[b"path"] == (105, 30)
    assert t[b"below_m"] == (-1, 4)
    assert t[b"rc"] == (109, 60) and t[b"rc_stored_forward"] == (-1, 0)       # (the table holds one strand)
    assert t[b"iupac"][0] == 103 and 0 < t[b"iupac"][1] < 60
    assert t[b"n_mid"] == (2000000007, 23 + 22)
    assert t[b"nobody"] == (-1, 0) and t[b"cold"] == (-1, 0) and t[b"short"] == (-1, 0)
    assert wc[5] == 2                                                  # both ties count, the one across trees too
    got, wc, _ = check(L, T, s, m=1, say="classes, M 1")
    assert dict((n, sn) for _, n, sn, _ in tags_of(got))[b"below_m"] == 106
    got, wc, _ = check(L, T, s, m=31, say="classes, M 31")
    t = {name: (sn, sc) for _, name, sn, sc in tags_of(got)}
    assert t[b"path"] == (-1, 30) and t[b"leaf4"] == (104, 60)        # the score is reported below M too


def test_base_quality_mask(L, T, genome):
    rs = np.random.RandomState(4)
    holes = bytes([5 if i % 20 == 10 else 35 for i in range(150)])     # no window of 31 bases survives the mask
    g = lambda v: of_node(genome, v, 2 * int(rs.randint(0, 1900)), 150)      # noqa: E731
    s = HDR + b"".join([R("clean", g(4), qual=bytes([35] * 150)), R("holes", g(5), qual=holes),
                        R("holes_rc", bamio.revcomp(g(6)), flag=0x10, qual=holes), R("no_qual", g(8), qual=b"\xff" * 150),
                        R("low_tail", g(9), qual=bytes([35] * 100 + [3] * 50))])
    assert check(L, T, s, say="mask off")[1][2] == 5
    L.set_min_base_qual(20)
    try:
        got, wc, _ = check(L, T, s, min_qual=20, say="mask 20")
        t = {name: (sn, sc) for _, name, sn, sc in tags_of(got)}
        assert wc[2] == 3 and t[b"holes"] == (-1, 0) and t[b"holes_rc"] == (-1, 0) and t[b"no_qual"] == (108, 60) and t[b"low_tail"] == (109, 35)
    finally:
        L.set_min_base_qual(0)
    assert check(L, T, s, say="mask off again")[1][2] == 5


def test_long_record_and_a_record_of_nine_nodes(L, T, genome):
    """both leave the per-thread path of classify_kernel for classify_long_kernel: more than CLS_LONG = 4096 positions, more than
    CLS_CAP = 8 distinct nodes"""
    rs = np.random.RandomState(6)
    nine = "N".join(of_node(genome, v, 2 * v, 40 + 2 * v) for v in range(1, 10))
    eight = "N".join(of_node(genome, v, 2 * v, 40 + 2 * v) for v in range(2, 10))
    recs = [R("a", of_node(genome, 3, 0, 100)), R("long5000", genome[3000:8000].decode(), aux=aux_exact(rs, 23)), R("b", cold(rs)),
            R("nine", nine, aux=aux_exact(rs, 7)), R("eight", eight), R("long_cold", cold(rs, 5000)),
            R("long5000_rc", bamio.revcomp(genome[3000:8000].decode()), flag=0x10)]
    got, wc, _ = check(L, T, HDR + b"".join(recs), say="long, nine nodes")
    t = {name: (sn, sc) for _, name, sn, sc in tags_of(got)}
    assert t[b"long5000"] == (102, 500 + 2000 - 15) and t[b"long5000_rc"] == t[b"long5000"]      # node 1's last 1000 bases, all of node 2's
    assert t[b"long_cold"] == (-1, 0)
    # node v has 5 + v hits: the path 7-9 scores 12 + 14, more than 1-3-6 with 6 + 8 + 11
    assert t[b"nine"] == (109, 26) and t[b"eight"] == (109, 26)


def test_forest_of_4100_nodes(L, T, genome):
    """n_nodes + 1 >= CLS_LDS = 4096: direct[] and node_hits[] are added up with global atomics"""
    n = 4100
    parent = np.arange(n + 1, dtype=np.uint32) // 2                    # a binary heap: 1 is the root, parent[v] = v / 2
    parent[1] = 0
    parent[4000] = 0                                                   # ... and a second tree of one node
    node_of_stretch = np.array([4099, 2049, 1024, 4098, 3000, 4000, 1, 0, 4100, 0], np.uint32)      # 4099 - 2049 - 1024 is a path
    t2 = types.SimpleNamespace(db=T.db, keys=T.keys, row_node=node_of_stretch[np.minimum(T.stretch, 9)], parent=parent, n=n,
                               value=(np.arange(n + 1, dtype=np.int64) * 1000 - 1).astype(np.int32), stretch=T.stretch)
    rs = np.random.RandomState(8)
    g = lambda st, off, ln: of_node(genome, st + 1, off, ln)      # noqa: E731
    recs = [R("leaf", g(0, 0, 150)), R("up", g(0, 200, 40) + "N" + g(1, 200, 60) + "N" + g(2, 200, 80)),
            R("siblings", g(0, 400, 40) + "N" + g(3, 400, 40)), R("trees", g(5, 0, 50) + "N" + g(4, 0, 50)), R("root", g(6, 0, 100)),
            R("cold", cold(rs)), R("deep", g(8, 0, 90))] + [R("f%d" % i, g(i % 9, 2 * i, 60 + i % 40)) for i in range(300)]
    got, wc, wd = check(L, t2, HDR + b"".join(recs), say="4100 nodes")
    t = {name: (sn, sc) for _, name, sn, sc in tags_of(got)}
    assert t[b"leaf"] == (4099 * 1000 - 1, 60) and t[b"up"] == (4099 * 1000 - 1, 5 + 15 + 25)
    assert t[b"siblings"] == (2049 * 1000 - 1, 5) and t[b"trees"] == (-1, 10) and t[b"root"] == (999, 35) and t[b"deep"] == (4100 * 1000 - 1, 30)
    assert wd[4100] and wd[4099] and wd[4000] and wd[1]


# ------------------------------------------------------------------------------------------------
# aux fields in front of the appended tags
# ------------------------------------------------------------------------------------------------
EVERY_TYPE = (b"XAAs" + b"XccS" + b"XCCn" + b"XssSN" + b"XSSsn" + b"XiisnSC" + b"XIIscsn" + b"XffSNSC" + b"XZZsnsc snZ\0" + b"XHH5A\0" + b"XzZ\0" +
              b"".join(b"Y" + sub + b"B" + sub + struct.pack("<I", c) + b"sn" * (c * size // 2) + b"s" * (c * size % 2)
                       for sub, size in ((b"c", 1), (b"C", 1), (b"s", 2), (b"S", 2), (b"i", 4), (b"I", 4), (b"f", 4)) for c in (0, 1, 3)))


def test_aux_fields_of_every_type(L, T, genome):
    assert bam_tag_model.aux_walk(EVERY_TYPE, b"snsc") == 0 and len(bam_tag_model.aux_fields(EVERY_TYPE)) == 11 + 21
    hot = of_node(genome, 4, 0, 100)
    s = HDR + R("every", hot, aux=EVERY_TYPE) + R("none", hot) + R("sn_not_kept", hot, flag=0x800, aux=b"sni!\0\0\0sci\1\0\0\0") + \
        R("inside_z", hot, aux=b"XZZsnA!\0") + R("every_again", hot, aux=EVERY_TYPE * 3)
    got, wc, _ = check(L, T, s, say="every type")
    assert wc[:4] == [5, 4, 4, 0]
    assert tags_of(got)[2][2:] == (ord("!"), 1)                       # the record that is not kept keeps its own sn and sc
    assert [x[2:] for i, x in enumerate(tags_of(got)) if i != 2] == [(104, 35)] * 4
    got, wc, _ = check(L, T, s, tags=b"XaXb", say="custom tags")
    assert [x[2:] for i, x in enumerate(tags_of(got, b"XaXb")) if i != 2] == [(104, 35)] * 4


@pytest.mark.parametrize("bearing,count", [((b"snA!",), 1), ((b"sci\1\0\0\0", b"XAAx" + b"snZabc\0", EVERY_TYPE + b"scCx"), 3),
                                           ((b"snA!" + b"scA!",), 1)])
def test_a_kept_record_that_bears_a_tag(L, T, genome, bearing, count):
    hot = of_node(genome, 4, 0, 100)
    recs = [R("a", hot), R("b", hot, aux=b"XAAx")] + [R("t%d" % i, hot, aux=a) for i, a in enumerate(bearing)] + [R("c", hot, aux=EVERY_TYPE)]
    got, wc, _ = check(L, T, HDR + b"".join(recs), say="bears a tag")
    assert got is None and wc[3] == count
    got, wc, _ = check(L, T, HDR + b"".join(recs), tags=b"XaXb", say="... under other tags")      # (XA, Xa: the case counts)
    assert got is not None


@pytest.mark.parametrize("aux", [b"XXz1234", b"XX\0", b"XZZabc", b"XHH0A", b"XBBi\5\0\0\0" + b"x" * 19, b"XBBA\1\0\0\0x", b"XBBs\xff\xff\xff\xff" + b"ab",
                                 b"XiIabc", b"XA", b"X", b"XAAxY", b"XBBc\1\0"])
def test_damaged_aux_fields(L, T, genome, aux):
    hot = of_node(genome, 4, 0, 100)
    assert bam_tag_model.aux_walk(aux, b"snsc") == 2
    for recs in ([R("d", hot, aux=aux)], [R("a", hot), R("d", hot, aux=EVERY_TYPE + aux), R("b", hot)],
                 [R("t", hot, aux=b"snA!"), R("d", hot, aux=aux)]):                                # damaged wins over a tagged record
        got, wc, _ = check(L, T, HDR + b"".join(recs), say="damaged %r" % aux)
        assert got is None and wc[3] == 0
    check(L, T, HDR + R("d", hot, flag=0x100, aux=aux) + R("a", hot), say="not kept: not walked")


# ------------------------------------------------------------------------------------------------
# pairs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257])
def test_pairs_on_the_streams_of_the_mate_link(L, T, n):
    s = well_formed(bam_pairs_cases.stream(n), seed=n)
    got, wc, _ = check(L, T, s, pairs=True, say="pairs %d" % n)
    assert wc[0] == n
    check(L, T, s, pairs=False, say="plain %d" % n)
    if n >= 255:
        assert wc[4] < wc[1] < n
        by_name = {}
        for flag, name, sn, sc in tags_of(got):
            if not flag & 0x900 and flag & 0x1 and sn is not None:
                by_name.setdefault(name, []).append((sn, sc))
        assert sum(1 for v in by_name.values() if len(v) == 2) >= 100 and all(len(set(v)) == 1 for v in by_name.values())


def test_pairs_classify_the_fragment(L, T, genome):
    g = lambda v, off, n: of_node(genome, v, off, n)      # noqa: E731
    rs = np.random.RandomState(12)
    far = [R("f%d" % i, cold(rs, 60), aux=aux_exact(rs, i % 41)) for i in range(300)]
    recs = [R("leaves", g(4, 0, 36), flag=0x41), R("below", bamio.revcomp(g(6, 0, 34)), flag=0x81 | 0x10)] + far[:150] + \
           [R("orphan", g(8, 0, 100), flag=0x81), R("single", g(9, 0, 100), flag=0), R("leaves", g(4, 100, 36), flag=0x100 | 0x81)] + far[150:] + \
           [R("below", bamio.revcomp(g(6, 100, 36)), flag=0x41 | 0x10), R("leaves", g(5, 0, 36), flag=0x81)]
    s = HDR + b"".join(recs)
    def by_name(got):
        t = {}
        for _, name, sn, sc in tags_of(got):
            t.setdefault(name, []).append((sn, sc))
        return t

    got, wc, _ = check(L, T, s, m=3, pairs=True, say="pairs: the fragment, M 3")
    t = by_name(got)
    assert t[b"leaves"] == [(102, 3), (None, None), (102, 3)]          # 3 hits each -> their parent, from a tie; the secondary record is not kept
    assert t[b"orphan"] == [(108, 35)] and t[b"single"] == [(109, 35)]
    assert wc[4] == wc[1] - 2 and wc[5] == 1
    got, wc, _ = check(L, T, s, m=5, pairs=True, say="pairs: the fragment, M 5")
    t = by_name(got)
    assert t[b"below"] == [(106, 5), (106, 5)]                         # 2 + 3 hits reach M = 5 together
    assert t[b"leaves"] == [(-1, 3), (None, None), (-1, 3)] and wc[5] == 0
    got, wc, _ = check(L, T, s, m=5, pairs=False, say="the same stream, by record")
    t = by_name(got)
    assert t[b"leaves"] == [(-1, 3), (None, None), (-1, 3)] and t[b"below"] == [(-1, 2), (-1, 3)]
    got, wc, _ = check(L, T, s, m=3, pairs=False, say="... M 3")
    t = by_name(got)
    assert t[b"leaves"] == [(104, 3), (None, None), (105, 3)]          # alone, the mates go to two different leaves
    assert t[b"below"] == [(-1, 2), (106, 3)]


@pytest.mark.parametrize("shape", ["three_of_one_name", "two_of_role_1", "role_0_shares_a_name", "one_name_257"])
def test_pairs_violations(L, T, shape):
    s = well_formed(bam_pairs_cases.violating()[shape])
    got, wc, _ = check(L, T, s, pairs=True, say=shape)
    assert got is None
    assert check(L, T, s, pairs=False, say=shape + ", plain")[0] is not None


# ------------------------------------------------------------------------------------------------
# a seeded mix
# ------------------------------------------------------------------------------------------------
def seeded_records(genome, seed, n):
    """n templates, shuffled: singles, pairs (mates anywhere), orphans, secondary / supplementary decoys under a template's name,
    records without bases, 0x10 records, IUPAC codes, records without qualities, aux fields of 0..40 bytes, a CIGAR or none"""
    rs = np.random.RandomState(seed)
    out = []
    for t in range(n):
        name = "t%d" % t
        kind = int(rs.randint(0, 10))                                  # 0..3 single, 4..8 pair, 9 orphan
        for m in range(2 if 4 <= kind <= 8 else 1):
            ln = int(rs.randint(20, 200))
            r = rs.random_sample()
            if r < 0.5:
                v = 1 + int(rs.randint(0, 9))
                seq = of_node(genome, v, 2 * int(rs.randint(0, 1900)), ln)
                if rs.random_sample() < 0.3:                           # ... spliced with another node's bases
                    w = 1 + int(rs.randint(0, 9))
                    seq = seq[:ln // 2] + of_node(genome, w, 2 * int(rs.randint(0, 1900)), ln - ln // 2)
            elif r < 0.8:
                seq = cold(rs, ln)
            else:
                seq = genome[36000 + 2 * int(rs.randint(0, 1800)):][:ln].decode()
            if rs.random_sample() < 0.1:
                j = int(rs.randint(0, ln))
                seq = seq[:j] + "NMRWY="[int(rs.randint(0, 6))] + seq[j + 1:]
            flag = 4 if kind < 4 else 0x1 | (0x40 if m == 0 else 0x80) if kind < 9 else 0x1 | (0x40, 0x80, 0, 0xC0)[int(rs.randint(0, 4))]
            if rs.random_sample() < 0.3:
                flag |= 0x10
            q = b"\xff" * ln if rs.random_sample() < 0.03 else qual_of(rs, ln)
            out.append(R(name, seq, flag=flag, qual=q, aux=aux_exact(rs, int(rs.randint(0, 41))), cigar=((ln << 4),) if rs.random_sample() < 0.5 else ()))
        if rs.random_sample() < 0.1:
            out.append(R(name, of_node(genome, 3, 0, 100), flag=(0x100 if rs.random_sample() < 0.5 else 0x800 | 0x10) | (0x41 if kind >= 4 else 0),
                         aux=b"snA!" if rs.random_sample() < 0.5 else b""))
        if rs.random_sample() < 0.03:
            out.append(R(name, "", flag=0x41 if kind >= 4 else 4))
    return [out[i] for i in rs.permutation(len(out))]


@pytest.fixture(scope="module")
def big_stream(genome):
    recs = seeded_records(genome, 7, 3000)
    assert 4500 <= len(recs) <= 5500
    return HDR + b"".join(recs)


@pytest.mark.parametrize("pairs", [False, True])
def test_seeded_mix_equals_the_model(L, T, big_stream, pairs):
    got, wc, wd = check(L, T, big_stream, m=8, pairs=pairs, say="seeded")
    assert wc[0] > wc[1] >= 4000 and 0 < wc[2] < wc[1] and wc[5] > 0 and wd.all()
    assert (wc[4] < wc[1]) == pairs


def test_host_walk_serves_a_stream_the_device_walk_declines(L, T, big_stream):
    L.check(L.lib().ss_test_hook(7, 1), "hook")
    try:
        check(L, T, big_stream, m=8, pairs=True, say="host walk")
    finally:
        L.check(L.lib().ss_test_hook(7, 0), "hook")


def test_tags_equal_the_resident_sets_classes(L, T, big_stream):
    """sn of the kept records, in order, = node_value[class] of ReadSet.classify(want_classes=True) on the flat block of the same
    stream; direct is equal"""
    flat, n_reads = bamio.flat(bamio.decode(big_stream))
    d = C.c_void_p()
    L.check(L.lib().ss_dev_alloc(C.byref(d), len(flat)), "ss_dev_alloc")
    try:
        L.check(L.lib().ss_memcpy_h2d(d, flat, len(flat), None), "ss_memcpy_h2d")
        L.check(L.lib().ss_device_sync(), "sync")
        rset = L.ReadSet.from_flat_dev(d.value, len(flat), order=False)
        try:
            L.check(L.lib().ss_device_sync(), "sync")
            res = rset.classify(T.db, T.row_node, T.parent, 8, want_classes=True)
        finally:
            rset.close()
    finally:
        L.check(L.lib().ss_dev_free(d), "ss_dev_free")
    got, c, direct, _, _ = L.bam_tag(big_stream, T.db, T.row_node, T.parent, 8, T.value, want_counts=True)
    sn = [x[2] for x in tags_of(got) if x[2] is not None and not x[0] & 0x900]
    assert len(sn) == n_reads == c["tagged"] == len(res["classes"])
    assert sn == [int(T.value[k]) for k in res["classes"]]
    assert (direct == res["direct"]).all() and c["ties"] == res["ties"]
    sc = [x[3] for x in tags_of(got) if x[2] is not None and not x[0] & 0x900]
    assert all((s >= 8) or k == 0 for s, k in zip(sc, res["classes"]))


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def test_refusals(L, T, genome):
    s = class_stream(genome)
    want, wc = bam_tag_model.model(s, T.keys, T.row_node, T.parent, T.n, K, 5, T.value)[:2]

    def code(**kw):
        a = dict(stream=s, kdb=T.db, row_node=T.row_node, parent=T.parent, m=5, node_value=T.value)
        a.update(kw)
        with pytest.raises(L.SSError) as e:
            L.bam_tag(**a)
        return e.value.code

    flat = L.KmerDB.from_text(_kfa([genome[i:i + 15] for i in range(0, 3000, 16)]), 15, True)
    try:
        assert code(kdb=flat, row_node=np.zeros(flat.n_rows, np.uint32)) == L.SS_ERANGE
    finally:
        flat.close()
    assert code(m=0) == L.SS_EINVAL
    assert code(parent=np.zeros(1, np.uint32), node_value=np.zeros(1, np.int32)) == L.SS_EINVAL                     # no node
    assert code(row_node=T.row_node + 1) == L.SS_EINVAL                                                              # a row node above n_nodes
    assert code(parent=np.array([0, 0, 1, 1, 2, 2, 3, 0, 7, 10], np.uint32)) == L.SS_EINVAL                           # a parent above n_nodes
    assert code(parent=np.array([0, 2, 1, 1, 2, 2, 3, 0, 7, 7], np.uint32)) == L.SS_EINVAL                            # a cycle
    for tags in (b"snsn", b"1asc", b"sn1c", b"s_sc", b"sns-", b"\0nsc"):
        assert code(tags=tags) == L.SS_EINVAL, tags
    for tags in (b"s1s2", b"SNsn", b"Z9z0"):
        assert L.bam_tag(s, T.db, T.row_node, T.parent, 5, T.value, tags=tags)[0] == \
            bam_tag_model.model(s, T.keys, T.row_node, T.parent, T.n, K, 5, T.value, tags)[0]
    for cut in (1, 7, 40):
        assert code(stream=s[:-cut]) == L.SS_EIO
    assert code(stream=b"BAX\1" + s[4:]) == L.SS_EIO
    # NULL arguments; cap too small: SS_ERANGE, *out_len exact, the counters set
    out = np.zeros(len(want), np.uint8)
    n, c = C.c_uint64(), (C.c_uint64 * 6)()
    args = [s, len(s), T.db.handle, L.ptr(T.row_node), 9, L.ptr(T.parent), 5, L.ptr(T.value), b"snsc", 0, L.ptr(out), len(want), C.byref(n), c,
            None, None, None]
    for i in (0, 2, 3, 5, 7, 8, 10, 12, 13):
        a = list(args)
        a[i] = None
        assert L.lib().ss_bam_tag_stream(*a) == L.SS_EINVAL, i
    for n_nodes in (0, 65536):
        a = list(args)
        a[4] = n_nodes
        assert L.lib().ss_bam_tag_stream(*a) == L.SS_EINVAL
    for cap in (0, len(want) - 1):
        a = list(args)
        a[11] = cap
        assert L.lib().ss_bam_tag_stream(*a) == L.SS_ERANGE and n.value == len(want) and list(c) == wc
        assert not out.any()
    assert L.lib().ss_bam_tag_stream(*args) == 0 and out.tobytes() == want and n.value == len(want)
    assert L.lib().ss_bam_tag_calls(None) == L.SS_EINVAL and L.lib().ss_bam_tag_timing(None) == L.SS_EINVAL


# ------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------
def _records_of(stream):
    return [stream[r["at"]:r["at"] + r["size"]] for r in bam_pairs_model.walk(stream)]


@pytest.mark.parametrize("big", [True, False])
def test_file_above_and_below_1_mb(L, T, genome, big_stream, tmp_path, big):
    import gzip
    rs = np.random.RandomState(15)
    stream = big_stream
    if big:                                                            # six long records: the file passes 1 MB
        recs = _records_of(big_stream)
        for i in range(6):
            recs.insert(700 * i + 17, R("long%d" % i, cold(rs, 150000) if i else genome[:35000].decode() + cold(rs, 115000), qual=qual_of(rs, 150000),
                                         aux=aux_exact(rs, 30)))
        stream = HDR + b"".join(recs)
    p, out = tmp_path / "in.bam", tmp_path / "out.bam"
    p.write_bytes(bamio.bgzf(HDR, _records_of(stream), level=1))
    assert (p.stat().st_size > (1 << 20)) == big
    want, wc, wd, wh, _ = bam_tag_model.model(stream, T.keys, T.row_node, T.parent, T.n, K, 8, T.value, pairs=big)
    before, calls = L.bam_counters(), L.bam_tag_calls()
    c, d, h, _ = L.bam_tag_file(str(p), T.db, T.row_node, T.parent, 8, T.value, str(out), pairs=big, want_counts=True)
    after = L.bam_counters()
    assert L.bam_tag_calls() == calls + 1
    assert after["device" if big else "host"] == before["device" if big else "host"] + 1
    assert [c[x] for x in L.BAM_TAG_COUNTERS] == wc and (d == wd).all() and (h == wh).all()
    assert sorted(os.listdir(tmp_path)) == ["in.bam", "out.bam"]      # no .tmp is left
    data = out.read_bytes()
    assert data.endswith(bamio.EOF) and gzip.decompress(data) == HDR + want
    assert bamio.decode(data) == bamio.decode(stream)
    tm = L.bam_tag_timing()
    print(tm)
    assert tm["total"] > 0 and tm["classify"] > 0 and (tm["mates_join"] > 0) == big
    # a record that bears a tag: SS_EIO and no file, the one that stood there stays
    recs = _records_of(stream)
    recs[5] = R("bears", of_node(genome, 4, 0, 100), aux=b"XAAx" + b"sci\7\0\0\0")
    p.write_bytes(bamio.bgzf(HDR, recs, level=1))
    other = tmp_path / "other.bam"
    with pytest.raises(L.BamTagError) as e:
        L.bam_tag_file(str(p), T.db, T.row_node, T.parent, 8, T.value, str(other), pairs=big)
    assert e.value.code == L.SS_EIO and e.value.counters["already_tagged"] == 1
    assert sorted(os.listdir(tmp_path)) == ["in.bam", "out.bam"]
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    with pytest.raises(L.SSError) as e:
        L.bam_tag_file(str(fq), T.db, T.row_node, T.parent, 8, T.value, str(other))
    assert e.value.code == L.SS_EINVAL and not other.exists()
