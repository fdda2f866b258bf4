"""The inputs of tests/test_binning_general_gpu.py, built here and held to the geometry they claim -- on the CPU, through
tests/binmodel.py alone: the newline really sits at tile0 + 16384 + 511, the tile really has 129 record starts, the tile really
goes to the kernel the case is about.  No case is a candidate for the one-length paths, so ss_reorder.hip's general passes
(count_kernel, place_kernel, place_again_kernel) are entered directly.  The model is held to itself as well: the slab it builds
parses back into the records it was built from, and a slab with a record dropped, a slot shifted or a pad byte overwritten does not.

CASES maps a case's name to its builder; case(name) builds it once per process.  A case is (block, facts): facts["tile"] is the
tile the case is about, the rest is what its family's test asserts.  Every family but F to I exists once with that tile being
tile 0 (suffix "0") and once behind full filler tiles (suffix "+")."""
import functools

import numpy as np
import pytest

from tests import binmodel as bm
from tests.binmodel import RB, CH, HALO, TCAP, LEN_LIMIT, PRE_PIECES

GENOME = np.frombuffer(b"ACGT", np.uint8)[np.random.RandomState(20261).randint(0, 4, size=300000)]
SHIFTS = {"0": 0, "+": 2 * RB}          # where the tile a case is about begins


class _Block:
    """A flat block under construction: records cut from GENOME, each followed by a newline."""
    def __init__(self, seed):
        self.rs, self.parts, self.pos, self.k = np.random.RandomState(seed), [], 0, 0

    def cut(self, length):
        s = int(self.rs.randint(0, len(GENOME) - length))
        return GENOME[s:s + length].tobytes()

    def raw(self, b):
        self.parts.append(b)
        self.pos += len(b)

    def rec(self, r):
        self.raw((self.cut(r) if isinstance(r, int) else r) + b"\n")

    def filler(self, length=None):
        """a ragged record, 100..200 bases unless told; every 13th with an N behind its first k-mer, every 29th with one in it"""
        r = self.cut(int(self.rs.randint(100, 201)) if length is None else length)
        self.k += 1
        if self.k % 13 == 0 and len(r) > 41:
            r = r[:40] + b"N" + r[41:]
        if self.k % 29 == 0 and len(r) > 41:
            r = r[:7] + b"N" + r[8:]
        self.rec(r)

    def fill_to(self, off):
        """fillers up to exactly `off`: the last one or two are adjusted (100..201 bytes each when the gap allows it)"""
        assert off == self.pos or off - self.pos >= 2, (off, self.pos)
        while off - self.pos > 402:
            self.filler()
        if off - self.pos > 201:
            self.filler((off - self.pos) // 2 - 1)
        if off > self.pos:
            self.filler(off - self.pos - 1)
        assert self.pos == off

    def done(self, tail=3, final=b""):
        """`tail` fillers behind everything (more while the block would be a candidate for the one-length paths), then `final`"""
        for _ in range(tail):
            self.filler()
        while bm.one_length_candidate(b"".join(self.parts) + final) is not None:
            self.filler()
        return b"".join(self.parts) + final


def place(seed, items, tail=3):
    """A block in which chosen records start at chosen absolute offsets: items = [(offset or None, record), ...] in ascending
    order; a record is its bytes or a length (cut from GENOME); offset None: directly behind the item before.  Ragged fillers
    in between, `tail` of them behind the last item."""
    b = _Block(seed)
    for off, r in items:
        if off is not None:
            b.fill_to(off)
        b.rec(r)
    return b.done(tail)


# ---- A: a record that starts / ends at T - 1, T, T + 1, T the end of the tile the case is about ---------------------------------
def _a_start(delta, shift):
    T = shift + RB
    return place(100 + delta, [(T + delta, 150)]), dict(tile=shift // RB, T=T, start=T + delta, length=150)


def _a_end(delta, shift):
    T = shift + RB
    where = {-1: bm.TILE, 0: bm.HALO_END, 1: bm.HALO_END}[delta]
    return place(110 + delta, [(T + delta - 150, 150)]), dict(tile=shift // RB, T=T, start=T + delta - 150, length=150, newline=T + delta, ends=where)


# ---- B: a record of the tile whose newline is at tile0 + RB + d ------------------------------------------------------------------
B_D = (510, 511, 512, 513, 527, 528, 529)


def _b(d, start_at, shift, again=False):
    tile0 = shift
    start = tile0 + (RB - 1 if start_at == "last" else 70)
    nl = tile0 + RB + d
    items = [(start, nl - start)]
    if again:
        items = [(tile0 + 1000, b"ACGT"), (None, b"ACGT")] + items
    return place(200 + d, items), dict(tile=tile0 // RB, start=start, length=nl - start, newline=nl,
                                       ends=bm.HALO_END if d < HALO else bm.WALKED, path=bm.AGAIN if again else bm.TABLE)


# ---- C: long records ----------------------------------------------------------------------------------------------------------
def _c_span(shift):
    start = shift + 16000
    return place(301, [(start, 51200)]), dict(tile=shift // RB, start=start, length=51200, ends=bm.WALKED, empty_tiles=3, path=bm.TABLE)


def _c_30k(shift, again):
    start = shift + 15000
    items = [(start, 30720)]
    if again:
        items = [(shift + 1000, b"ACGT"), (None, b"ACGT")] + items
    return place(302, items), dict(tile=shift // RB, start=start, length=30720, ends=bm.WALKED, path=bm.AGAIN if again else bm.TABLE,
                                   min_starts=90, min_pieces=PRE_PIECES + 1)


# ---- D: 128 and 129 record starts in a tile, one per chunk at most ----------------------------------------------------------------
def _d(n_starts, shift):
    b = _Block(400 + n_starts)
    b.fill_to(shift)
    if n_starts == 128:
        for i in range(64):                     # 64 x (127 + 129) bytes = the tile
            b.rec(126)
            b.rec(128)
    else:
        for i in range(64):                     # 64 x (126 + 128) bytes, and the 129th start 128 bytes in front of the tile's end
            b.rec(125)
            b.rec(127)
        b.rec(150)
    return b.done(), dict(tile=shift // RB, starts=n_starts, per_chunk=1, path=bm.TABLE if n_starts == 128 else bm.AGAIN)


# ---- E: several record starts in one lane's chunk -------------------------------------------------------------------------------
def _e_two(shift):
    b = _Block(501)
    b.fill_to(shift)
    for r in (3000, 3000, 387, b"ACGT", b"ACGT", 3000, 3000, 4000):     # (the tiny ones fill the last 10 bytes of a chunk)
        b.rec(r)
    return b.done(), dict(tile=shift // RB, max_starts=10, per_chunk=2, path=bm.AGAIN, chunk=shift + 6336)


def _e_32(shift):
    b = _Block(502)
    b.fill_to(shift + 6400)
    b.raw(b"A\nC\nG\nT\n" * 8)
    return b.done(), dict(tile=shift // RB, per_chunk=32, path=bm.AGAIN, chunk=shift + 6400)


def _e_newlines(shift):
    b = _Block(503)
    b.fill_to(shift + 6400)
    b.raw(b"\n" * CH)
    return b.done(), dict(tile=shift // RB, per_chunk=1, path=bm.TABLE, chunk=shift + 6400, chunk_is=b"\n" * CH)


# ---- F: both placing kernels in one call -----------------------------------------------------------------------------------------
def _f():
    b = _Block(601)
    while b.pos < (1 << 20):
        stop = b.pos + 3 * RB
        while b.pos < stop:
            b.filler()
        stop = b.pos + 3 * RB
        while b.pos < stop:
            b.filler(int(b.rs.randint(20, 61)))
    return b.done(), dict(tile=0)


# ---- G: the buffer's edges ---------------------------------------------------------------------------------------------------------
def _g_small(n):
    b = _Block(700 + n)
    b.rec(20)                                   # (a first record below FIX_MIN_L: no candidate for the one-length paths)
    b.rec(n - 21 - 1)
    return b.done(0), dict(tile=0, n=n, records=2)


def _g_final(kind, n_fill):
    """n_fill fillers, then: "no_newline" a 150-base record without one; "31" a record of exactly 31 valid bases without a
    newline (start + 32 > n: the last bin); "31nl" the same with its newline (keyed)"""
    b = _Block(710 + n_fill)
    for _ in range(n_fill):
        b.filler()
    last = b.cut(150 if kind == "no_newline" else 31)
    block = b.done(0, last + (b"\n" if kind == "31nl" else b""))
    start = len(block) - len(last) - (1 if kind == "31nl" else 0)
    return block, dict(tile=start // RB, last=last, start=start, keyed=kind != "31", final_newline=kind == "31nl")


def _g_lead():
    b = _Block(721)
    b.raw(b"\n" * 70)
    return b.done(40), dict(tile=0, head=b"\n" * 70)


def _g_trail():
    b = _Block(722)
    for _ in range(40):
        b.filler()
    return b.done(0, b"\n" * 39), dict(tile=0, foot=b"\n" * 40)       # (the last filler's own newline is the first of the 40)


def _g_not16():
    b = _Block(723)
    for _ in range(40):
        b.filler()
    while b.pos % 16 == 0 or bm.one_length_candidate(b"".join(b.parts)) is not None:
        b.filler()
    return b"".join(b.parts), dict(tile=0, not16=True)


def _g_only_newlines():
    return b"\n" * 100, dict(tile=0, records=0)


# ---- H: the 26-bit length field ----------------------------------------------------------------------------------------------------
def _h():
    b = _Block(801)
    b.fill_to(2 * RB + 4000)
    head = b"".join(b.parts)
    rs = np.random.RandomState(802)
    lut = np.frombuffer(b"ACGT", np.uint8)
    longs = [lut[rs.randint(0, 4, size=n, dtype=np.uint8)] for n in (LEN_LIMIT - 1, LEN_LIMIT)]
    t = _Block(803)
    for _ in range(220):
        t.filler()
    first = head.find(b"\n")
    while (len(head) + 2 * LEN_LIMIT + 1 + t.pos) % (first + 1) < 64:      # (no candidate for the one-length paths)
        t.filler()
    nl = np.full(1, 10, np.uint8)
    block = np.concatenate([np.frombuffer(head, np.uint8), longs[0], nl, longs[1], nl, np.frombuffer(b"".join(t.parts), np.uint8)]).tobytes()
    s0 = len(head)
    return block, dict(tile=s0 // RB, starts_at=(s0, s0 + LEN_LIMIT), lengths=(LEN_LIMIT - 1, LEN_LIMIT))


# ---- I: a bin width above the minimum ----------------------------------------------------------------------------------------------
def _i(n_rec, seed):
    rs = np.random.RandomState(seed)
    lens = rs.randint(100, 201, size=n_rec)
    lens[5::211] = rs.randint(1, 31, size=len(lens[5::211]))           # shorter than a k-mer
    starts = rs.randint(0, len(GENOME) - 200, size=n_rec)
    recs = [GENOME[s:s + n].tobytes() for s, n in zip(starts.tolist(), lens.tolist())]
    for i in range(3, n_rec, 97):
        recs[i] = recs[i][:11] + b"N" + recs[i][12:]
    for i in range(7, n_rec, 89):
        recs[i] = recs[i][:5] + recs[i][5:25].lower() + recs[i][25:]
    block = b"\n".join(recs) + b"\n"
    while bm.one_length_candidate(block) is not None:
        block += GENOME[:int(rs.randint(100, 201))].tobytes() + b"\n"
    return block, dict(tile=0)


CASES = {}
for _s, _shift in SHIFTS.items():
    for _delta in (-1, 0, 1):
        CASES["A_start%+d_%s" % (_delta, _s)] = functools.partial(_a_start, _delta, _shift)
        CASES["A_end%+d_%s" % (_delta, _s)] = functools.partial(_a_end, _delta, _shift)
    for _d_ in B_D:
        for _at in ("last", "first"):
            CASES["B_%d_%s_%s" % (_d_, _at, _s)] = functools.partial(_b, _d_, _at, _shift)
    for _d_ in (511, 512):
        CASES["B_%d_last_again_%s" % (_d_, _s)] = functools.partial(_b, _d_, "last", _shift, True)
    CASES["C_span_" + _s] = functools.partial(_c_span, _shift)
    CASES["C_30k_table_" + _s] = functools.partial(_c_30k, _shift, False)
    CASES["C_30k_again_" + _s] = functools.partial(_c_30k, _shift, True)
    CASES["D_128_" + _s] = functools.partial(_d, 128, _shift)
    CASES["D_129_" + _s] = functools.partial(_d, 129, _shift)
    CASES["E_two_" + _s] = functools.partial(_e_two, _shift)
    CASES["E_32_" + _s] = functools.partial(_e_32, _shift)
    CASES["E_newlines_" + _s] = functools.partial(_e_newlines, _shift)
CASES["F_both_kernels"] = _f
for _n in (64, 65, 79):
    CASES["G_%d_bytes" % _n] = functools.partial(_g_small, _n)
for _kind in ("no_newline", "31", "31nl"):
    CASES["G_final_%s_0" % _kind] = functools.partial(_g_final, _kind, 30)
    CASES["G_final_%s_+" % _kind] = functools.partial(_g_final, _kind, 260)
CASES["G_leading_newlines"] = _g_lead
CASES["G_trailing_newlines"] = _g_trail
CASES["G_not_16"] = _g_not16
CASES["G_only_newlines"] = _g_only_newlines
CASES["H_length_field"] = _h
CASES["I_bits13"] = functools.partial(_i, 27000, 901)
CASES["I_bits14"] = functools.partial(_i, 40000, 902)

LARGE = ("H_length_field",)                     # the one case whose records the pure-Python code must keep away from


@functools.lru_cache(maxsize=None)
def case(name):
    block, facts = CASES[name]()
    return block, facts


def family(letter):
    return [n for n in CASES if n.startswith(letter + "_")]


def _record_at(block, start):
    lay = bm.layout(block)
    i = int(np.searchsorted(lay["start"], start))
    assert i < len(lay) and lay["start"][i] == start, ("no record starts at", start)
    return i, lay


# ---- what every case must be ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_case_enters_the_general_passes_and_the_model_holds_on_it(name):
    """No one-length candidate, at least the 64 bytes below which nothing is binned; the records per bin partition the input;
    the slab the model builds has the model's length and parses back into exactly those records, in ascending bins."""
    block, facts = case(name)
    assert len(block) >= bm.MIN_BINNED
    assert bm.one_length_candidate(block) is None
    lay = bm.layout(block)
    want = bm.expected_slab(block)
    assert want["n_records"] == len(lay) and want["bits"] == bm.order_bits(len(block))
    assert sum(len(v) for v in want["per_bin"].values()) == len(lay)
    if name in LARGE:
        assert sorted(len(r) for v in want["per_bin"].values() for r in v) == sorted(lay["length"].tolist())
    else:
        assert sorted(r for v in want["per_bin"].values() for r in v) == sorted(r for r in block.split(b"\n") if r)
    assert want["total"] == int(lay["slot"].sum()) and want["slab_len"] % 16 == 0 and want["slab_len"] >= max(want["total"], 16)
    assert want["slab_len"] - want["total"] < 16 or want["total"] == 0
    slab, total = bm.build_slab(block)
    assert total == want["total"] and len(slab) == want["slab_len"]
    back = bm.parse_slab(slab, total)
    assert len(back) == len(lay)
    order = np.argsort(lay["bin"], kind="stable")
    recs = bm.records_of(block, lay)
    assert back == [recs[i] for i in order.tolist()]
    tiles, ends = bm.tile_facts(block)
    assert len(tiles) == (len(block) + RB - 1) // RB and len(ends) == len(lay)
    assert sum(t["starts"] for t in tiles) == len(lay)


def test_vectorised_bins_agree_with_bin_of():
    """bins_of_heads (what layout uses) against the scalar bin_of, on the ragged case with N and lower case in first k-mers."""
    block, _ = case("I_bits13")
    lay = bm.layout(block)
    bits = bm.order_bits(len(block))
    assert bits == 13
    recs = bm.records_of(block, lay)
    for i in range(0, len(recs), 7):
        assert lay["bin"][i] == bm.bin_of(recs[i], bits), i
    assert (lay["bin"] == 1 << bits).sum() > 100 and len(set(lay["bin"].tolist())) > 4000


# ---- the geometry each family claims ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", family("A"))
def test_a_tile_boundary(name):
    block, f = case(name)
    i, lay = _record_at(block, f["start"])
    assert lay["length"][i] == 150 and f["T"] % RB == 0 and f["T"] >= RB
    assert block[f["start"] - 1] == 10                          # (a start at T: the closing newline is the previous tile's last byte)
    if "newline" in f:
        assert block[f["newline"]] == 10 and f["newline"] == f["start"] + 150 and f["newline"] - f["T"] in (-1, 0, 1)
        assert bm.tile_facts(block)[1][i] == f["ends"]
        assert f["start"] // RB == f["tile"]
    else:
        assert f["start"] - f["T"] in (-1, 0, 1)
        assert f["start"] // RB == f["tile"] + (0 if f["start"] < f["T"] else 1)
        if f["start"] < f["T"]:                                 # one byte in the tile, the rest in the halo
            assert bm.tile_facts(block)[1][i] == bm.HALO_END


@pytest.mark.parametrize("name", family("B"))
def test_b_halo_edge(name):
    block, f = case(name)
    i, lay = _record_at(block, f["start"])
    tile0 = f["tile"] * RB
    d = f["newline"] - tile0 - RB
    assert d in B_D and name.startswith("B_%d_" % d)
    assert f["start"] // RB == f["tile"] and f["start"] - tile0 in (70, RB - 1)
    assert lay["length"][i] == f["length"] and block[f["newline"]] == 10 and b"\n" not in block[f["start"]:f["newline"]]
    tiles, ends = bm.tile_facts(block)
    assert ends[i] == f["ends"] == (bm.HALO_END if d <= HALO - 1 else bm.WALKED)
    assert tiles[f["tile"]]["path"] == f["path"]
    assert len(block) > f["newline"] + 200                      # (the walk ends at a newline, not at the buffer's end)


@pytest.mark.parametrize("name", family("C"))
def test_c_long_records(name):
    block, f = case(name)
    i, lay = _record_at(block, f["start"])
    tiles, ends = bm.tile_facts(block)
    t = f["tile"]
    assert f["start"] // RB == t and lay["length"][i] == f["length"] and ends[i] == f["ends"]
    assert tiles[t]["path"] == f["path"]
    if "empty_tiles" in f:
        assert [tiles[t + j]["starts"] for j in (1, 2, 3)] == [0, 0, 0] and tiles[t + 4]["starts"] > 0
        assert f["start"] + f["length"] > (t + 4) * RB
    else:
        assert tiles[t]["starts"] >= f["min_starts"] and tiles[t]["pieces"] >= f["min_pieces"]
        assert (tiles[t]["per_chunk"] > 1) == (f["path"] == bm.AGAIN) and tiles[t]["starts"] <= TCAP


@pytest.mark.parametrize("name", family("D"))
def test_d_table_capacity(name):
    block, f = case(name)
    tiles, _ = bm.tile_facts(block)
    t = tiles[f["tile"]]
    assert t["starts"] == f["starts"] and f["starts"] - TCAP in (0, 1)
    assert t["per_chunk"] == 1 and not t["big"] and t["path"] == f["path"]
    lay = bm.layout(block)
    mine = lay[(lay["start"] // RB) == f["tile"]]
    assert (mine["length"] + 1 >= CH).all() and len(set(mine["length"].tolist())) > 1


@pytest.mark.parametrize("name", family("E"))
def test_e_several_starts_in_one_chunk(name):
    block, f = case(name)
    tiles, _ = bm.tile_facts(block)
    t = tiles[f["tile"]]
    assert f["chunk"] % CH == 0 and f["chunk"] // RB == f["tile"]
    lay = bm.layout(block)
    in_chunk = int(((lay["start"] >= f["chunk"]) & (lay["start"] < f["chunk"] + CH)).sum())
    assert t["per_chunk"] == f["per_chunk"] and t["path"] == f["path"]
    if "chunk_is" in f:
        assert block[f["chunk"]:f["chunk"] + CH] == f["chunk_is"] and in_chunk == 0
        assert block[f["chunk"] - 2] != 10 and block[f["chunk"] + CH] != 10        # between two records
    else:
        assert in_chunk == f["per_chunk"]
    if "max_starts" in f:
        assert t["starts"] <= f["max_starts"]


def test_f_both_placing_kernels_share_bins():
    block, _ = case("F_both_kernels")
    assert 1 << 20 <= len(block) < (1 << 20) + 8 * RB
    lay = bm.layout(block)
    tiles, _ = bm.tile_facts(block)
    paths = np.array([t["path"] == bm.AGAIN for t in tiles])
    assert paths.sum() >= 10 and (~paths).sum() >= 10
    again = paths[lay["start"] // RB]
    shared = set(lay["bin"][again].tolist()) & set(lay["bin"][~again].tolist())
    assert len(shared) > 100 and (1 << bm.order_bits(len(block))) in shared
    assert (lay["length"][again] < 31).sum() > 100


@pytest.mark.parametrize("name", family("G"))
def test_g_buffer_edges(name):
    block, f = case(name)
    lay = bm.layout(block)
    bits = bm.order_bits(len(block))
    if "n" in f:
        assert len(block) == f["n"] and len(lay) == f["records"] == 2
    if "last" in f:
        assert block.endswith(f["last"] + (b"\n" if f["final_newline"] else b"")) and not f["last"].endswith(b"\n")
        assert lay["start"][-1] == f["start"] and lay["length"][-1] == len(f["last"]) and f["start"] // RB == f["tile"]
        assert (f["tile"] > 1) == name.endswith("+")
        if len(f["last"]) == 31:
            assert set(f["last"]) <= set(b"ACGT") and bm.bin_of(f["last"], bits) < 1 << bits
            assert (f["start"] + 32 <= len(block)) == f["keyed"]
            assert lay["bin"][-1] == (bm.bin_of(f["last"], bits) if f["keyed"] else 1 << bits)
            assert bm.expected_slab(block)["by_rule"] == ([] if f["keyed"] else [f["last"]])
    if "head" in f:
        assert block.startswith(f["head"]) and block[len(f["head"])] != 10 and lay["start"][0] == len(f["head"])
    if "foot" in f:
        assert block.endswith(f["foot"]) and block[-len(f["foot"]) - 1] != 10
    if "not16" in f:
        assert len(block) % 16 != 0
    if f.get("records") == 0:
        assert set(block) == {10} and len(block) >= 64 and len(lay) == 0
        assert bm.build_slab(block) == (b"\n" * 16, 0) and bm.expected_slab(block)["slab_len"] == 16


def test_h_length_field():
    block, f = case("H_length_field")
    assert 127 << 20 < len(block) < 130 << 20
    lay = bm.layout(block)
    tiles, ends = bm.tile_facts(block)
    for start, length, path in zip(f["starts_at"], f["lengths"], (bm.TABLE, bm.AGAIN)):
        i = int(np.searchsorted(lay["start"], start))
        assert lay["start"][i] == start and lay["length"][i] == length and ends[i] == bm.WALKED
        t = tiles[start // RB]
        assert t["path"] == path and t["big"] == (length >= LEN_LIMIT) and t["starts"] <= TCAP and t["per_chunk"] == 1
    assert f["lengths"] == (LEN_LIMIT - 1, LEN_LIMIT) and f["starts_at"][0] // RB == f["tile"] >= 2
    assert tiles[f["starts_at"][1] // RB]["starts"] == 1
    assert lay["bin"][lay["length"] >= LEN_LIMIT - 1].max() < 1 << bm.order_bits(len(block))      # keyed by their first 31 bases
    assert sum(t["path"] == bm.AGAIN for t in tiles) == 1


@pytest.mark.parametrize("name,bits", [("I_bits13", 13), ("I_bits14", 14)])
def test_i_bin_width_above_the_minimum(name, bits):
    """order_bits of a ragged block of ~4 MB is 13, of ~6 MB 14: the prefix over the 2^bits + 1 bin sizes takes more than two
    workgroups of 4096 entries (ss_reorder.hip SCAN_PER)."""
    block, _ = case(name)
    assert bm.order_bits(len(block)) == bits and ((1 << bits) + 1 + 4095) // 4096 > 2
    assert (3.9e6 < len(block) < 4.3e6) if bits == 13 else (5.8e6 < len(block) < 6.3e6)
    lay = bm.layout(block)
    assert (lay["length"] < 31).sum() > 50 and len(set(lay["length"].tolist())) > 100
    recs = bm.records_of(block, lay)
    assert sum(1 for r in recs if b"N" in r[:31]) > 100 and sum(1 for r in recs if r[:31] != r[:31].upper()) > 100
    assert set(b // 4096 for b in lay["bin"].tolist()) == set(range(((1 << bits) + 1 + 4095) // 4096))      # every workgroup of the prefix


# ---- the checker can fail ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A_start+0_0", "E_32_+", "G_final_31_0"])
def test_parse_slab_rejects_a_damaged_slab(name):
    """A model-built slab with a record dropped, a slot shifted by 8, a byte that is no newline in a slot's padding or behind the
    total: parse_slab raises on each (and takes the slab as it was built)."""
    block, _ = case(name)
    slab, total = bm.build_slab(block)
    recs = bm.parse_slab(slab, total)
    slots = [bm.slot_of(len(r)) for r in recs]
    at = np.concatenate([[0], np.cumsum(slots)]).tolist()
    j = next(i for i, r in enumerate(recs) if slots[i] - len(r) >= 2 and i > 0)     # a slot with padding behind its newline
    dropped = slab[:at[j]] + b"\n" * slots[j] + slab[at[j + 1]:]                     # the record's bytes gone, its slot left empty
    with pytest.raises(bm.SlabError):
        bm.parse_slab(dropped, total)
    shifted = slab[:at[j]] + b"\n" * 8 + slab[at[j]:len(slab) - 8]                   # this slot and all behind it 8 bytes late
    with pytest.raises(bm.SlabError):
        bm.parse_slab(shifted, total)
    pad = bytearray(slab)
    pad[at[j + 1] - 1] = ord("A")                                                    # the last pad byte of the slot
    with pytest.raises(bm.SlabError):
        bm.parse_slab(bytes(pad), total)
    if len(slab) > total:
        behind = bytearray(slab)
        behind[total] = ord("A")
        with pytest.raises(bm.SlabError):
            bm.parse_slab(bytes(behind), total)
    with pytest.raises(bm.SlabError):
        bm.parse_slab(slab, total - 8)                                               # a wrong total: the last slot runs beyond it
