"""The DEFLATE streams of test_deflate_streams_host.py and test_ginflate_streams_gpu.py: every named shape and the fuzz seeds,
written bit by bit with tests/deflate_writer.py (and, for `zlib_*`, by zlib in the modes the rest of the suite never asks for).
Everything is seeded and fixed here; nothing is drawn at run time.  A stream is built once per process (lru_cache).

The budget.  The device inflater reserves SYM_RATIO = 12 symbols per byte of deflate data plus 4096 per chunk and may decline
beyond that; the streams promise that any 4096 bytes of deflate data produce at most 8 x 4096 bytes of text.  `Governor` keeps
that by construction: the tokens that begin in one aligned 256-byte piece of the deflate data produce at most SOFT_CAP bytes
before it pays with ballast (literals of 6 bits or more: at most 341 more bytes in the piece), or -- where the block has no
such literal -- ends the block and fills the piece with a stored block (256 more at most).  A stretch of 4096 bytes touches
17 pieces: 17 x (SOFT_CAP + 341) <= 32768; a stretch of B bytes touches B / 256 + 2: less than 8 B + 4096."""
import base64
import functools
import random
import zlib

import numpy as np

from . import deflate_writer as dw

RING_REACH, FAR_MAX, WIN_MAX = 1784, 12, 264      # ss_ginflate_dev.h (restated where the GPU test lists its constants)
GZIP_HEADER_BITS = 80                              # the member's 10-byte header: the device stages the FILE's dwords
PIECE_BITS, SOFT_CAP = 256 * 8, 1550


class Stream:
    def __init__(self, name, member, text, writer=None, notes=None):
        self.name, self.member, self.text, self.writer, self.notes = name, member, text, writer, notes or {}
        self.raw = member[10:-8]
        self.n_blocks = len(writer.blocks) if writer else None


class Governor:
    def __init__(self, w, rng):
        self.w, self.rng = w, rng
        self.piece, self.base = -1, 0
        self.ballast, self.reopen = [], None

    def block(self, ballast, reopen=None):
        """The literals the open block may pay with (code lengths of 6 bits or more), or how to open the same block again."""
        self.ballast, self.reopen = list(ballast), reopen
        assert self.ballast or reopen

    def fits(self, n):
        p = self.w.bitpos // PIECE_BITS
        if p != self.piece:
            self.piece, self.base = p, len(self.w.text)
        return len(self.w.text) - self.base + n <= SOFT_CAP

    def pay(self, n):
        """Ballast until `n` more bytes fit."""
        while not self.fits(n):
            if self.ballast:
                self.w.token(("L", self.rng.choice(self.ballast)))
            else:
                self.w.end_block()
                room = -(-(self.w.bitpos + 40) // PIECE_BITS) * PIECE_BITS - self.w.bitpos
                self.w.stored(self.rng.randbytes(max(1, room // 8 - 4)))
                self.reopen()

    def token(self, t):
        self.pay(dw.token_length(t))
        self.w.token(t)


def long_literals(lit_lens, least=6):
    return [s for s in range(256) if lit_lens[s] >= least]


def bushy_chain(units, n_total):
    """chain_code over `units`, each a symbol or a list of 2^m symbols that share the unit's leaf as a flat subtree."""
    assert len(units) <= 16
    lens = [0] * n_total
    for i, u in enumerate(units):
        d = min(i + 1, len(units) - 1)
        syms = u if isinstance(u, (list, tuple)) else [u]
        syms = syms[:1 << min(15 - d, (len(syms) - 1).bit_length())]      # (a bush that would grow beyond 15 bits is cut back)
        m = (len(syms) - 1).bit_length()
        assert len(syms) == 1 << m and d + m <= 15
        for s in syms:
            lens[s] = d + m
    assert dw.kraft(lens) == 32768
    return lens


def random_prelude(w, rng, n=33000):
    """Random bytes over all 256 values as stored blocks: text for the distances up to 32768 to reach into."""
    w.stored(rng.randbytes(n))


def random_match(rng, lit_lens, dist_lens, have, len_syms=None, dist_syms=None):
    """A random match among the coded length and distance symbols whose distance lies within the `have` bytes of text (None: none)."""
    len_syms = len_syms or [s for s in range(257, len(lit_lens)) if lit_lens[s]]
    dist_syms = [d for d in (dist_syms or [d for d in range(len(dist_lens)) if dist_lens[d]]) if dw.DIST_BASE[d] <= min(have, 32768)]
    if not len_syms or not dist_syms:
        return None
    ls, ds = rng.choice(len_syms), rng.choice(dist_syms)
    top = min(have, 32768) - dw.DIST_BASE[ds]
    return ("M", ls, rng.randrange(1 << dw.LEN_EXTRA[ls - 257]), ds, rng.randint(0, min(top, (1 << dw.DIST_EXTRA[ds]) - 1)))


ORDINARY_LITS = [0x00, 0x7F, 0x80, 0xFF] + list(range(0x30, 0x6C))      # 64 byte values


def ordinary_codes(n_lit=286, n_dist=30):
    """An everyday block: 64 literals, end of block and eleven length symbols in a flat code (6-7 bits), eight distance symbols."""
    lit = dw.flat_code([s for s in ORDINARY_LITS + [256, 257, 258, 259, 260, 262, 265, 268, 270, 273, 277, 285] if s < n_lit], n_lit)
    dist = dw.flat_code([0, 2, 5, 9, 12, 16, 19, 23], n_dist)
    return lit, dist


def ordinary_block(w, gov, rng, n_tokens, final=False, codes=None, cl_plan=None):
    lit, dist = codes or ordinary_codes()
    w.begin_dynamic(lit, dist, final, cl_plan)
    gov.block(long_literals(lit))
    lits = [s for s in range(256) if lit[s]]
    for _ in range(n_tokens):
        t = random_match(rng, lit, dist, len(w.text)) if rng.random() < 0.3 else None
        gov.token(t or ("L", rng.choice(lits)))
    w.end_block()


def finish(name, w, notes=None):
    return Stream(name, w.gzip(), bytes(w.text), w, notes)


# ---- inside one chunk ----------------------------------------------------------------------------------------------------------

LONG_LIT_UNITS = [0x00, [1, 2, 3, 4, 5, 6, 7, 8], 0x7F, 285, 0x80, [257, 258, 259, 260], 0xFF, 284, 256, [0x20, 0x21], 264, 0x41, 277, 0x0A, 281, 0xC3]
LONG_DIST_UNITS = [0, 1, 29, 28, [2, 3], 4, 10, 16, 17, 20, 22, 24, 26, 27, 5, [6, 7, 8, 9]]


def build_long_codes():
    """Sixteen blocks; the literal/length units and the distance units are rotated through the chain's depths 1 .. 15, so every
    literal, length symbol and distance symbol named there is written with every code length: 15-bit codes of all three kinds,
    literal codes of exactly 9 and 10 bits (both sides of the 9-bit direct table) and distance codes of exactly 8 and 9."""
    rng = random.Random(101)
    w = dw.DeflateWriter()
    gov = Governor(w, rng)
    seen = dict(lit=set(), length=set(), dist=set())
    for k in range(16):
        lu = LONG_LIT_UNITS[k:] + LONG_LIT_UNITS[:k]
        du = LONG_DIST_UNITS[(5 * k) % 16:] + LONG_DIST_UNITS[:(5 * k) % 16]
        lit, dist = bushy_chain(lu, 286), bushy_chain(du, 30)
        w.begin_dynamic(lit, dist, final=k == 15)
        gov.block(long_literals(lit))
        for _ in range(2200):
            u = rng.choice(lu)
            s = rng.choice([x for x in u if lit[x]]) if isinstance(u, list) else u
            if s == 256:
                continue
            if s < 256:
                t = ("L", s)
            else:
                du_pick = rng.choice(du)
                t = random_match(rng, lit, dist, len(w.text), [s], [x for x in du_pick if dist[x]] if isinstance(du_pick, list) else [du_pick])
                if t is None:
                    continue
                seen["length"].add(lit[s])
                seen["dist"].add(dist[t[3]])
            if s < 256:
                seen["lit"].add(lit[s])
            gov.token(t)
        w.end_block()
    return finish("long_codes", w, dict(seen=seen))


def build_widest_item():
    """The 48-bit item (a 15-bit length code + 5 extra bits, a 15-bit distance code + 13 extra bits), its first bit of the FILE at
    each of the 32 offsets within a dword, and across the 512-byte boundaries of the file (every second one is a 1024-byte one)."""
    rng = random.Random(102)
    w = dw.DeflateWriter()
    gov = Governor(w, rng)
    random_prelude(w, rng)
    eight = list(range(0x40, 0x50))
    lit = bushy_chain([0x00, 0xFF, 0x80, eight, 0x7F, 0x01, 0x02, 256, 257, 265, 270, 275, 279, 281, 284, 283], 286)
    dist = bushy_chain([0, 1, 5, 9, 12, 15, 18, 20, 22, 24, 25, 26, 23, 27, 29, 28], 30)
    assert lit[284] == lit[283] == 15 and dist[29] == dist[28] == 15 and lit[0x00] == 1
    starts, target = [], 0
    while w.bitpos < (33 + 80) * 1024 * 8:
        w.begin_dynamic(lit, dist)
        gov.block(eight)
        for _ in range(24):
            pos = GZIP_HEADER_BITS + w.bitpos
            lo = pos + 2100 + 31
            edge = -(-lo // 4096) * 4096                 # the next 512-byte boundary of the file
            if len(starts) % 2 and edge - 47 < lo + 2300 and edge - 47 >= lo:
                start = edge - rng.randint(1, 47)        # the item lies across it
            else:
                start = lo + (target % 32 - lo) % 32
            while GZIP_HEADER_BITS + w.bitpos + 8 + 31 <= start:
                w.token(("L", rng.choice(eight)))
            gov.pay(258 + 40)                            # (never needed: the ballast above has left the piece behind)
            while GZIP_HEADER_BITS + w.bitpos + 8 <= start:
                w.token(("L", rng.choice(eight)))
            while GZIP_HEADER_BITS + w.bitpos < start:
                w.token(("L", 0x00))
            if GZIP_HEADER_BITS + w.bitpos != start:
                continue
            ds = rng.choice((28, 29))
            t = ("M", rng.choice((283, 284)), rng.randrange(32), ds, rng.randrange(8192))
            assert w.token_bits(t) == 48
            starts.append(GZIP_HEADER_BITS + w.bitpos)
            target += start % 32 == target % 32
            w.token(t)
        w.end_block()
    ordinary_block(w, gov, rng, 50, final=True)
    return finish("widest_item", w, dict(starts=starts))


def build_every_length_and_distance():
    rng = random.Random(103)
    w = dw.DeflateWriter()
    gov = Governor(w, rng)
    random_prelude(w, rng)
    lit, dist = dw.flat_code(range(286), 286), dw.flat_code(range(30), 30)
    jobs = [dw.match(n, d) for n in range(3, 259) for d in (rng.randint(1, 32768),)]
    jobs += [dw.match(258, rng.randint(1, 32768), long_258=True) for _ in range(8)]
    for ds in range(30):
        for ls in (257, 265, 285):
            jobs += [("M", ls, 0, ds, 0), ("M", ls, 0, ds, (1 << dw.DIST_EXTRA[ds]) - 1)]
    edge = [2047, 2048, 2049, 32767, 32768]
    for n in (FAR_MAX, FAR_MAX + 1):
        edge += [RING_REACH - 1, RING_REACH, RING_REACH + 1, RING_REACH + n - 1, RING_REACH + n]
    jobs += [dw.match(n, d) for d in edge for n in (3, FAR_MAX, FAR_MAX + 1, 64, 258)]
    jobs = jobs * 3
    rng.shuffle(jobs)
    for a in range(0, len(jobs), 150):
        w.begin_dynamic(lit, dist)
        gov.block(long_literals(lit))
        for t in jobs[a:a + 150]:
            for _ in range(rng.randint(0, 6)):
                gov.token(("L", rng.randrange(256)))
            gov.token(t)
        w.end_block()
    ordinary_block(w, gov, rng, 50, final=True)
    return finish("every_length_and_distance", w, dict(jobs=set(jobs)))


def build_overlap():
    """Matches that overlap themselves (distance < length), at every ring position the ballast leaves them."""
    rng = random.Random(104)
    w = dw.DeflateWriter()
    gov = Governor(w, rng)
    lit, dist = dw.flat_code(range(286), 286), dw.flat_code(range(30), 30)
    pairs = [(d, n) for d in (1, 2, 3, 63, 64, 65, 257) for n in (3, 64, 65, 258) if d < n]
    w.begin_dynamic(lit, dist)
    gov.block(long_literals(lit))
    for _ in range(300):
        gov.token(("L", rng.randrange(256)))
    w.end_block()
    while w.bitpos < 36 * 1024 * 8:
        w.begin_dynamic(lit, dist)
        gov.block(long_literals(lit))
        rng.shuffle(pairs)
        for d, n in pairs:
            for _ in range(rng.randint(1, 5)):
                gov.token(("L", rng.randrange(256)))
            gov.token(dw.match(n, d, long_258=rng.random() < 0.5))
        w.end_block()
    ordinary_block(w, gov, rng, 50, final=True)
    return finish("overlap", w, dict(pairs=pairs))


def build_window_totals():
    """Two-bit literals and six-bit matches of 258: up to thirty items in one 64-bit window, delivering 258 + 0 .. 29 symbols -- both
    sides of WIN_MAX --; pairs of matches of 115 .. 130; and blocks of 12-bit matches of 11 and 12 from beyond the ring's reach, six
    of which begin in one window: more than 64 far symbols."""
    rng = random.Random(105)
    w = dw.DeflateWriter()
    gov = Governor(w, rng)
    random_prelude(w, rng, 4000)
    eight = list(range(0x60, 0x6E))
    lit = [0] * 286
    for s in (0x00, 0x80, 0xFF):
        lit[s] = 2
    for s in (285, 280, 257):
        lit[s] = 4
    for s in eight + [256, 264]:
        lit[s] = 8
    dist = [0] * 30
    dist[0] = dist[1] = dist[16] = 2
    dist[22] = dist[29] = 3
    far_lit = bushy_chain([265, 0x00, 0xFF, eight + [0x10, 0x11], 0x80, 256], 286)
    far_dist = bushy_chain([21, 0, 22, 29], 30)
    far_runs = 0
    two = (0x00, 0x80, 0xFF)
    for rnd in range(14):
        w.begin_dynamic(lit, dist)
        gov.block(eight)
        for k in range(30):
            gov.pay(258 + 30)
            for _ in range(k):
                w.token(("L", rng.choice(two)))
            w.token(("M", 285, 0, rng.choice((0, 1)), 0))
            for _ in range(29 - k):
                w.token(("L", rng.choice(two)))
        for k in range(16):
            gov.pay(2 * 130 + 30)
            x = rng.randrange(16)
            w.token(("M", 280, x, 16, rng.randrange(128)))
            for _ in range(k):
                w.token(("L", rng.choice(two)))
            w.token(("M", 280, rng.randrange(16), 0, 0))
            for _ in range(22 - k):
                w.token(("L", rng.choice(two)))
        w.end_block()
        w.begin_dynamic(far_lit, far_dist)
        gov.block(eight + [0x10, 0x11])
        for _ in range(40):
            gov.pay(8 * 12 + 4)
            for _ in range(8):
                if len(w.text) > 2048:
                    w.token(("M", 265, rng.randrange(2), 21, rng.randint(RING_REACH + FAR_MAX - 1537, 511)))
                    assert w.token_bits(("M", 265, 0, 21, 0)) == 12
            far_runs += 1
            for _ in range(rng.randint(0, 3)):
                w.token(("L", rng.choice((0x00, 0xFF))))
        w.end_block()
    ordinary_block(w, gov, rng, 50, final=True)
    return finish("window_totals", w, dict(far_runs=far_runs))


def build_header_shapes():
    rng = random.Random(106)
    w = dw.DeflateWriter()
    gov = Governor(w, rng)
    kinds = []

    def special(kind, lit, dist, n_tokens=400, cl_plan=None, matches=True):
        w.begin_dynamic(lit, dist, cl_plan=cl_plan)
        kinds.append((kind, dict(w.header)))
        ballast = long_literals(lit)
        lits = [s for s in range(256) if lit[s]]
        plan = cl_plan
        gov.block(ballast, None if ballast else (lambda: w.begin_dynamic(lit, dist, cl_plan=plan)))
        for _ in range(n_tokens if lits else 0):
            t = random_match(rng, lit, dist, len(w.text)) if matches and rng.random() < 0.3 else None
            gov.token(t or ("L", rng.choice(lits)))
        w.end_block()

    def runs_code():
        coded = list(range(0, 7)) + list(range(10, 14)) + [24] + list(range(36, 100)) + list(range(238, 260))
        lit = dw.flat_code(coded, 286)
        dist = [0] * 5 + dw.flat_code(range(8), 8)
        rest = lit[36:100]
        tail = lit[238:] + dist
        items = [(6, 1), (16, 6), (17, 3), (6, 1), (16, 3), (17, 10), (6, 1), (18, 11)] + dw.plain_cl_items(rest) + [(18, 138)] + dw.plain_cl_items(tail)
        assert lit[0] == 6 and lit[13] == 6 and lit[24] == 6
        return lit, dist, items

    for rnd in range(5):
        ordinary_block(w, gov, rng, 300)
        special("literal_only", dw.flat_code(list(range(127)) + [256], 257), [0], matches=False)
        ordinary_block(w, gov, rng, 300)
        lit = dw.flat_code(list(range(64, 186)) + [256, 257, 260, 264, 266, 285], 286)
        special("one_distance_code", lit, [1])
        special("one_distance_code_far", lit, [0] * 19 + [1])
        ordinary_block(w, gov, rng, 300)
        eob_only = [0] * 257
        eob_only[256] = 1
        special("empty", eob_only, [0], n_tokens=0)
        ordinary_block(w, gov, rng, 300)
        special("hlit_286_hdist_30", dw.flat_code(range(286), 286), dw.flat_code(range(30), 30))
        lit, dist = ordinary_codes(270, 24)
        special("hclen_smallest", lit, dist)
        special("hclen_19", lit, dist, cl_plan=dict(hclen=19))
        lit, dist, items = runs_code()
        special("runs_min_max", lit, dist, cl_plan=dict(items=items))
        # a run of zeros from the literal lengths into the distance lengths, and a run of copies likewise
        special("zero_run_crosses", dw.flat_code(ORDINARY_LITS + [256, 257, 258, 259], 286), [0] * 6 + dw.flat_code(range(8), 8))
        lit = dw.flat_code(list(range(100, 224)) + [256, 283, 284, 285], 286)
        special("copy_run_crosses", lit, [7, 7, 7, 7, 5, 4, 3, 2, 1])
        # 200 equal lengths: 33 x "copy the previous length six times" in a row, across the header parser's windows
        lit = [8] * 200 + [0] * 56 + [7] * 28
        special("copies_in_a_row", lit + [0] * 2, dw.flat_code(range(16), 16))
    ordinary_block(w, gov, rng, 50, final=True)
    return finish("header_shapes", w, dict(kinds=kinds))


def build_stored_blocks():
    """Stored blocks of LEN 0, 1, 1023, 1024, 1025 and 65535 behind dynamic blocks that end at each of the eight bit positions of a
    byte (0 .. 7 padding bits), a match right behind each that reads from it, and a stored block as the final one."""
    rng = random.Random(107)
    w = dw.DeflateWriter()
    gov = Governor(w, rng)
    lit = bushy_chain([0x00, list(range(0x40, 0x60)), 0xFF, [257, 258, 259, 260, 262, 265, 268, 270], 256, 0x80, 0x7F], 286)
    dist = dw.flat_code(range(30), 30)
    assert lit[0x00] == 1
    lits = [s for s in range(256) if lit[s]]
    pads = []
    for n in (0, 1, 1023, 1024, 1025, 65535):
        for align in ((0, 5) if n == 65535 else range(8)):
            w.begin_dynamic(lit, dist)
            gov.block(long_literals(lit))
            if pads:                                          # a match right behind the stored block, reading from it
                have = w.blocks[-1][3]
                for d in sorted({1, max(1, have // 2), min(have, 32768)} if have else ()):
                    gov.token(dw.match(rng.choice((3, 12, 26)), d))
            for _ in range(120):
                t = random_match(rng, lit, dist, len(w.text)) if rng.random() < 0.3 else None
                gov.token(t or ("L", rng.choice(lits)))
            while (w.bitpos + lit[256] + 3) % 8 != (8 - align) % 8:
                w.token(("L", 0x00))
            w.end_block()
            pads.append((n, -(w.bitpos + 3) % 8))
            assert pads[-1][1] == align
            w.stored(rng.randbytes(n))
    ordinary_block(w, gov, rng, 200)
    w.stored(rng.randbytes(1025), final=True)
    return finish("stored_blocks", w, dict(pads=pads))


def build_fixed_between():
    rng = random.Random(108)
    w = dw.DeflateWriter()
    gov = Governor(w, rng)
    random_prelude(w, rng)
    used = dict(length=set(), dist=set())
    while w.bitpos < 40 * 1024 * 8:
        ordinary_block(w, gov, rng, 300)
        w.begin_fixed()
        gov.block(range(256))
        for _ in range(rng.choice((1, 40, 700))):
            if rng.random() < 0.4:
                t = random_match(rng, dw.FIXED_LIT[:286], dw.FIXED_DIST, len(w.text), list(range(280, 286)) + [257, 270])
                used["length"].add(t[1])
                used["dist"].add(t[3])
            else:
                t = ("L", rng.randrange(256))
            gov.token(t)
        w.end_block()
    w.begin_fixed(final=True)
    w.token(("L", 0xFF))
    w.end_block()
    return finish("fixed_between", w, dict(used=used))


# ---- across chunks --------------------------------------------------------------------------------------------------------------

def build_heirloom():
    """32 KB of random bytes, then only short matches 32000 .. 32768 back and a few literals: every 4096-byte chunk's text is
    shorter than the window and nearly all of it is handed down from chunk to chunk, through every window map, across the groups."""
    rng = random.Random(109)
    w = dw.DeflateWriter()
    gov = Governor(w, rng)
    w.stored(rng.randbytes(32768))
    some = [0x00, 0x7F, 0x80, 0xFF] + list(range(0xA0, 0xAC))
    lit = dw.flat_code(some + [256] + list(range(257, 266)), 286)
    dist = [0] * 28 + [1, 1]
    while w.bitpos < (32768 + 82 * 4096) * 8:
        w.begin_dynamic(lit, dist)
        gov.block([], lambda: w.begin_dynamic(lit, dist))
        stop = w.bitpos + rng.randint(2048, 3072) * 8
        while w.bitpos < stop:
            if rng.random() < 0.12:
                gov.token(("L", rng.choice(some)))
            else:
                gov.token(dw.match(rng.randint(3, 11), rng.randint(32000, 32768)))
        w.end_block()
    ordinary_block(w, gov, rng, 50, final=True)
    return finish("heirloom", w)


def build_tiny_blocks():
    """Dynamic blocks of 1 .. 600 symbols (the search's probe is 512 symbols), some empty ones in between."""
    rng = random.Random(110)
    w = dw.DeflateWriter()
    gov = Governor(w, rng)
    random_prelude(w, rng, 3000)
    sizes = list(range(1, 48)) + list(range(500, 525)) + [600, 599, 513, 512, 511] + [rng.randint(1, 600) for _ in range(60)]
    rng.shuffle(sizes)
    eob_only = [0] * 257
    eob_only[256] = 1
    codes = [ordinary_codes(), ordinary_codes(270, 24), (dw.flat_code(list(range(64, 186)) + [256, 257, 260, 264, 266, 285], 286), [1])]
    for i, n in enumerate(sizes):
        ordinary_block(w, gov, rng, n, codes=codes[i % 3])
        if i % 7 == 3:
            w.dynamic(eob_only, [0], [])
        if i % 7 == 5:
            ordinary_block(w, gov, rng, 0)
    ordinary_block(w, gov, rng, 50, final=True)
    return finish("tiny_blocks", w, dict(sizes=sizes))


def random_stream(name, seed, target_bytes, group=False):
    """Random block types and sizes, random complete codes of up to 15 bits, random tokens with distances up to min(32768, the bytes
    so far); the budget kept by the governor.  group: no final block, an empty stored block instead, which ends on a byte."""
    rng = random.Random(seed)
    w = dw.DeflateWriter()
    gov = Governor(w, rng)
    while True:
        final = w.bitpos >= target_bytes * 8
        if final and group:
            w.stored(b"")
            return finish(name, w)
        kind = rng.choice(("dynamic",) * 6 + ("fixed", "stored", "stored"))
        if final and kind == "dynamic":
            ordinary_block(w, gov, rng, rng.randint(0, 40), final=True)
            return finish(name, w)
        if kind == "stored":
            w.stored(rng.randbytes(rng.choice((0, 1, rng.randint(2, 300), rng.randint(300, 5000)))), final)
        else:
            if kind == "fixed":
                lit, dist = dw.FIXED_LIT[:286], dw.FIXED_DIST
                w.begin_fixed(final)
                gov.block(range(256))
            else:
                lits = rng.sample(range(256), rng.choice((1, 2, 3, 8, 30, 100, 200, 256)))
                lens_ = rng.sample(range(257, 286), rng.randint(0, 29))
                lit = dw.random_code(rng, lits + lens_ + [256], 257 + max([s - 256 for s in lens_] + [0]), deep=rng.random())
                dists = rng.sample(range(30), rng.randint(1, 30))
                dist = dw.random_code(rng, dists, max(dists) + 1, deep=rng.random()) if lens_ else [0]
                plan = dict(hclen=19) if rng.random() < 0.2 else None
                w.begin_dynamic(lit, dist, final, plan)
                ballast = long_literals(lit)
                gov.block(ballast, None if ballast else (lambda: w.begin_dynamic(lit, dist, False, plan)))
            lits = [s for s in range(256) if lit[s]]
            p_match = rng.random() * 0.6
            for _ in range(20 if final else rng.choice((0, 1, rng.randint(2, 100), rng.randint(100, 5000)))):
                t = random_match(rng, lit, dist, len(w.text)) if rng.random() < p_match else None
                gov.token(t or ("L", rng.choice(lits)))
            w.end_block()
        if final:
            return finish(name, w)


def long_stream(n_groups=54, group_bytes=72 * 1024):
    """What pigz writes: self-contained pieces (no match reaches in front of its piece), each ending in an empty stored block,
    joined as bytes; here eight random pieces in a fixed shuffled order, then an empty final stored block.  -> Stream"""
    groups = [random_stream("group", 2000 + g, group_bytes, group=True) for g in range(8)]
    order = random.Random(113)
    picks = [groups[order.randrange(8)] for _ in range(n_groups)]
    for g in groups:
        assert g.writer.bitpos % 8 == 0 and zlib.decompress(g.writer.raw() + b"\x01\0\0\xff\xff", -15) == g.text
    raw = b"".join(g.writer.raw() for g in picks) + b"\x01\0\0\xff\xff"
    text = b"".join(g.text for g in picks)
    return Stream("long", dw.gzip_member(raw, text), text)


def build_mixed():
    return random_stream("mixed", 111, 150 * 1024)


# ---- zlib in the modes the rest of the suite never asks for ----------------------------------------------------------------------

def zlib_data(kind):
    rs = np.random.RandomState(112)
    if kind == "text":
        return base64.b64encode(rs.bytes(300000))                                  # 400 KB over 64 characters: ratio 1.33
    return np.cumsum(rs.randint(0, 1000, 100000)).astype("<i4").tobytes()          # the .npz member's kind of data


ZLIB_MODES = dict(sync=dict(flush=zlib.Z_SYNC_FLUSH), full=dict(flush=zlib.Z_FULL_FLUSH), mem1=dict(mem=1), mem9=dict(mem=9), win512=dict(wbits=25))


def build_zlib(mode, kind):
    data, m = zlib_data(kind), ZLIB_MODES[mode]
    co = zlib.compressobj(6, zlib.DEFLATED, m.get("wbits", 31), m.get("mem", 8))
    out = []
    for a in range(0, len(data), 128 << 10):
        out.append(co.compress(data[a:a + (128 << 10)]))
        if "flush" in m:
            out.append(co.flush(m["flush"]))
    out.append(co.flush())
    return Stream("zlib_%s_%s" % (mode, kind), b"".join(out), data)


NAMED = dict(long_codes=build_long_codes, widest_item=build_widest_item, every_length_and_distance=build_every_length_and_distance,
             overlap=build_overlap, window_totals=build_window_totals, header_shapes=build_header_shapes, stored_blocks=build_stored_blocks,
             fixed_between=build_fixed_between, heirloom=build_heirloom, tiny_blocks=build_tiny_blocks, mixed=build_mixed)
for _mode in ZLIB_MODES:
    for _kind in ("text", "int32"):
        NAMED["zlib_%s_%s" % (_mode, _kind)] = functools.partial(build_zlib, _mode, _kind)
FUZZ_SEEDS = list(range(40))
FUZZ = {"fuzz_%02d" % s: functools.partial(random_stream, "fuzz_%02d" % s, 1000 + s, (30 + 170 * s * s // (39 * 39)) * 1024) for s in FUZZ_SEEDS}
ALL = dict(NAMED, **FUZZ)


@functools.lru_cache(maxsize=None)
def stream(name):
    return ALL[name]()


def zlib_trace(raw, step=64):
    """The trace of a stream without a writer: zlib's inflater fed `step` bytes at a time (bits fed, text so far)."""
    do = zlib.decompressobj(-15)
    bits, outs, n = [0], [0], 0
    for a in range(0, len(raw), step):
        n += len(do.decompress(raw[a:a + step]))
        bits.append(8 * min(len(raw), a + step))
        outs.append(n)
    return np.array(bits, np.int64), np.array(outs, np.int64)


def budget_figures(bits, outs):
    """From a writer's trace: the most text that the tokens beginning in any 4096 bytes of deflate data produce, and the largest
    excess of a stretch's text over 12 bytes per byte of its deflate data (the driver adds 4096 per chunk)."""
    j = np.searchsorted(bits, bits + 4096 * 8, "left")
    j = np.minimum(j, len(bits) - 1)
    worst = int((outs[j] - outs).max())
    f = outs - 12 * bits / 8.0
    excess = float((f - np.minimum.accumulate(f)).max())
    return worst, excess
