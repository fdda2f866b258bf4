"""A DEFLATE writer for tests (RFC 1951; gzip framing of RFC 1952).  No compressor: it writes exactly the blocks, codes and
tokens it is told to write, so a test chooses every bit of its input.  Pure Python, no GPU.

Tokens are ('L', byte) or ('M', length_symbol, length_extra, distance_symbol, distance_extra).  The writer replays what it
writes (`text`), records for every block (kind, first bit, last bit, bytes produced) in `blocks`, and for every token its
first bit and the text length in front of it (`trace()`), so that a test can make assertions about its own input."""
import zlib

import numpy as np

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0) + tuple(i // 2 for i in range(2, 28))
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30          # (the fixed distance code has 32 five-bit codes; 30 and 31 never occur)


def length_token_part(length, long_258=False):
    """(length symbol, extra) of a match length 3..258; long_258: 258 spelled as symbol 284 with extra 31."""
    if length == 258:
        return (284, 31) if long_258 else (285, 0)
    s = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + s, length - LEN_BASE[s]


def distance_token_part(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, dist - DIST_BASE[s]


def match(length, dist, long_258=False):
    return ("M",) + length_token_part(length, long_258) + distance_token_part(dist)


def token_length(t):
    return 1 if t[0] == "L" else LEN_BASE[t[1] - 257] + t[2]


def token_distance(t):
    return DIST_BASE[t[3]] + t[4]


def replay(text, tokens):
    """The plain LZ77 replay of `tokens` behind the bytearray `text` (in place)."""
    for t in tokens:
        if t[0] == "L":
            text.append(t[1])
        else:
            n, d = LEN_BASE[t[1] - 257] + t[2], DIST_BASE[t[3]] + t[4]
            assert 0 < d <= len(text), "a match that reaches in front of the text"
            if d >= n:
                text += text[len(text) - d:len(text) - d + n]
            else:
                text += (bytes(text[-d:]) * (n // d + 1))[:n]
    return text


def expected(tokens, prefix=b""):
    return bytes(replay(bytearray(prefix), tokens))


def canonical_codes(lens):
    """Code length per symbol -> the canonical code values, bit-reversed (the writer is LSB first, Huffman codes go MSB first)."""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, n in enumerate(lens):
        if n:
            out[s] = int(format(nxt[n], "0%db" % n)[::-1], 2)
            nxt[n] += 1
    return out


def kraft(lens):
    """Sum of 2^(15 - length) over the coded symbols: 32768 for a complete code."""
    return sum(1 << (15 - n) for n in lens if n)


def random_code(rng, symbols, n_total, max_bits=15, deep=0.5):
    """A random COMPLETE code for `symbols` (lengths for n_total symbols, 0 for the others): a tree is grown by splitting leaves
    -- with probability `deep` the deepest one that may still be split, else a random one -- until there is a leaf per symbol.
    One symbol alone gets one bit (the only incomplete code DEFLATE allows)."""
    symbols = list(symbols)
    lens = [0] * n_total
    if len(symbols) == 1:
        lens[symbols[0]] = 1
        return lens
    leaves = [1, 1]
    while len(leaves) < len(symbols):
        can = [i for i, d in enumerate(leaves) if d < max_bits]
        i = max(can, key=lambda k: leaves[k]) if rng.random() < deep else rng.choice(can)
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(symbols)
    for s, d in zip(symbols, leaves):
        lens[s] = d
    assert kraft(lens) == 32768
    return lens


def chain_code(symbols, n_total):
    """The "chain" code: lengths 1, 2, ..., k - 2, k - 1, k - 1 for the k symbols in the order given (16 symbols: 1 .. 14, 15, 15)."""
    symbols = list(symbols)
    assert 2 <= len(symbols) <= 16
    lens = [0] * n_total
    for i, s in enumerate(symbols):
        lens[s] = min(i + 1, len(symbols) - 1)
    assert kraft(lens) == 32768
    return lens


def flat_code(symbols, n_total):
    """A complete code whose lengths differ by one bit at most."""
    symbols = list(symbols)
    lens = [0] * n_total
    if len(symbols) == 1:
        lens[symbols[0]] = 1
        return lens
    m = (len(symbols) - 1).bit_length()
    short = (1 << m) - len(symbols)
    for i, s in enumerate(symbols):
        lens[s] = m - 1 if i < short else m
    assert kraft(lens) == 32768
    return lens


def plain_cl_items(seq):
    """Code lengths -> run-length items (v, count): v 0..15 a length (count 1), 16 = copy the previous 3..6 times, 17 = 3..10
    zeros, 18 = 11..138 zeros.  One valid choice among many."""
    items, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                items.append((18, k))
                run -= k
            if run >= 3:
                items.append((17, run))
                run = 0
        else:
            items.append((v, 1))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                items.append((16, k))
                run -= k
        items += [(v, 1)] * run
        i = j
    return items


def cl_items_lengths(items):
    """What a decoder makes of run-length items."""
    out = []
    for v, k in items:
        if v < 16:
            out.append(v)
        elif v == 16:
            assert 3 <= k <= 6 and out
            out += [out[-1]] * k
        else:
            assert (3 <= k <= 10) if v == 17 else (11 <= k <= 138)
            out += [0] * k
    return out


class DeflateWriter:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0                  # bits in acc
        self.text = bytearray()     # the replay of everything written so far
        self.blocks = []            # (kind, first bit, last bit (exclusive), bytes produced)
        self._tb, self._to = [], []
        self._open = None

    # ---- bits, LSB first
    @property
    def bitpos(self):
        return len(self.buf) * 8 + self.n

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits
        if self.n >= 512:
            k = self.n >> 3
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def _flush_bytes(self):
        k = self.n >> 3
        if k:
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def _mark(self):
        self._tb.append(self.bitpos)
        self._to.append(len(self.text))

    # ---- blocks
    def stored(self, data, final=False):
        assert self._open is None and len(data) <= 65535
        first, t0 = self.bitpos, len(self.text)
        self._mark()
        self.put(1 if final else 0, 1)
        self.put(0, 2)
        self.put(0, -self.bitpos % 8)
        self.put(len(data), 16)
        self.put(len(data) ^ 0xFFFF, 16)
        self._flush_bytes()
        assert self.n == 0
        for a in range(0, len(data), 256):
            self._mark()
            self.buf += data[a:a + 256]
            self.text += data[a:a + 256]
        self.blocks.append(("stored", first, self.bitpos, len(self.text) - t0))

    def begin_fixed(self, final=False):
        assert self._open is None
        self._open = ("fixed", self.bitpos, len(self.text))
        self.put(1 if final else 0, 1)
        self.put(1, 2)
        self._set_codes(FIXED_LIT, FIXED_DIST)

    def begin_dynamic(self, lit_lens, dist_lens, final=False, cl_plan=None):
        """cl_plan: dict with any of `items` (run-length items (v, count) that decode to lit_lens + dist_lens), `cl_lens` (the 19
        lengths of the code-length code: complete, at most 7 bits) and `hclen` (4..19, at least what cl_lens needs)."""
        assert self._open is None
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        assert 257 <= len(lit_lens) <= 286 and 1 <= len(dist_lens) <= 30 and lit_lens[256]
        plan = cl_plan or {}
        items = plan.get("items") or plain_cl_items(lit_lens + dist_lens)
        assert cl_items_lengths(items) == lit_lens + dist_lens
        used = sorted({v for v, _ in items})
        cl_lens = plan.get("cl_lens")
        if cl_lens is None:
            cl_lens = flat_code(used if len(used) > 1 else used + [u for u in (0, 1) if u not in used][:1], 19)
        assert kraft(cl_lens) == 32768 and max(cl_lens) <= 7 and all(cl_lens[v] for v in used)
        need = max(i for i in range(19) if cl_lens[CL_ORDER[i]]) + 1
        hclen = plan.get("hclen") or max(4, need)
        assert max(4, need) <= hclen <= 19
        self._open = ("dynamic", self.bitpos, len(self.text))
        self.header = dict(hlit=len(lit_lens), hdist=len(dist_lens), hclen=hclen, items=items, item_bits=[])
        self.put(1 if final else 0, 1)
        self.put(2, 2)
        self.put(len(lit_lens) - 257, 5)
        self.put(len(dist_lens) - 1, 5)
        self.put(hclen - 4, 4)
        for i in range(hclen):
            self.put(cl_lens[CL_ORDER[i]], 3)
        cc = canonical_codes(cl_lens)
        for v, k in items:
            self.header["item_bits"].append(self.bitpos)
            self.put(cc[v], cl_lens[v])
            if v == 16:
                self.put(k - 3, 2)
            elif v == 17:
                self.put(k - 3, 3)
            elif v == 18:
                self.put(k - 11, 7)
        self._set_codes(lit_lens, dist_lens)

    def _set_codes(self, lit_lens, dist_lens):
        self.lit_lens, self.dist_lens = lit_lens, dist_lens
        self._lc, self._dc = canonical_codes(lit_lens), canonical_codes(dist_lens)

    def token_bits(self, t):
        if t[0] == "L":
            return self.lit_lens[t[1]]
        return self.lit_lens[t[1]] + LEN_EXTRA[t[1] - 257] + self.dist_lens[t[3]] + DIST_EXTRA[t[3]]

    def token(self, t):
        self._mark()
        if t[0] == "L":
            assert self.lit_lens[t[1]]
            self.put(self._lc[t[1]], self.lit_lens[t[1]])
        else:
            _, ls, lx, ds, dx = t
            assert self.lit_lens[ls] and self.dist_lens[ds] and lx < (1 << LEN_EXTRA[ls - 257]) and dx < (1 << DIST_EXTRA[ds])
            nb = self.lit_lens[ls]
            v = self._lc[ls] | lx << nb
            nb += LEN_EXTRA[ls - 257]
            v |= self._dc[ds] << nb
            nb += self.dist_lens[ds]
            v |= dx << nb
            self.put(v, nb + DIST_EXTRA[ds])
        replay(self.text, (t,))

    def end_block(self):
        kind, first, t0 = self._open
        self._mark()
        self.put(self._lc[256], self.lit_lens[256])
        self.blocks.append((kind, first, self.bitpos, len(self.text) - t0))
        self._open = None

    def fixed(self, tokens, final=False):
        self.begin_fixed(final)
        for t in tokens:
            self.token(t)
        self.end_block()

    def dynamic(self, lit_lens, dist_lens, tokens, final=False, cl_plan=None):
        self.begin_dynamic(lit_lens, dist_lens, final, cl_plan)
        for t in tokens:
            self.token(t)
        self.end_block()

    # ---- results
    def raw(self):
        """The deflate data (the last byte padded with zero bits)."""
        assert self._open is None
        self._flush_bytes()
        return bytes(self.buf) + (bytes([self.acc & 0xFF]) if self.n else b"")

    def gzip(self):
        """One gzip member: a 10-byte header, the deflate data, CRC-32 and ISIZE."""
        return gzip_member(self.raw(), bytes(self.text))

    def trace(self):
        """(first bit of every token -- stored blocks: of every 256 bytes --, text length in front of it), with the end of the
        stream as the last entry."""
        return (np.array(self._tb + [self.bitpos], np.int64), np.array(self._to + [len(self.text)], np.int64))


def gzip_member(raw, text):
    return b"\x1f\x8b\x08\0\0\0\0\0\0\xff" + raw + (zlib.crc32(text) & 0xFFFFFFFF).to_bytes(4, "little") + (len(text) & 0xFFFFFFFF).to_bytes(4, "little")
