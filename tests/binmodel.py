"""A host model of what the GENERAL binning passes of ss_reorder.hip (count_kernel, place_kernel, place_again_kernel) leave
behind: which records a flat block holds, the bin and the slot of each, the slab they are placed into -- and, beside the result,
the geometry the kernels meet on the way (which tile a record starts in, where it ends relative to that tile, which of the two
placing kernels the tile goes to).  Plain Python and numpy; nothing here imports the library or reads what a kernel wrote.

The constants restate ss_reorder.hip; each names the line it restates."""
import numpy as np

CH = 64                       # ss_reorder.hip:70   constexpr int CH = 64            bytes of a slab owned by one lane
RB = 256 * CH                 # ss_reorder.hip:71   constexpr int RB = 256 * CH      ... by one workgroup: the 16 KB tile
HALO = 512                    # ss_reorder.hip:73   constexpr int HALO = 512         bytes behind the tile searched in parallel
MAX_ORDER_BITS = 22           # ss_reorder.hip:74   constexpr int MAX_ORDER_BITS = 22
TCAP = 2 * CH                 # ss_reorder.hip:76   constexpr int TCAP = 2 * CH      record starts a tile's table holds (128)
WALK = 16                     # ss_reorder.hip:251  e += 16                          stride of the walk behind the halo
LEN_LIMIT = 1 << 26           # ss_reorder.hip:164-165  LEN_BITS = 26, LEN_LIMIT     a longer record does not fit a table entry
PRE = 6                       # ss_reorder.hip:373  constexpr int PRE = 6            pieces a lane of place_kernel loads ahead
PRE_PIECES = PRE * 256        # ... per tile: place_kernel's tail loop (ss_reorder.hip:424) copies the pieces beyond them
KEY_BYTES = 32                # ss_reorder.hip:290, 447  (s + 32 <= n) ? record_bin(...) : (1u << bits)
MIN_BINNED = 64               # ss_ingest.hip:892   n >= 64: a smaller block is not binned
K, M = 31, 15                 # the k-mer and the minimizer of record_bin (ss_reorder.hip:118-147)

CHUNK, TILE, HALO_END, WALKED = "chunk", "tile", "halo", "walk"     # where a record ends, seen from the tile it starts in
TABLE, AGAIN = "table", "again"                                     # place_kernel / place_again_kernel


def slot_of(length):
    """ss_reorder.hip:270: record + newline, padded to 8 bytes."""
    return (length + 1 + 7) & ~7


def order_bits(n_bytes):
    """ss_reorder.hip:972-977: about four records per bin, 12 bits at least, 22 at most."""
    bits = 12
    while bits < MAX_ORDER_BITS and (n_bytes // 152) >> (bits + 2):
        bits += 1
    return bits


def bin_of(rec, bits, k=K, m=M):
    """Bin of a record (ss_reorder.hip record_bin): top `bits` bits of mix30 of the minimizer of its first 31 bases (either
    case; ordering key of the index, leftmost on ties); 1 << bits when it has no first k-mer.  The `start + 32` rule is not
    here: it depends on where the record lies in its block (layout)."""
    code = {65: 0, 67: 1, 84: 2, 71: 3}
    if len(rec) < k:
        return 1 << bits
    cs = [code.get(c & 0xDF, -1) for c in rec[:k]]
    if min(cs) < 0:
        return 1 << bits
    km = sum(c << (2 * j) for j, c in enumerate(cs))
    best, bx = None, 0
    for i in range(k - m + 1):
        x = (km >> (2 * i)) & 0x3FFFFFFF
        h = (((x & 0xFFFFFF) * (0x4F1BB << 5) + 0x7F4A7C00) & 0xFFFFFFFF) & ~31
        if best is None or h < best:
            best, bx = h, x
    M30 = 0x3FFFFFFF
    h = (bx * 0x9E3779B1) & M30
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & M30
    h ^= h >> 14
    return h >> (30 - bits)


_CODE = np.full(256, 255, np.uint8)
for _c, _v in ((65, 0), (67, 1), (84, 2), (71, 3)):
    _CODE[_c] = _v
    _CODE[_c | 0x20] = _v


def bins_of_heads(heads, bits, k=K, m=M):
    """bin_of for every row of heads (n x 31 bytes, the first k-mers of n records), in numpy (test_binning_general_host.py holds
    it to bin_of)."""
    n = heads.shape[0]
    codes = _CODE[heads[:, :k]]
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


def one_length_candidate(block):
    """(L, n_rec) when order_flat_dev takes the block for the one-length paths (ss_reorder.hip probe_one_length), else None:
    the first newline says L, within FIX_MIN_L..FIX_MAX_L, at least 64 bytes, fewer than 64 bytes behind the last whole record."""
    n, length = len(block), block[:1025].find(b"\n")
    if n < 64 or not 32 <= length <= 1023 or n % (length + 1) >= 64:
        return None
    return length, n // (length + 1)


LAYOUT = np.dtype([("start", np.int64), ("length", np.int64), ("bin", np.int64), ("slot", np.int64)])


def layout(block):
    """(start, length, bin, slot) of every record of a flat block, in file order (a numpy record array).  A record is a maximal
    run of bytes other than newline; slot = (length + 1 + 7) & ~7; the bin is that of order_bits(len(block)) -- and 1 << bits,
    whatever its bases are, for a record with start + 32 > len(block): the kernels call record_bin only where 32 bytes are
    readable (ss_reorder.hip:290 in count_kernel, :447 in place_again_kernel)."""
    a = np.frombuffer(block, np.uint8)
    n = a.size
    bits = order_bits(n)
    nl = a == 10
    before = np.empty(n, bool)
    if n:
        before[0] = True
        before[1:] = nl[:-1]
    starts = np.flatnonzero(~nl & before)
    nls = np.flatnonzero(nl)
    at = np.searchsorted(nls, starts)
    ends = np.where(at < nls.size, nls[np.minimum(at, nls.size - 1)], n) if nls.size else np.full(starts.size, n)
    out = np.zeros(starts.size, LAYOUT)
    out["start"], out["length"] = starts, ends - starts
    out["slot"] = (out["length"] + 1 + 7) & ~7
    out["bin"] = bins_at(a, starts, out["length"], bits)
    out["bin"][starts + KEY_BYTES > n] = 1 << bits
    return out


def bins_at(a, starts, lengths, bits):
    """record_bin of the records of the byte array `a` that start at `starts` with `lengths`, by their bases alone."""
    out = np.full(len(starts), 1 << bits, np.int64)
    keyed = np.flatnonzero(np.asarray(lengths) >= K)
    if keyed.size:
        out[keyed] = bins_of_heads(a[np.asarray(starts)[keyed][:, None] + np.arange(K)[None, :]], bits)
    return out


def records_of(block, lay=None):
    """The records of a block as bytes, in file order."""
    lay = layout(block) if lay is None else lay
    return [block[s:s + n] for s, n in zip(lay["start"].tolist(), lay["length"].tolist())]


def slab_length(total):
    """ss_reorder.hip:1067 slab_positions: the total rounded up to 16, and at least 16."""
    return max((total + 15) & ~15, 16)


def expected_slab(block):
    """What the general passes make of a block: {"n_records", "bits", "per_bin": {bin: sorted records}, "total": the sum of the
    slots, "slab_len": the total rounded up to 16 and at least 16, "by_rule": the records that are in the last bin by the
    start + 32 rule alone (their bases have a bin)}."""
    lay = layout(block)
    bits = order_bits(len(block))
    recs = records_of(block, lay)
    per_bin = {}
    for b, r in zip(lay["bin"].tolist(), recs):
        per_bin.setdefault(b, []).append(r)
    for b in per_bin:
        per_bin[b].sort()
    total = int(lay["slot"].sum())
    late = np.flatnonzero(lay["start"] + KEY_BYTES > len(block)).tolist()
    by_rule = [recs[i] for i in late if bin_of(recs[i], bits) != 1 << bits]
    return dict(n_records=len(lay), bits=bits, per_bin=per_bin, total=total, slab_len=slab_length(total), by_rule=by_rule)


def build_slab(block):
    """A slab as the model would place it: the records in bin order (file order inside a bin), each in its slot, newlines up
    to slab_len.  -> (slab, total)"""
    lay = layout(block)
    recs = records_of(block, lay)
    order = np.argsort(lay["bin"], kind="stable").tolist()
    parts = [recs[i] + b"\n" * (int(lay["slot"][i]) - len(recs[i])) for i in order]
    total = int(lay["slot"].sum())
    return b"".join(parts) + b"\n" * (slab_length(total) - total), total


class SlabError(AssertionError):
    pass


def parse_slab(slab, total):
    """Walks a read-back ASCII slab slot by slot: at a slot start, the record runs to the first newline; the next slot starts
    slot_of(its length) further on; until `total`.  Raises SlabError when a slot starts with a newline before `total` (a gap, a
    lost record), when a byte of a slot behind its record is not a newline, when a slot runs beyond `total`, or when anything but
    newlines follows `total`.  -> the records in slab order."""
    if total > len(slab):
        raise SlabError("total %d beyond the slab's %d bytes" % (total, len(slab)))
    recs, p = [], 0
    while p < total:
        if slab[p] == 10:
            raise SlabError("slot at %d starts with a newline (total %d): a gap or a lost record" % (p, total))
        e = slab.find(b"\n", p)
        if e < 0 or e >= total:
            raise SlabError("record at %d has no newline before the total %d" % (p, total))
        nxt = p + slot_of(e - p)
        if nxt > total:
            raise SlabError("slot at %d (record of %d bytes) ends at %d, beyond the total %d" % (p, e - p, nxt, total))
        if slab.count(b"\n", e, nxt) != nxt - e:
            raise SlabError("padding of the slot at %d (record of %d bytes) holds a byte that is no newline" % (p, e - p))
        recs.append(slab[p:e])
        p = nxt
    if slab.count(b"\n", total) != len(slab) - total:
        raise SlabError("a byte behind the total %d is no newline" % total)
    return recs


def tile_facts(block):
    """What the kernels meet in each 16 KB tile and for each record.
    -> (tiles, ends): tiles = a list, one dict per tile: "starts" (record starts in it), "per_chunk" (the most starts in one
    64-byte chunk), "big" (a record of 2^26 bytes or more starts in it), "pieces" (16-byte pieces of its records' slots: more
    than PRE_PIECES and place_kernel's tail loop runs), "path": TABLE when starts <= 128, at most one start per chunk and no such
    record (ss_reorder.hip:295: fits = !more && cnt <= TCAP && !big), else AGAIN; ends = for every record of layout(block), where
    its end (its newline, or the buffer's end) lies seen from the tile it starts in: CHUNK (in the lane's 64 bytes), TILE, HALO_END
    (the 512 bytes behind the tile) or WALKED (behind them: the loop of ss_reorder.hip:246-254)."""
    lay = layout(block)
    n = len(block)
    n_tiles = (n + RB - 1) // RB
    start, length = lay["start"], lay["length"]
    tile = start // RB
    starts = np.bincount(tile, minlength=n_tiles)
    chunk_counts = np.bincount(start // CH, minlength=n_tiles * (RB // CH)).reshape(n_tiles, RB // CH)
    big = np.bincount(tile, weights=(length >= LEN_LIMIT), minlength=n_tiles) > 0
    pieces = np.bincount(tile, weights=(lay["slot"] + 15) >> 4, minlength=n_tiles).astype(np.int64)
    tiles = []
    for t in range(n_tiles):
        per_chunk = int(chunk_counts[t].max())
        fits = starts[t] <= TCAP and per_chunk <= 1 and not big[t]
        tiles.append(dict(starts=int(starts[t]), per_chunk=per_chunk, big=bool(big[t]), pieces=int(pieces[t]),
                          path=TABLE if fits else AGAIN))
    end = start + length
    tile0 = tile * RB
    ends = np.where(end < (start // CH + 1) * CH, CHUNK,
                    np.where(end < tile0 + RB, TILE, np.where(end < tile0 + RB + HALO, HALO_END, WALKED)))
    return tiles, ends.tolist()
