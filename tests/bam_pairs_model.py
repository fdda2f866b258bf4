"""The model of the BAM mate link and its fragments (ss_bam_mates, ss_reads_join_pairs_bam, ss_bam_select_pairs), restating the rule
of include/strainscan_hip.h, "Read pairs from a BAM", on top of tests/bamio.decode.

KEPT is the loader's rule: neither 0x100 nor 0x800, l_seq != 0.  flat(r) is the loader's form of kept record r: what bamio.decode
gives (reverse-complemented for 0x10, letters), with the base-quality mask applied in the stored order.  The NAME is the bytes of
read_name before the first NUL -- compared as bytes here: the device compares a 128-bit digest.

A kept record with 0x1 clear is a SINGLE.  A kept record with 0x1 set has ROLE 1 (0x40 and not 0x80), ROLE 2 (0x80 and not 0x40) or
ROLE 0, and the 0x1 records of one name form a group: one record = an ORPHAN, two records of roles {1, 2} = a PAIR, anything else
= a VIOLATION (nothing is built).  Fragments, in the stream order of each one's earlier record:
    pair                     flat(m1) N flat(m2)
    orphan of role 2         N flat
    orphan of role 0 or 1    flat N
    single                   flat N
"""
import struct

import numpy as np

from tests import bamio

NO_MATE, NOT_KEPT = 0xFFFFFFFE, 0xFFFFFFFF
COUNTERS = ("records", "kept", "pairs", "orphans", "singles", "violating")


def header_end(stream):
    l_text = struct.unpack_from("<i", stream, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", stream, p)[0]
    return p


def walk(stream):
    """[dict(at, size, flag, lseq, name, qual)] of the records behind the header of an inflated stream"""
    p, out = header_end(stream), []
    while p < len(stream):
        bs = struct.unpack_from("<i", stream, p)[0]
        lrn = stream[p + 12]
        ncig, flag, lseq = struct.unpack_from("<HHI", stream, p + 16)
        q0 = p + 36 + lrn + 4 * ncig + (lseq + 1) // 2
        out.append(dict(at=p, size=4 + bs, flag=flag, lseq=lseq, name=stream[p + 36:p + 36 + lrn].split(b"\0")[0], qual=stream[q0:q0 + lseq]))
        p += 4 + bs
    assert p == len(stream)
    return out


def kept(rec):
    return not rec["flag"] & 0x900 and rec["lseq"] != 0


def role(rec):
    f = rec["flag"] & 0xC0
    return 1 if f == 0x40 else 2 if f == 0x80 else 0


def flat_forms(stream, recs, min_qual=0):
    """{record index: flat(r)} of the kept records"""
    reads = bamio.decode(stream)
    idx = [i for i, r in enumerate(recs) if kept(r)]
    assert len(reads) == len(idx)
    out = {}
    for i, seq in zip(idx, reads):
        q = recs[i]["qual"]
        if min_qual and q[0] != 0xFF:
            if recs[i]["flag"] & 0x10:
                q = q[::-1]
            seq = "".join("N" if v < min_qual else c for c, v in zip(seq, q))
        out[i] = seq.encode()
    return out


def link(recs):
    """-> (mate: np.uint32[records], counters: [6] in the order of COUNTERS)"""
    mate = np.full(len(recs), NOT_KEPT, np.uint32)
    groups, singles = {}, 0
    for i, r in enumerate(recs):
        if not kept(r):
            continue
        mate[i] = NO_MATE
        if r["flag"] & 0x1:
            groups.setdefault(r["name"], []).append(i)
        else:
            singles += 1
    pairs = orphans = bad = 0
    for g in groups.values():
        if len(g) == 1:
            orphans += 1
        elif len(g) == 2 and sorted(role(recs[i]) for i in g) == [1, 2]:
            mate[g[0]], mate[g[1]] = g[1], g[0]
            pairs += 1
        else:
            bad += len(g)
    n_kept = sum(1 for r in recs if kept(r))
    return mate, [len(recs), n_kept, pairs, orphans, singles, bad]


def fragments(stream, min_qual=0):
    """-> (the fragments in order, or None with a violation; mate; counters; [(leader, its mate or None)])"""
    recs = walk(stream)
    mate, counters = link(recs)
    if counters[5]:
        return None, mate, counters, None
    flat = flat_forms(stream, recs, min_qual)
    out, who = [], []
    for i, r in enumerate(recs):
        if not kept(r):
            continue
        m = int(mate[i])
        if m == NO_MATE:
            out.append(b"N" + flat[i] if r["flag"] & 0x1 and role(r) == 2 else flat[i] + b"N")
            who.append((i, None))
        elif m > i:
            m1, m2 = (i, m) if role(r) == 1 else (m, i)
            out.append(flat[m1] + b"N" + flat[m2])
            who.append((i, m))
    return out, mate, counters, who


def select(stream, hits_of_text, n, min_qual=0):
    """ss_bam_select_pairs: hits_of_text(flat block) -> the hits of each of its records.  -> (the written records' bytes,
    [records, kept, fragments selected, records written])"""
    recs = walk(stream)
    mate, counters = link(recs)
    assert not counters[5]
    flat = flat_forms(stream, recs, min_qual)
    idx = sorted(flat)
    hits = dict(zip(idx, (int(h) for h in hits_of_text(b"".join(flat[i] + b"\n" for i in idx)))))
    out, frags = [], 0
    for i in idx:
        m = int(mate[i])
        if hits[i] + (hits[m] if m != NO_MATE else 0) >= n:
            out.append(stream[recs[i]["at"]:recs[i]["at"] + recs[i]["size"]])
            frags += m == NO_MATE or m > i
    return b"".join(out), [len(recs), len(idx), frags, len(out)]
