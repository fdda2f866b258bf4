"""Hand-built BAM streams for the mate link and the fragment join (tests/test_bam_pairs_host.py, tests/test_bam_pairs_gpu.py).

stream(n) holds exactly n records, n in SIZES.  From 255 records on every stream carries all of:
  placement   a pair whose mates are the first and the last record of the stream, mate 2 standing first; the rest shuffled
  flags       0x10 on mate 1, on mate 2, on both; both and neither of 0x40 / 0x80 on a name of its own (an orphan of role 0); 0x1
              clear on records with repeated names, 0x40 set on one of them, one of them bearing a pair's name (singles all)
  not kept    secondary, supplementary and l_seq == 0 records under a pair's name; a pair whose only third record is a secondary
              one; orphans whose mate is not kept (no bases; secondary)
  names       r1 and r10, a name of 1 byte, two names of 254 bytes that differ in the last byte
  lengths     mates of 1, 15, 16, 17 and 150 bases in every combination (fragment starts at every residue modulo 16 come with the
              number of records); 4097 records: a pair of 20 000-base mates (the join's piece loop wraps: 16 lanes x 16 bytes)
  qualities   a pair without qualities (0xFF), the rest seeded in 2..40
"""
import numpy as np

from tests import bamio

HDR = bamio.header()
SIZES = (0, 1, 2, 255, 256, 257, 4097)
LENGTHS = (1, 15, 16, 17, 150)
R = bamio.record


def _seq(rs, n):
    return "".join("ACGT"[i] for i in rs.randint(0, 4, size=n))


def _rec(rs, name, n, flag, qual=None):
    seq = _seq(rs, n)
    q = rs.randint(2, 41, size=n).astype(np.uint8).tobytes() if qual is None else qual
    return R(name, seq, flag=flag, qual=q, aux=rs.bytes(int(rs.randint(0, 9))))


def _pair(rs, name, n1, n2, f1=0, f2=0, qual=None):
    return [_rec(rs, name, n1, 0x41 | f1, qual and qual * n1), _rec(rs, name, n2, 0x81 | f2, qual and qual * n2)]


def _fixed(rs):
    """the units every stream of 255 records and more carries"""
    u = []
    u += _pair(rs, "r1", 150, 150) + _pair(rs, "r10", 17, 16) + _pair(rs, "x", 1, 1)
    u += _pair(rs, "n" * 254, 15, 150) + _pair(rs, "n" * 253 + "m", 150, 15)
    u += _pair(rs, "rev1", 150, 17, f1=0x10) + _pair(rs, "rev2", 16, 150, f2=0x10) + _pair(rs, "rev12", 15, 16, f1=0x10, f2=0x10)
    u += _pair(rs, "d", 150, 150) + [_rec(rs, "d", 100, 0x100 | 0x41), _rec(rs, "d", 90, 0x800 | 0x81 | 0x10), _rec(rs, "d", 0, 0x41)]
    u += _pair(rs, "e", 16, 16) + [_rec(rs, "e", 80, 0x100 | 0x81)]
    u += [_rec(rs, "o", 150, 0x41), _rec(rs, "o", 0, 0x81), _rec(rs, "o2", 17, 0x81), _rec(rs, "o2", 50, 0x41 | 0x100)]
    u += [_rec(rs, "neither", 150, 0x1), _rec(rs, "both", 15, 0x1 | 0x40 | 0x80), _rec(rs, "lone1", 16, 0x41 | 0x10), _rec(rs, "lone2", 1, 0x81)]
    u += [_rec(rs, "s", 150, 4), _rec(rs, "s", 17, 0), _rec(rs, "s", 16, 0x10), _rec(rs, "s", 15, 0x40), _rec(rs, "r1", 150, 4)]
    u += _pair(rs, "noqual", 150, 16, qual=b"\xff")
    for a in LENGTHS:                                    # 10 more pairs: every combination of two lengths, one way round
        for b in LENGTHS:
            if a < b:
                u += _pair(rs, "len%d_%d" % (a, b), a, b)
    return u


def records(n, seed=0):
    rs = np.random.RandomState(1000 + n + seed)
    if n == 0:
        return []
    if n == 1:
        return [_rec(rs, "solo", 150, 0x41)]
    if n == 2:
        return [_rec(rs, "p", 17, 0x81 | 0x10), _rec(rs, "p", 150, 0x41)]        # mate 2 first; first and last record of the stream
    body = _fixed(rs)
    if n >= 4097:
        body += _pair(rs, "long", 20000, 20000, f2=0x10)
    ends = _pair(rs, "ends", 150, 16)
    i = 0
    while len(body) + 2 + 2 <= n:
        a, b = LENGTHS[i % 5], LENGTHS[(i // 5) % 5]
        body += _pair(rs, "f%d" % i, a, b, f1=0x10 * (i % 3 == 0), f2=0x10 * (i % 4 == 0))
        i += 1
    while len(body) + 2 < n:
        body.append(_rec(rs, "pad%d" % len(body), 33, 4))
    body = [body[j] for j in rs.permutation(len(body))]
    out = [ends[1]] + body + [ends[0]]
    assert len(out) == n
    return out


def stream(n, seed=0):
    return HDR + b"".join(records(n, seed))


def violating():
    """{shape: stream}: every one holds ordinary pairs as well, and the 257-record stream bears one name on every record"""
    rs = np.random.RandomState(77)
    ok = _pair(rs, "a", 150, 150) + _pair(rs, "b", 16, 17) + [_rec(rs, "c", 150, 4)]
    s = {}
    s["three_of_one_name"] = ok + _pair(rs, "t", 150, 150) + [_rec(rs, "t", 150, 0x41)]
    s["two_of_role_1"] = ok + [_rec(rs, "u", 150, 0x41), _rec(rs, "u", 150, 0x41 | 0x10)]
    s["role_0_shares_a_name"] = ok[:2] + [_rec(rs, "v", 150, 0x1)] + ok[2:] + [_rec(rs, "v", 150, 0x81)]
    s["one_name_257"] = [_rec(rs, "same", 15 + i % 3, 0x41 if i % 2 else 0x81) for i in range(257)]
    return {k: HDR + b"".join(v) for k, v in s.items()}
