"""A seeded BAM writer and a pure-Python reference decoder, for the BAM input tests.

The writer makes BGZF the way bgzip does: raw-deflate members of at most 0xff00 bytes of stream, each with the "BC" extra
field, CRC-32 and ISIZE, and the 28-byte EOF block.  The decoder follows the contract of ss_bam_decode: the reads of a
default `samtools fastq` (secondary 0x100 and supplementary 0x800 records and records without bases skipped, 0x10 records
reverse-complemented), each kept read's letters and '\\n' make the flat block; blocks of 4096 kept records go round the
ranks of a sharded run."""
import gzip
import struct
import zlib

import numpy as np

CODES = "=ACMGRSVTWYHKDBN"
COMP = str.maketrans(CODES, "=TGKCYSBAWRDMHVN")
BLOCK = 0xff00
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SHARD_LOG2 = 12


def revcomp(seq):
    return seq.translate(COMP)[::-1]


def pack_seq(seq):
    codes = [CODES.index(c) for c in seq]
    if len(codes) % 2:
        codes.append(0)
    return bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))


def record(name, seq, flag=4, ref=-1, pos=-1, cigar=(), qual=None, aux=b"", mapq=255, next_ref=-1, next_pos=-1):
    """One BAM record (block_size included).  seq: the letters as STORED (a 0x10 record stores the reverse complement)."""
    rn = name.encode() + b"\0"
    q = bytes([30] * len(seq)) if qual is None else qual
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(rn), mapq, 4680, len(cigar), flag, len(seq), next_ref, next_pos, 0)
    body += rn + b"".join(struct.pack("<I", c) for c in cigar) + pack_seq(seq) + q + aux
    return struct.pack("<i", len(body)) + body


def header(n_ref=2, text="@HD\tVN:1.6\tSO:unsorted\n"):
    t = text.encode()
    out = b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", n_ref)
    for i in range(n_ref):
        nm = ("chr%d" % (i + 1)).encode() + b"\0"
        out += struct.pack("<i", len(nm)) + nm + struct.pack("<i", 1000000)
    return out


def member(data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = c.compress(data) + c.flush()
    bsize = 18 + len(cdata) + 8
    assert bsize <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize - 1) + cdata +
            struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


def bgzf(header_bytes, records, level=6, cuts="htslib", eof=True, seed=0):
    """The BGZF file of a stream.  cuts='htslib': the header is a member of its own, a record starts a new member when it
    does not fit in the current one (a record longer than a member spans several); cuts='random': members end at arbitrary
    offsets (inside block_size too)."""
    stream = header_bytes + b"".join(records)
    pieces = []
    if cuts == "htslib":
        pieces.append(header_bytes)
        cur = b""
        for r in records:
            if cur and len(cur) + len(r) > BLOCK:
                pieces.append(cur)
                cur = b""
            cur += r
            while len(cur) > BLOCK:
                pieces.append(cur[:BLOCK])
                cur = cur[BLOCK:]
        if cur:
            pieces.append(cur)
    else:
        rs = np.random.RandomState(seed)
        o = 0
        while o < len(stream):
            n = int(rs.randint(1, BLOCK + 1)) if rs.random_sample() < 0.7 else int(rs.randint(1, 64))
            pieces.append(stream[o:o + n])
            o += n
    return b"".join(member(p, level) for p in pieces) + (EOF if eof else b"")


def sample_records(seed, reads, aligned=False, decoys=0.0, extras=False):
    """reads: [(name, letters as sequenced)] -> BAM records.  aligned: half of them are 0x10 records storing the reverse
    complement, with a reference, a position and a CIGAR; decoys: that share of secondary / supplementary records holding
    other sequences is mixed in; extras: records without bases, and aux data on every record."""
    rs = np.random.RandomState(seed)
    out = []
    lut = "ACGT"
    for name, seq in reads:
        aux = b"RGZgrp1\0NMC" + bytes([int(rs.randint(0, 9))]) if extras else b""
        qual = rs.randint(2, 41, size=len(seq)).astype(np.uint8).tobytes()       # (a constant quality deflates to nothing)
        if aligned and rs.random_sample() < 0.5:
            out.append(record(name, revcomp(seq), flag=0x10 | 0x1 | 0x40, ref=int(rs.randint(0, 2)), pos=int(rs.randint(0, 99999)),
                              cigar=((len(seq) << 4) | 0,), qual=qual[::-1], aux=aux, mapq=60))
        elif aligned:
            out.append(record(name, seq, flag=0x1 | 0x80, ref=int(rs.randint(0, 2)), pos=int(rs.randint(0, 99999)),
                              cigar=((len(seq) << 4) | 0,), qual=qual, aux=aux, mapq=60))
        else:
            out.append(record(name, seq, flag=4, qual=qual, aux=aux))
        if decoys and rs.random_sample() < decoys:
            other = "".join(lut[i] for i in rs.randint(0, 4, size=int(rs.randint(30, 200))))
            out.append(record(name, other, flag=0x100 if rs.random_sample() < 0.5 else 0x800 | 0x10, ref=0, pos=5, cigar=((len(other) << 4),)))
        if extras and rs.random_sample() < 0.01:
            out.append(record(name + "_empty", "", flag=4))
    return out


def decode(data):
    """The reference decoder: BGZF/gzip (or an uncompressed stream) -> the kept reads, in file order.  ValueError when the
    stream is damaged."""
    if data[:2] == b"\x1f\x8b":
        try:
            data = gzip.decompress(data)
        except (OSError, EOFError, zlib.error) as e:
            raise ValueError("gzip layer: %s" % e)
    if data[:4] != b"BAM\1":
        raise ValueError("no BAM magic")
    n = len(data)

    def need(q):
        if q > n:
            raise ValueError("header runs past the end")
    need(12)
    l_text = struct.unpack_from("<i", data, 4)[0]
    if l_text < 0:
        raise ValueError("l_text")
    p = 8 + l_text
    need(p + 4)
    n_ref = struct.unpack_from("<i", data, p)[0]
    if n_ref < 0:
        raise ValueError("n_ref")
    p += 4
    for _ in range(n_ref):
        need(p + 4)
        ln = struct.unpack_from("<i", data, p)[0]
        if ln < 0:
            raise ValueError("l_name")
        p += 8 + ln
        need(p)
    reads = []
    while p < n:
        if n - p < 36:
            raise ValueError("record runs past the end")
        bs = struct.unpack_from("<i", data, p)[0]
        if bs < 32 or bs > n - p - 4:
            raise ValueError("block_size")
        lrn = data[p + 12]
        ncig, flag, lseq = struct.unpack_from("<HHI", data, p + 16)
        if lrn == 0 or 32 + lrn + 4 * ncig + (lseq + 1) // 2 + lseq > bs or data[p + 36 + lrn - 1] != 0:
            raise ValueError("record fields")
        if not (flag & 0x900) and lseq:
            s0 = p + 36 + lrn + 4 * ncig
            packed = data[s0:s0 + (lseq + 1) // 2]
            seq = "".join(CODES[b >> 4] + CODES[b & 15] for b in packed)[:lseq]
            reads.append(revcomp(seq) if flag & 0x10 else seq)
        p += 4 + bs
    return reads


def flat(reads, rank=0, world=1):
    """The flat block of a rank's share of the kept reads -> (bytes, number of reads)."""
    mine = [r for i, r in enumerate(reads) if (i >> SHARD_LOG2) % world == rank]
    return "".join(r + "\n" for r in mine).encode(), len(mine)


def fastq(reads, names=None):
    names = names or ["r%d" % i for i in range(len(reads))]
    return "".join("@%s\n%s\n+\n%s\n" % (nm, r, "I" * len(r)) for nm, r in zip(names, reads)).encode()


def bgzip_text(text, level=6):
    """A bgzip-style .gz of a text (members of 0xff00 bytes, EOF block)."""
    return b"".join(member(text[o:o + BLOCK], level) for o in range(0, len(text), BLOCK)) + EOF


def fastq_reads(text):
    """(names, letters) of a four-line FASTQ text, as `samtools import` would store them (upper case)."""
    lines = text.split(b"\n")
    names = [lines[i][1:].split()[0].decode() for i in range(0, len(lines) - 3, 4)]
    seqs = [lines[i].decode().upper() for i in range(1, len(lines) - 2, 4)]
    return names, seqs
