"""BAM input without a GPU: the writer and the reference decoder of tests/bamio.py against hand-checked records and each
other, the host decoder of the library (ss_bam_decode) against the reference decoder for every writer option and shard,
damaged streams, CRAM refusal, and how ss_input_kind tells the formats apart."""
import gzip
import struct

import numpy as np
import pytest

from tests import bamio


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.lib()
    return _lib


def _reads(seed, n, lo=20, hi=300, iupac=False):
    rs = np.random.RandomState(seed)
    alpha = bamio.CODES if iupac else "ACGT"
    out = []
    for i in range(n):
        ln = int(rs.randint(lo, hi))
        s = "".join(alpha[j] for j in rs.randint(0, len(alpha), size=ln))
        out.append(("read%d%s" % (i, "x" * int(rs.randint(0, 40))), s))
    return out


def test_hand_checked_record():
    r = bamio.record("q1", "ACGTN", flag=0x10, ref=0, pos=7, cigar=(5 << 4,))
    bs = struct.unpack_from("<i", r)[0]
    assert bs == len(r) - 4 == 32 + 3 + 4 + 3 + 5
    assert r[4 + 32:4 + 35] == b"q1\0"
    assert r[4 + 39:4 + 42] == bytes([0x12, 0x48, 0xF0])          # A C | G T | N pad
    data = bamio.bgzf(bamio.header(), [r, bamio.record("q2", "ACMGRSVTWYHKDBN=", flag=4)], level=0)
    assert gzip.decompress(data)[:4] == b"BAM\1"
    assert bamio.decode(data) == ["NACGT", "ACMGRSVTWYHKDBN="]
    # complement = the four bits reversed
    for i, c in enumerate(bamio.CODES):
        rev = int("{:04b}".format(i)[::-1], 2)
        assert c.translate(bamio.COMP) == bamio.CODES[rev]


def test_skips_and_keeps():
    recs = [bamio.record("a", "ACGT", flag=0x100), bamio.record("b", "CCCC", flag=0x800), bamio.record("c", "", flag=4),
            bamio.record("d", "GGGA", flag=0x200), bamio.record("e", "TTTA", flag=0x400), bamio.record("f", "AACC", flag=0x10)]
    assert bamio.decode(bamio.bgzf(bamio.header(), recs)) == ["GGGA", "TTTA", "GGTT"]


OPTIONS = [
    dict(level=0, cuts="htslib", aligned=False, decoys=0.0, extras=False, eof=True),
    dict(level=6, cuts="htslib", aligned=True, decoys=0.2, extras=True, eof=True),
    dict(level=6, cuts="random", aligned=True, decoys=0.2, extras=True, eof=False),
    dict(level=0, cuts="random", aligned=False, decoys=0.1, extras=True, eof=True, iupac=True),
    dict(level=6, cuts="htslib", aligned=True, decoys=0.0, extras=False, eof=True, long=True),
    dict(level=6, cuts="random", aligned=False, decoys=0.0, extras=False, eof=True, long=True),
]


def _sample(opt, seed, n=9000):
    reads = _reads(seed, n, iupac=opt.get("iupac", False))
    if opt.get("long"):
        reads = reads[:300] + _reads(seed + 1, 6, lo=70000, hi=140000) + reads[300:600]
    recs = bamio.sample_records(seed, reads, aligned=opt["aligned"], decoys=opt["decoys"], extras=opt["extras"])
    data = bamio.bgzf(bamio.header(), recs, level=opt["level"], cuts=opt["cuts"], eof=opt["eof"], seed=seed)
    return reads, data


@pytest.mark.parametrize("oi", range(len(OPTIONS)))
def test_host_decoder_equals_reference(L, oi):
    reads, data = _sample(OPTIONS[oi], 100 + oi)
    got = bamio.decode(data)
    assert got == [s for _, s in reads]
    stream = gzip.decompress(data)
    for world in (1, 2, 3):
        for rank in range(world):
            want, nw = bamio.flat(got, rank, world)
            flat, nrec = L.bam_decode(stream, rank, world)
            assert nrec == nw and flat == want, (oi, rank, world)


def _damaged(kind):
    recs = [bamio.record("r%d" % i, "ACGT" * 20) for i in range(50)]
    hdr = bamio.header()
    stream = hdr + b"".join(recs)
    o = len(hdr) + len(recs[0]) * 7                  # the 8th record
    s = bytearray(stream)
    if kind == "block_size_small":
        s[o:o + 4] = struct.pack("<i", 31)
    elif kind == "block_size_fields":
        s[o:o + 4] = struct.pack("<i", 40)
    elif kind == "name_not_nul":
        s[o + 4 + 32 + 2] = ord("x")                 # "r7\0" -> "r7x"
    elif kind == "l_read_name_0":
        s[o + 12] = 0
    elif kind == "past_end":
        s = s[:-7]
    elif kind == "no_magic":
        s[0:4] = b"BAN\1"
    return bytes(s)


DAMAGE = ["block_size_small", "block_size_fields", "name_not_nul", "l_read_name_0", "past_end", "no_magic"]


@pytest.mark.parametrize("kind", DAMAGE)
def test_damaged_streams_raise(L, kind):
    s = _damaged(kind)
    with pytest.raises(ValueError):
        bamio.decode(s)
    with pytest.raises(L.SSError) as e:
        L.bam_decode(s)
    assert e.value.code == L.SS_EIO


def test_member_crc_and_length_are_checked(tmp_path):
    recs = [bamio.record("r%d" % i, "ACGT" * 20) for i in range(50)]
    data = bytearray(bamio.bgzf(bamio.header(), recs, level=0))
    bad_crc = bytearray(data)
    bad_crc[len(data) - 28 - 8] ^= 1               # the last data member's CRC-32
    with pytest.raises(ValueError):
        bamio.decode(bytes(bad_crc))
    bad_len = bytearray(data)
    bad_len[len(data) - 28 - 4] ^= 1               # ... and its ISIZE
    with pytest.raises(ValueError):
        bamio.decode(bytes(bad_len))


def test_input_kind(L, tmp_path):
    recs = [bamio.record("r%d" % i, "ACGT" * 20) for i in range(5)]
    p = tmp_path / "x.reads"                       # (not the extension: the inflated magic decides)
    p.write_bytes(bamio.bgzf(bamio.header(), recs))
    assert L.input_kind(str(p)) == "bam"
    raw = tmp_path / "raw.bin"
    raw.write_bytes(bamio.header() + b"".join(recs))
    assert L.input_kind(str(raw)) == "bam"
    fq = tmp_path / "a.fastq.gz"
    fq.write_bytes(gzip.compress(b"@r\nACGT\n+\nIIII\n"))
    assert L.input_kind(str(fq)) == "fastx"
    bfq = tmp_path / "b.fq.gz"
    bfq.write_bytes(bamio.bgzip_text(b"@r\nACGT\n+\nIIII\n"))
    assert L.input_kind(str(bfq)) == "fastx"
    cram = tmp_path / "c.cram"
    cram.write_bytes(b"CRAM\3\0" + b"\0" * 40)
    assert L.input_kind(str(cram)) == "cram"
    assert L.input_kind(str(tmp_path / "missing")) == "fastx"


def test_cram_is_refused(L, tmp_path):
    cram = tmp_path / "s.cram"
    cram.write_bytes(b"CRAM\3\0" + b"\0" * 40)
    with pytest.raises(ValueError, match="CRAM"):
        L.refuse_cram([str(cram), ""])
    L.refuse_cram([str(tmp_path / "missing"), ""])      # (not this check's business)
    from strainscan_amd import multi_db
    db = tmp_path / "db"
    (db / "Tree_database").mkdir(parents=True)
    with pytest.raises(SystemExit) as e:
        multi_db.main(["-i", str(cram), "-d", str(db), "-o", str(tmp_path / "o")])
    assert e.value.code == 2
    assert not (tmp_path / "o").exists()
