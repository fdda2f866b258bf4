"""ss_bgzf_write (ss_bam_out.hip, host only): head + body as BGZF -- members of at most 0xff00 stream bytes and 65536 file
bytes, each with the "BC" field and the right BSIZE, CRC-32 and ISIZE, then the 28-byte EOF block; gzip.decompress gives head +
body back; a path that cannot be written gives SS_EIO and leaves no file."""
import gzip
import os
import struct
import zlib

import pytest

from tests import bamio

BLOCK = 0xff00
SIZES = [0, 1, BLOCK - 1, BLOCK, BLOCK + 1, 300 * 1024 + 7]
HEAD = bamio.header()


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.lib()
    return _lib


def _body(kind, n):
    if kind == "random":
        return os.urandom(n)
    line = b"ACGTTGCAAGGCTTAACCGGTTAGACTAGGATCCA\tread name %d\n"
    text = b"".join(line % i for i in range(n // 40 + 2))
    return text[:n]


def _members(data):
    """[(stream bytes of the member)] of a BGZF file, every field checked on the way; the EOF block comes back as b''"""
    out, o = [], 0
    while o < len(data):
        assert data[o:o + 4] == b"\x1f\x8b\x08\x04", o
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        assert xlen == 6 and data[o + 12:o + 16] == b"BC\x02\0", o
        bsize = struct.unpack_from("<H", data, o + 16)[0] + 1
        assert 26 <= bsize <= 65536 and o + bsize <= len(data), (o, bsize)
        raw = zlib.decompressobj(-15)
        text = raw.decompress(data[o + 18:o + bsize - 8])
        assert raw.eof and not raw.unused_data, o
        crc, isize = struct.unpack_from("<II", data, o + bsize - 8)
        assert isize == len(text) <= BLOCK and crc == zlib.crc32(text) & 0xffffffff, o
        out.append(text)
        o += bsize
    return out


@pytest.mark.parametrize("level", [0, 1, 6])
@pytest.mark.parametrize("kind", ["text", "random"])
@pytest.mark.parametrize("size", SIZES)
def test_members_and_round_trip(L, tmp_path, size, kind, level):
    body = _body(kind, size)
    assert len(body) == size
    p = tmp_path / "out.bam"
    L.bgzf_write(str(p), HEAD, body, level)
    data = p.read_bytes()
    assert data.endswith(bamio.EOF)
    assert gzip.decompress(data) == HEAD + body
    m = _members(data)
    assert m[-1] == b"" and all(m[:-1])
    assert b"".join(m) == HEAD + body
    # the header has members of its own: the first record starts a member
    assert m[0] == HEAD
    assert len(m) == 1 + (size + BLOCK - 1) // BLOCK + 1
    if kind == "text" and level and size >= BLOCK:
        assert len(data) < size // 2
    if level == 0:
        assert len(data) > size


def test_empty_head_and_body_is_the_eof_block(L, tmp_path):
    p = tmp_path / "e.bam"
    L.bgzf_write(str(p), b"", b"", 1)
    assert p.read_bytes() == bamio.EOF


def test_threads_give_the_same_file(L, tmp_path, monkeypatch):
    body = _body("text", 20 * 1024 * 1024)
    monkeypatch.setenv("SS_HOST_THREADS", "1")
    L.bgzf_write(str(tmp_path / "a"), HEAD, body, 1)
    monkeypatch.setenv("SS_HOST_THREADS", "7")
    L.bgzf_write(str(tmp_path / "b"), HEAD, body, 1)
    a, b = (tmp_path / "a").read_bytes(), (tmp_path / "b").read_bytes()
    assert a == b and gzip.decompress(a) == HEAD + body


def test_unwritable_path_and_bad_level(L, tmp_path):
    p = tmp_path / "no_such_dir" / "out.bam"
    with pytest.raises(L.SSError) as e:
        L.bgzf_write(str(p), HEAD, b"abc", 1)
    assert e.value.code == L.SS_EIO
    assert not os.path.exists(str(p)) and not os.path.exists(os.path.dirname(str(p)))
    for level in (-1, 10):
        with pytest.raises(L.SSError) as e:
            L.bgzf_write(str(tmp_path / "x.bam"), HEAD, b"abc", level)
        assert e.value.code == L.SS_EINVAL
    assert not os.path.exists(str(tmp_path / "x.bam"))
