"""The device gzip inflater (strainscan_amd/csrc/ss_ginflate.hip with ss_ginflate_dev.h) on DEFLATE streams whose every bit the
test chose (tests/deflate_streams.py, written with tests/deflate_writer.py), against zlib.

test_ginflate_gpu.py feeds it zlib's own compressor on one FASTQ generator and accepts "declined" in several places; a decoder
bug does not produce wrong text there but a CRC mismatch, a decline and the host inflaters, twenty times slower, and the suite
stays green.  Here every stream lies inside the documented contract -- one member, under 8 MB, and no 4096 bytes of deflate
data produce more than 8 x 4096 bytes of text, which test_deflate_streams_host.py asserts from the writer's records against the
SYM_RATIO = 12 symbols per byte (+ 4096 per chunk) that the driver reserves -- so for every case: SS_OK, the bytes zlib gives,
the handled counter + 1, the declined counter + 0.  A decline is a failure.

What these cases see, tried with value-only changes to ss_ginflate_dev.h on a copy: len_code giving 257 for symbol 285 and
tails_kernel's short-chunk branch without its "+ L" pass test_ginflate_gpu.py untouched and fail here (the first in every
writer-made case, the second in heirloom, mixed and most seeds at 4096-byte chunks); lane_long counting to 13, copy_match
without "% dist" and read_dynamic without its `prev` carry fail in both files.  One change no stream can see: taking a match of
at most FAR_MAX symbols the far way from RING_REACH on instead of RING_REACH + length - 1.  Its sources lie 1773 symbols or more
in front of the window, a wave never holds more than 1024 + WIN_MAX unflushed symbols, so the far way loads from global memory
exactly what the ring still holds: the bound is a safety margin, not a value (every_length_and_distance has those distances).

The cases name what they hold (deflate_streams.py builds them, the host test asserts that the shapes are really there), with
these constants of ss_ginflate_dev.h / ss_ginflate.hip, restated here in one place so that the edges move with them:"""
import ctypes as C
import os

import pytest

from tests import deflate_streams as ds

pytestmark = pytest.mark.gpu

SS_OK = 0
LITBITS, DISTBITS = 9, 8        # the direct tables of the literal/length and of the distance code: longer codes go through lane_long
RING, RING_REACH = 2048, 1784   # symbols of a wave in LDS; a match at most RING_REACH back reads them there
WIN_MAX = 264                   # a 64-position window that delivers more symbols goes item by item
FAR_MAX = 12                    # the longest match whose symbols are loaded together from beyond the ring's reach
SYM_RATIO, PROBE, MIN_GROUP = 12, 512, 8      # the driver's symbol budget, the sync search's probe, the smallest group of window maps
assert (ds.RING_REACH, ds.FAR_MAX, ds.WIN_MAX) == (RING_REACH, FAR_MAX, WIN_MAX) and RING - RING_REACH == WIN_MAX

# every case at the default chunking; a case of several blocks also with 4096-byte search chunks (nearly every chunk then holds
# an entry: tens of chunks, windows handed from chunk to chunk and from group to group) and without entries inside blocks
VARIANTS = dict(default={}, chunk4096=dict(SS_GZ_CHUNK="4096"), split0=dict(SS_GZ_SPLIT_KB="0"))
CASES = [(name, v) for name in ds.ALL for v in VARIANTS]


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _counters(L):
    a, b = C.c_uint64(), C.c_uint64()
    L.check(L.lib().ss_gz_gpu_counters(C.byref(a), C.byref(b)), "ss_gz_gpu_counters")
    return int(a.value), int(b.value)


@pytest.mark.parametrize("name,variant", CASES, ids=["%s-%s" % c for c in CASES])
def test_stream(L, tmp_path, monkeypatch, name, variant):
    s = ds.stream(name)
    assert s.n_blocks is None or s.n_blocks > 1          # (every stream has several blocks: every variant applies)
    for key in ("SS_GZ_CHUNK", "SS_GZ_SPLIT_KB", "SS_GZ_SEG_KB", "SS_GZ_NO_RUNOVER"):
        monkeypatch.delenv(key, raising=False)
    for key, value in VARIANTS[variant].items():
        monkeypatch.setenv(key, value)                   # (the driver reads both on every call)
    p = tmp_path / (name + ".gz")
    p.write_bytes(s.member)
    handled, declined = _counters(L)
    t, n = C.c_void_p(), C.c_uint64()
    rc = L.lib().ss_gz_inflate_gpu(os.fsencode(str(p)), C.byref(t), C.byref(n))
    assert rc == SS_OK, "declined (SS_INGEST_TRACE=1 prints the reason)" if rc == -34 else rc
    got = C.string_at(t, n.value)
    L.lib().ss_gz_free(t)
    assert len(got) == len(s.text) and got == s.text
    assert _counters(L) == (handled + 1, declined)
