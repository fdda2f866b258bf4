"""The hand-built DEFLATE streams of tests/deflate_streams.py (written with tests/deflate_writer.py) on the CPU: zlib is the
reference -- every stream inflates to the writer's own replay of its tokens --, every stream keeps the budget that the device
inflater's contract names (so that test_ginflate_streams_gpu.py can call a decline a failure), every shape a case promises is
really in its stream (asserted from the writer's bit positions and block records), and the host inflaters -- libdeflate through
ss_gz_inflate mode 2, the threaded two-pass inflater of ss_pgz.hip through mode 1 -- handle them."""
import gzip
import random
import zlib

import pytest

from tests import deflate_streams as ds
from tests import deflate_writer as dw


def test_writer_against_zlib_bit_by_bit():
    """The shapes zlib's own compressor never writes, one block each: 15-bit codes of all three kinds in one block, both spellings
    of 258, distance 32768, a literal-only block with one distance length of 0, a single 1-bit distance code, an empty block whose
    literal/length code is the end-of-block symbol alone."""
    rng = random.Random(1)
    w = dw.DeflateWriter()
    w.stored(rng.randbytes(40000))
    lit = dw.chain_code(list(range(65, 78)) + [256, 285, 284], 286)
    dist = dw.chain_code(list(range(14)) + [29, 28], 30)
    assert lit[285] == lit[284] == 15 and dist[29] == dist[28] == 15 and lit[77] == 13
    toks = [("L", rng.randrange(65, 78)) for _ in range(500)]
    toks += [("M", 285, 0, 29, 8191), ("M", 284, 31, 29, 0), ("M", 284, 30, 28, 8191), ("M", 284, 31, 13, 31)]
    assert [dw.token_length(t) for t in toks[-4:]] == [258, 258, 257, 258] and dw.token_distance(toks[-4]) == 32768
    w.dynamic(lit, dist, toks)
    w.dynamic(dw.flat_code(list(range(127)) + [256], 257), [0], [("L", rng.randrange(127)) for _ in range(300)])
    w.dynamic(dw.flat_code(list(range(126)) + [256, 257], 258), [1], [("L", 65), ("M", 257, 0, 0, 0), ("L", 66)])
    eob_only = [0] * 257
    eob_only[256] = 1
    w.dynamic(eob_only, [0], [])
    w.fixed([("L", 200), dw.match(258, 1), dw.match(3, 32768)], final=True)
    assert [b[0] for b in w.blocks] == ["stored", "dynamic", "dynamic", "dynamic", "dynamic", "fixed"]
    assert w.blocks[4][3] == 0 and w.blocks[3][3] == 5
    text = dw.expected(toks, bytes(w.text[:40000]))
    assert bytes(w.text[:len(text)]) == text
    assert zlib.decompress(w.raw(), -15) == bytes(w.text)
    assert gzip.decompress(w.gzip()) == bytes(w.text)
    # the code helpers: complete, within 15 bits, and what a decoder makes of the run-length items is the lengths
    for seed in range(50):
        r = random.Random(seed)
        syms = r.sample(range(286), r.randint(2, 286))
        lens = dw.random_code(r, syms, 286, deep=r.random())
        assert dw.kraft(lens) == 32768 and max(lens) <= 15 and sorted(s for s in range(286) if lens[s]) == sorted(syms)
        assert dw.cl_items_lengths(dw.plain_cl_items(lens)) == lens
    assert sorted(x for x in dw.chain_code(range(16), 16)) == list(range(1, 15)) + [15, 15]


@pytest.mark.parametrize("name", list(ds.ALL))
def test_stream_is_what_zlib_reads_and_keeps_the_budget(name):
    s = ds.stream(name)
    assert zlib.decompress(s.raw, -15) == s.text          # (s.text is the writer's replay of its own tokens)
    assert gzip.decompress(s.member) == s.text
    assert len(s.member) < (8 << 20)                      # far from the "lonely stretch" rule
    if name not in ("heirloom",) and not name.startswith("zlib_mem1"):
        assert (30 << 10) <= len(s.raw) <= (310 << 10), len(s.raw)
    bits, outs = s.writer.trace() if s.writer else ds.zlib_trace(s.raw)
    worst, excess = ds.budget_figures(bits, outs)
    print("%s: %d bytes of deflate data, %d of text; most text from 4096 bytes: %d; excess over 12 per byte: %.0f" % (name, len(s.raw), len(s.text), worst, excess))
    assert worst <= 8 * 4096
    assert excess <= 4096
    if s.writer:
        b = s.writer.blocks
        assert b[0][1] == 0 and all(x[2] == y[1] for x, y in zip(b, b[1:])) and sum(x[3] for x in b) == len(s.text)
        assert -(-b[-1][2] // 8) == len(s.raw)


def test_the_named_shapes_are_in_their_streams():
    n = ds.stream("long_codes").notes["seen"]
    assert {9, 10, 15} <= n["lit"] and {15} <= n["length"] and {8, 9, 15} <= n["dist"]
    assert n["lit"] >= set(range(1, 16)) and n["dist"] >= set(range(1, 16))
    assert {0x00, 0x7F, 0x80, 0xFF} <= set(ds.stream("long_codes").text)

    starts = ds.stream("widest_item").notes["starts"]          # first bits of the 48-bit items, as bit positions of the FILE
    assert {p % 32 for p in starts} == set(range(32))
    across = lambda p, k: p // (8 * k) != (p + 47) // (8 * k)
    assert sum(across(p, 512) and not across(p, 1024) for p in starts) >= 5 and sum(across(p, 1024) for p in starts) >= 5
    raw = ds.stream("widest_item").raw
    for p in starts[:3]:                                       # ... and the item really is there: 15 one-bits begin the 15-bit code
        q = p - ds.GZIP_HEADER_BITS
        assert (int.from_bytes(raw[q // 8:q // 8 + 4], "little") >> (q % 8)) & 0x3FFF == 0x3FFF

    jobs = ds.stream("every_length_and_distance").notes["jobs"]
    pairs = {(dw.token_length(t), dw.token_distance(t)) for t in jobs}
    assert {p[0] for p in pairs} == set(range(3, 259))
    assert {(t[1], t[2]) for t in jobs} >= {(285, 0), (284, 31)}
    for d_sym in range(30):
        assert {(d_sym, 0), (d_sym, (1 << dw.DIST_EXTRA[d_sym]) - 1)} <= {(t[3], t[4]) for t in jobs}
    for length in (ds.FAR_MAX, ds.FAR_MAX + 1):
        for d in (ds.RING_REACH - 1, ds.RING_REACH, ds.RING_REACH + 1, ds.RING_REACH + length - 1, ds.RING_REACH + length, 2047, 2048, 2049, 32767, 32768):
            assert (length, d) in pairs
    assert set(ds.stream("overlap").notes["pairs"]) == {(d, n) for d in (1, 2, 3, 63, 64, 65, 257) for n in (3, 64, 65, 258) if d < n}

    kinds = dict(ds.stream("header_shapes").notes["kinds"])
    assert kinds["literal_only"]["hlit"] == 257 and kinds["literal_only"]["hdist"] == 1 and kinds["empty"]["hlit"] == 257
    assert kinds["hlit_286_hdist_30"]["hlit"] == 286 and kinds["hlit_286_hdist_30"]["hdist"] == 30
    assert kinds["hclen_19"]["hclen"] == 19 > kinds["hclen_smallest"]["hclen"] and kinds["hclen_19"]["items"] == kinds["hclen_smallest"]["items"]
    assert {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)} <= set(kinds["runs_min_max"]["items"])

    def crossing(h, v):          # a run-length item of kind v that begins in the literal lengths and ends in the distance lengths
        at = 0
        for item in h["items"]:
            if item[0] == v and at < h["hlit"] < at + item[1]:
                return True
            at += item[1]
        return False
    assert crossing(kinds["zero_run_crosses"], 18) and crossing(kinds["copy_run_crosses"], 16)
    h = kinds["copies_in_a_row"]
    run = [b for (v, k), b in zip(h["items"], h["item_bits"]) if v == 16][:33]
    assert len(run) == 33 and run[-1] - run[0] > 2 * 64          # the copies span more than two of the parser's 64-position windows

    pads = ds.stream("stored_blocks").notes["pads"]
    assert {p for p in pads if p[0] != 65535} == {(n, a) for n in (0, 1, 1023, 1024, 1025) for a in range(8)} and (65535, 0) in pads and (65535, 5) in pads
    assert ds.stream("stored_blocks").writer.blocks[-1][0] == "stored"
    u = ds.stream("fixed_between").notes["used"]
    assert u["length"] >= set(range(280, 286)) and u["dist"] == set(range(30))
    hl = ds.stream("heirloom")
    assert len(hl.raw) >= 80 * 4096 + 32768
    assert ds.budget_figures(*hl.writer.trace())[0] < 32768 // 2          # a 4096-byte chunk's text is far shorter than the window
    assert all(2048 <= (x[2] - x[1]) // 8 <= 3200 for x in hl.writer.blocks[1:-1])
    sizes = ds.stream("tiny_blocks").notes["sizes"]
    assert min(sizes) == 1 and max(sizes) == 600 and {511, 512, 513} <= set(sizes)
    assert {"stored", "fixed", "dynamic"} == {b[0] for b in ds.stream("mixed").writer.blocks}


@pytest.fixture(scope="module")
def host_lib():
    from strainscan_amd import _lib
    return _lib


@pytest.mark.parametrize("name", list(ds.NAMED))
def test_named_streams_through_libdeflate(host_lib, tmp_path, name):
    """ss_gz_inflate mode 2 (libdeflate only): handled, and equal."""
    s = ds.stream(name)
    p = tmp_path / (name + ".gz")
    p.write_bytes(s.member)
    got = host_lib.gz_inflate(str(p), 0, 2)
    assert got is not None, "declined"
    assert got == s.text


def test_long_stream_through_the_threaded_inflater(host_lib, tmp_path):
    """ss_gz_inflate mode 1 (ss_pgz.hip: entry points searched in the stream, chunks decoded against an unknown window by two threads):
    over 4 MB of deflate data in pigz's layout, made of blocks no compressor writes -- ss_gz_inflate gives a thread 2 MB of input at
    least, ss_pgz.hip wants 1 MB per thread.  Handled, and equal."""
    s = ds.long_stream()
    assert len(s.raw) >= (4 << 20) + 64
    assert zlib.decompress(s.raw, -15) == s.text
    p = tmp_path / "long.gz"
    p.write_bytes(s.member)
    got = host_lib.gz_inflate(str(p), 2, 1)
    assert got is not None, "declined"
    assert got == s.text
