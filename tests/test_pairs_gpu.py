"""ss_reads_join_pairs_dev and ss_reads_load_pairs (ss_pairs.hip): a resident set whose records are the read pairs.  With order = 0
the set read back is held byte for byte to tests/pairs_model.py (line i of block 1, 'N', line i of block 2, in line order); the
shapes put line starts and joints on every residue modulo 16, '\\n' on the last byte of a 1024-byte tile and the first of the
next, lines over several tiles, empty mates, blocks of only '\\n' and blocks below 16 bytes (joined from a padded private copy).
The per-record calls then run on the joined set unchanged: their results equal their Python models on the joined records, and the
hits equal those of the plain set of the same two blocks."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from tests import boot_model, class_cases as cc, class_model as cm, pairs_model as pm, rs_model

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 15, 16, 17, 150, 151, 1023, 1024, 1025, 3000)
LINE_COUNTS = (0, 1, 63, 64, 65, 257, 4097)


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def dev():
    """bytes -> (device pointer or None, length); the tensors live as long as the module"""
    import torch
    keep = []

    def put(block):
        if not block:
            return None, 0
        d = torch.frombuffer(bytearray(block), dtype=torch.uint8).cuda()
        keep.append(d)
        return d.data_ptr(), len(block)
    return put


def _join(L, dev, b1, b2, order=False):
    p1, n1 = dev(b1)
    p2, n2 = dev(b2)
    return L.ReadSet.join_pairs_dev(p1, n1, p2, n2, order=order)


def _check_exact(L, dev, b1, b2):
    want = pm.join_flat(b1, b2)
    calls = L.join_pairs_calls()
    rset = _join(L, dev, b1, b2)
    try:
        assert L.join_pairs_calls() == calls + 1
        text = rset.read_back()
        info = rset.info()
        assert len(text) % 16 == 0
        assert text[:len(want)] == want
        assert text[len(want):] == b"\n" * (len(text) - len(want)) and (not want or len(text) > len(want))
        assert len(want) == len(b1) + len(b2)
        assert info["n_records"] == len(pm.lines_of(b1)) and info["n_bases"] == len(want) - info["n_records"]
        assert rset.packed_slabs() == 0
    finally:
        rset.close()
    return want


def _rand_lines(rs, lengths):
    lut = np.frombuffer(b"ACGT", np.uint8)
    return [lut[rs.randint(0, 4, size=n)].tobytes() for n in lengths]


def _blocks(n_lines, seed):
    """two blocks of n_lines lines with lengths from LENGTHS; block 1 begins 1023, 0, 1023, 1024: '\\n' at bytes 1023 and 1024 (the
    last byte of a tile and the first of the next) and again at 2047"""
    rs = np.random.RandomState(seed)
    out = []
    for mate in range(2):
        lengths = [LENGTHS[i] for i in rs.randint(0, len(LENGTHS), size=n_lines)]
        head = ((1023, 0, 1022, 1024), (0, 1024, 3000, 1))[mate]
        lengths[:len(head)] = head[:n_lines]
        out.append(b"".join(r + b"\n" for r in _rand_lines(rs, lengths)))
    return out


def _cycle_blocks():
    """2 166 lines whose lengths cycle through 0 .. 18 on either side, independently: every pair of lengths six times over"""
    rs = np.random.RandomState(19)
    n = 19 * 19 * 6
    return [b"".join(r + b"\n" for r in _rand_lines(rs, lengths)) for lengths in ([i % 19 for i in range(n)], [(i // 19) % 19 for i in range(n)])]


@pytest.mark.parametrize("n_lines", LINE_COUNTS + ("lengths_0_18",))
def test_line_order_exact(L, dev, n_lines):
    if n_lines == "lengths_0_18":
        b1, b2 = _cycle_blocks()
        _check_exact(L, dev, b1, b2)
        l1, l2 = ([len(r) for r in pm.lines_of(b)] for b in (b1, b2))
        starts = np.cumsum([0] + [a + b + 2 for a, b in zip(l1, l2)][:-1])
        assert {(a, b) for a, b in zip(l1, l2)} == {(a, b) for a in range(19) for b in range(19)}
        assert len({(int(s) % 16, a) for s, a in zip(starts, l1)}) == 16 * 19 and len({(int(s) % 16, b) for s, b in zip(starts, l2)}) == 16 * 19
        return
    b1, b2 = _blocks(n_lines, 1000 + n_lines)
    want = _check_exact(L, dev, b1, b2)
    print("lines", n_lines, "bytes", len(b1), len(b2), "joined", len(want))
    if n_lines >= 257:       # the shapes do what the docstring says
        nl1 = np.flatnonzero(np.frombuffer(b1, np.uint8) == 10)
        assert {1023, 0} <= set((nl1 % 1024).tolist())
        s1 = np.concatenate(([0], nl1[:-1] + 1))
        nl2 = np.flatnonzero(np.frombuffer(b2, np.uint8) == 10)
        s2 = np.concatenate(([0], nl2[:-1] + 1))
        starts, joints = s1 + s2, nl1 + s2
        assert set((starts % 16).tolist()) == set(range(16)) and set((joints % 16).tolist()) == set(range(16))
        assert set((s1 % 16).tolist()) == set(range(16)) and set((s2 % 16).tolist()) == set(range(16))
        assert max(np.diff(nl1)) > 2048


@pytest.mark.parametrize("n", [1, 16, 17, 2048])
def test_only_newlines(L, dev, n):
    assert _check_exact(L, dev, b"\n" * n, b"\n" * n) == b"N\n" * n
    other = b"".join(r + b"\n" for r in _rand_lines(np.random.RandomState(n), [(7 * i) % 40 for i in range(n)]))
    _check_exact(L, dev, b"\n" * n, other)
    _check_exact(L, dev, other, b"\n" * n)


@pytest.mark.parametrize("size", list(range(1, 18)))
def test_small_blocks(L, dev, size):
    """a block of 1..17 bytes against a block as small, against one of long lines, and the other way round"""
    for small, tiny, long_ in _small_cases(size):
        for other in (tiny, long_):
            _check_exact(L, dev, small, other)
            _check_exact(L, dev, other, small)


def _small_cases(size):
    """(a block of `size` bytes, a block of as many lines of 0 or 1 bytes, one of lines of 40 bytes and more) for 1, 2, size / 2
    and size lines"""
    rs = np.random.RandomState(size)
    for n_lines in sorted(n for n in {1, 2, size // 2, size} if 0 < n <= size):
        cuts = rs.choice(np.arange(size - 1), n_lines - 1, replace=False).tolist() if n_lines > 1 else []
        small = bytearray(_rand_lines(rs, [size])[0])
        for c in cuts + [size - 1]:
            small[c] = 10
        small = bytes(small)
        assert len(small) == size and len(pm.lines_of(small)) == n_lines
        tiny = b"".join(r + b"\n" for r in _rand_lines(rs, [i % 2 for i in range(n_lines)]))
        long_ = b"".join(r + b"\n" for r in _rand_lines(rs, [40 + 13 * i for i in range(n_lines)]))
        yield small, tiny, long_


def test_bytes_are_kept(L, dev):
    b1 = b"acgtACGT\r\nRYKM\nnnNN\n\n" + b"acgtnRY" * 30 + b"\r\n"
    b2 = b"\nTTTT\r\nacgtacgtacgtacgtacgt\nR\n" + b"G" * 33 + b"\n"
    want = _check_exact(L, dev, b1, b2)
    assert want.startswith(b"acgtACGT\rN\nRYKMNTTTT\r\nnnNNNacgtacgtacgtacgtacgt\nNR\n")


def test_one_length_packs(L, dev):
    g = cc.source()
    lines = cc.one_length_block(g).split(b"\n")[:-1]
    b1, b2 = (b"".join(r + b"\n" for r in part) for part in (lines[:1500], lines[1500:]))
    rset = _join(L, dev, b1, b2, order=True)
    try:
        assert rset.packed_slabs() >= 1
        got = sorted(r for r in rset.read_back().split(b"\n") if r)
        assert got == sorted(pm.join_lines(lines[:1500], lines[1500:]))
        assert rset.info()["n_records"] == 1500 and rset.info()["n_bases"] == 1500 * 301
    finally:
        rset.close()


def test_errors(L, dev):
    p1, n1 = dev(b"ACGT\nAC\n")
    p2, n2 = dev(b"ACGT\nAC\nA\n")
    p3, n3 = dev(b"ACGT\nAC")
    calls = L.join_pairs_calls()
    fn = L.lib().ss_reads_join_pairs_dev
    for args, want in (((p1, n1, p2, n2), L.SS_EIO), ((p2, n2, p1, n1), L.SS_EIO), ((p1, n1, None, 0), L.SS_EIO),
                       ((p1, n1, p3, n3), L.SS_EINVAL), ((p3, n3, p1, n1), L.SS_EINVAL),
                       ((None, n1, p1, n1), L.SS_EINVAL), ((p1, n1, None, n1), L.SS_EINVAL)):
        for order in (0, 1):
            h = C.c_void_p(1)
            assert fn(*args, order, C.byref(h)) == want, (args, order)
            assert not h.value
    assert fn(p1, n1, p1, n1, 0, None) == L.SS_EINVAL
    assert L.lib().ss_reads_join_pairs_calls(None) == L.SS_EINVAL
    assert L.join_pairs_calls() == calls            # (a refused call is no join)
    empty = L.ReadSet.join_pairs_dev(None, 0, None, 0, order=True)
    try:
        assert empty.info()["n_records"] == 0 and empty.info()["n_bases"] == 0 and empty.read_back() == b""
    finally:
        empty.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the per-record calls on the joined set

@pytest.fixture(scope="module")
def pair_sets(L, dev):
    """(J in line order, J ordered, S: the plain set of the same two blocks, the joined text, the plain text)"""
    g = cc.source()
    lines = cc.one_length_block(g).split(b"\n")[:-1]
    rag = [r for r in cc.ragged_block(g, 1).split(b"\n")[:-1]]
    half = len(rag) // 2
    l1, l2 = lines[:1500] + rag[:half], lines[1500:] + rag[half:2 * half]
    b1, b2 = (b"".join(r + b"\n" for r in part) for part in (l1, l2))
    j0, j1 = _join(L, dev, b1, b2), _join(L, dev, b1, b2, order=True)
    p, n = dev(b1 + b2)
    s = L.ReadSet.from_flat_dev(p, n, order=False)
    yield j0, j1, s, pm.join_flat(b1, b2), b1 + b2
    for r in (j0, j1, s):
        r.close()


@pytest.mark.parametrize("tname", ["k31_sampled", "k25"])
def test_invariants_and_models(L, pair_sets, tname):
    j0, j1, s, jtext, stext = pair_sets
    g = cc.source()
    k, kmers, keys, row_node = cc.table(tname, g)
    par = cc.parents()
    n_pairs = len(pm.lines_of(jtext))
    assert j0.read_back()[:len(jtext)] == jtext
    db = L.KmerDB.from_text(cc.kfa(kmers), k, True)
    try:
        counts = []
        for rset in (s, j0, j1):
            db.reset()
            rset.scan_into(db)
            L.check(L.lib().ss_device_sync(), "sync")
            counts.append(db.counts_rows().copy())
        assert counts[0].sum() > 10000
        assert np.array_equal(counts[0], counts[1]) and np.array_equal(counts[0], counts[2])
        hist_s, hits_s = s.support(db)
        want_hist, want_hits = rs_model.support_model(jtext, keys, k)
        cls_s = s.classify(db, row_node, par, 2)
        per = cm.record_hits(jtext, keys, row_node, k)
        want_cls = cm.classify_model(jtext, keys, row_node, par, cc.N_NODES, k, 2, per[0])
        for rset in (j0, j1):
            hist, hits = rset.support(db)
            assert hits == hits_s == want_hits
            assert int(hist.sum()) == n_pairs
            assert (hist == want_hist).all()
            got = rset.classify(db, row_node, par, 2)
            assert (got["node_hits"] == cls_s["node_hits"]).all()
            assert (got["node_hits"] == want_cls[1]).all() and (got["direct"] == want_cls[0]).all()
            assert int(got["direct"].sum()) == n_pairs
        assert not (hist == hist_s).all()                     # (fragments are not mates: the flag matters)
        assert not (cls_s["direct"] == want_cls[0]).all()
    finally:
        db.close()


def test_resample_moves_both_mates(L, pair_sets):
    j0, j1, _, jtext, _ = pair_sets
    want = boot_model.resampled(L, jtext, 11, 3)
    for rset in (j0, j1):
        sub = rset.resample(11, 3)
        try:
            assert sorted(r for r in sub.read_back().split(b"\n") if r) == want
        finally:
            sub.close()


# ------------------------------------------------------------------------------------------------------------------------------
# ss_reads_load_pairs

def _fastq(lines, wrap=0, crlf=False, qual_seed=None):
    rs = np.random.RandomState(qual_seed) if qual_seed is not None else None
    out = []
    for i, r in enumerate(lines):
        q = bytes(rs.randint(33 + 2, 33 + 41, size=len(r)).astype(np.uint8)) if rs is not None else b"I" * len(r)
        if wrap and len(r) > wrap:
            seq = b"\n".join(r[j:j + wrap] for j in range(0, len(r), wrap))
            qq = b"\n".join(q[j:j + wrap] for j in range(0, len(q), wrap))
        else:
            seq, qq = r, q
        out.append(b"@r%d\n" % i + seq + b"\n+\n" + qq + b"\n")
    text = b"".join(out)
    return text.replace(b"\n", b"\r\n") if crlf else text


def _fasta(lines, wrap=60):
    return b"".join(b">r%d\n" % i + b"".join(r[j:j + wrap] + b"\n" for j in range(0, len(r), wrap)) for i, r in enumerate(lines))


def _load_case(L, dev, tmp_path, name, t1, t2, gz=False):
    paths = []
    for m, t in enumerate((t1, t2)):
        p = str(tmp_path / ("%s_%d.%s" % (name, m + 1, "fq.gz" if gz else "fq")))
        if gz:
            with gzip.GzipFile(p, "wb", compresslevel=1, mtime=0) as f:
                f.write(t)
        else:
            with open(p, "wb") as f:
                f.write(t)
        paths.append(p)
    flats = [L.fastx_to_flat(t)[0] for t in (t1, t2)]
    flats = [bytes(f) for f in flats]
    ref = _join(L, dev, flats[0], flats[1])
    got = L.ReadSet.load_pairs(paths[0], paths[1], order=False)
    try:
        a, b = got.read_back(), ref.read_back()
        assert a == b and got.info() == ref.info()
        assert a[:len(flats[0]) + len(flats[1])] == pm.join_flat(flats[0], flats[1])
    finally:
        got.close()
        ref.close()
    return paths


def test_load_pairs_small_files(L, dev, tmp_path):
    rs = np.random.RandomState(5)
    l1 = _rand_lines(rs, [150] * 300 + [0, 75, 151])
    l2 = _rand_lines(rs, [150] * 150 + [0] + [149] * 149 + [33, 0, 151])
    _load_case(L, dev, tmp_path, "plain", _fastq(l1), _fastq(l2))
    _load_case(L, dev, tmp_path, "gz", _fastq(l1), _fastq(l2), gz=True)
    _load_case(L, dev, tmp_path, "wrapped", _fastq(l1, wrap=70), _fasta(l2))
    _load_case(L, dev, tmp_path, "crlf", _fastq(l1, crlf=True), _fastq(l2))
    L.set_min_base_qual(20)
    try:
        paths = _load_case(L, dev, tmp_path, "q20", _fastq(l1, qual_seed=1), _fastq(l2, qual_seed=2))
        masked = L.ReadSet.load_pairs(paths[0], paths[1], order=False)
        text = masked.read_back()
        masked.close()
    finally:
        L.set_min_base_qual(0)
    plain = L.ReadSet.load_pairs(paths[0], paths[1], order=False)
    try:
        assert plain.read_back() != text and plain.read_back().count(b"N") < text.count(b"N")
    finally:
        plain.close()


def test_load_pairs_chunked_route(L, dev, tmp_path):
    """files of 9 million bytes of four-line FASTQ each: more than one 8 MiB chunk of the parallel parse, put together by chunk index"""
    rs = np.random.RandomState(6)
    n = 29000
    src = np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, size=400000)]
    starts = rs.randint(0, src.size - 150, size=(2, n))
    mates = [[src[s:s + 150].tobytes() for s in row] for row in starts]
    t1, t2 = _fastq(mates[0]), _fastq(mates[1])
    assert min(len(t1), len(t2)) > (8 << 20) + 500000
    paths = _load_case(L, dev, tmp_path, "big", t1, t2)
    ordered = L.ReadSet.load_pairs(paths[0], paths[1])
    try:
        assert ordered.packed_slabs() >= 1 and ordered.info()["n_records"] == n
    finally:
        ordered.close()


def test_load_pairs_errors(L, tmp_path):
    rs = np.random.RandomState(7)
    a, b = tmp_path / "a.fq", tmp_path / "b.fq"
    a.write_bytes(_fastq(_rand_lines(rs, [50] * 10)))
    b.write_bytes(_fastq(_rand_lines(rs, [50] * 11)))
    bam = tmp_path / "x.bam"
    bam.write_bytes(b"BAM\1" + b"\0" * 60)
    fn = L.lib().ss_reads_load_pairs
    for p1, p2, want in ((a, b, L.SS_EIO), (a, tmp_path / "missing.fq", L.SS_EIO), (a, bam, L.SS_EINVAL), (bam, a, L.SS_EINVAL)):
        h = C.c_void_p(1)
        assert fn(os.fsencode(str(p1)), os.fsencode(str(p2)), 1, C.byref(h)) == want, (p1, p2)
        assert not h.value
    assert fn(None, os.fsencode(str(a)), 1, C.byref(h)) == L.SS_EINVAL
