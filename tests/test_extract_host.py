"""The host half of -x / --extract_reads (ss_extract.hip), which needs no device: record digests (ss_flat_record_keys), the writer
(ss_extract_write) against a Python filter of the same text, pairs, the base-quality mask, failure leaving nothing behind, the
flag's handling, and the record walker under AddressSanitizer + UBSan as a stand-alone program (tests/extract_fuzz.cpp)."""
import argparse
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    return _lib


def _rand(rs, n):
    return np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, size=n)].tobytes()


def _qual(rs, n):
    return np.frombuffer(b"5678ABCDEFGHIJ", np.uint8)[rs.randint(0, 14, size=n)].tobytes()      # (nothing below Phred 20)


def _wrap(s, w, eol):
    return b"".join(s[i:i + w] + eol for i in range(0, len(s), w))


def _keys_of(L, flats):
    return L.flat_record_keys(b"".join(f + b"\n" for f in flats))


# ---------------------------------------------------------------------------------------------- digests


def test_digests(L):
    k = L.flat_record_keys(b"ACGT\nACGTAC\n\nACGT\nacgt\nACGT\r\nACG\n")
    assert k.shape == (6, 2) and k.dtype == np.uint64      # (the empty record has none)
    rows = [tuple(r) for r in k.tolist()]
    assert rows[0] == rows[2]                              # equal flat records
    assert rows[0] != rows[1] and rows[0] != rows[5]       # a record and its prefix, either way
    assert rows[0] != rows[3]                              # ACGT / acgt
    assert rows[0] != rows[4]                              # ACGT / ACGT\r
    assert len(set(rows)) == 5
    assert len({r[0] for r in rows}) == 5 and len({r[1] for r in rows}) == 5      # each 64-bit half tells them apart on its own
    assert all(r[0] != r[1] for r in rows)
    assert L.flat_record_keys(b"").shape == (0, 2) and L.flat_record_keys(b"\n\n").shape == (0, 2)
    assert (L.flat_record_keys(b"ACGT") == k[0]).all()     # a last record without its '\n'


def test_digests_tell_many_records_apart(L):
    """20 000 records that differ in one base, in their length by one, or in case: no two digests agree in either half"""
    rs = np.random.RandomState(3)
    base = bytearray(_rand(rs, 150))
    recs = set()
    for i in range(150):
        for c in b"ACGTacgtN":
            r = bytearray(base)
            r[i] = c
            recs.add(bytes(r))
    recs |= {bytes(base[:n]) for n in range(1, 150)}
    while len(recs) < 20000:
        recs.add(_rand(rs, int(rs.randint(1, 300))))
    recs = sorted(recs)
    k = _keys_of(L, recs)
    assert k.shape == (len(recs), 2)
    assert np.unique(k[:, 0]).size == len(recs) and np.unique(k[:, 1]).size == len(recs)


def test_keys_capacity(L):
    import ctypes as C
    flat = b"AC\nGT\nTT\n"
    n = C.c_uint64()
    keys = np.zeros((2, 2), np.uint64)
    rc = L.lib().ss_flat_record_keys(flat, len(flat), L.ptr(keys), 2, C.byref(n))
    assert rc == L.SS_ERANGE and n.value == 3
    assert (keys == L.flat_record_keys(flat)[:2]).all()


# ---------------------------------------------------------------------------------------------- the writer


def _cases():
    """name -> [(record text, flat form)]: the record's original text and what the loader's grammar makes of it"""
    rs = np.random.RandomState(17)
    out = {}
    recs = []
    for i in range(60):
        s = _rand(rs, int(rs.randint(1, 200)))
        q = _qual(rs, len(s))
        if i == 7:
            q = b"@" + q[1:]                       # a quality line that begins like a header
        if i == 9:
            q = b"+" + q[1:]
        recs.append((b"@r%d some text\n%s\n+\n%s\n" % (i, s, q), s))
    out["fastq4"] = recs
    recs = []
    for i in range(40):
        s = _rand(rs, int(rs.randint(1, 400)))
        q = _qual(rs, len(s))
        recs.append((b"@m%d\n" % i + _wrap(s, 50, b"\n") + b"+m%d\n" % i + _wrap(q, 50, b"\n"), s))
    out["fastq_multiline"] = recs
    recs = []
    for i in range(40):
        s = _rand(rs, int(rs.randint(1, 500)))
        recs.append((b">s%d wrapped at 60\n" % i + _wrap(s, 60, b"\n"), s))
    out["fasta60"] = recs
    recs = []
    for i in range(30):
        s = _rand(rs, int(rs.randint(1, 200)))
        q = _qual(rs, len(s))
        recs.append((b"@c%d\r\n%s\r\n+\r\n%s\r\n" % (i, s, q), s + b"\r"))
    out["fastq_crlf"] = recs
    recs = []
    for i in range(20):
        s = _rand(rs, int(rs.randint(61, 200)))
        recs.append((b">c%d\r\n" % i + _wrap(s, 60, b"\r\n"), b"".join(s[j:j + 60] + b"\r" for j in range(0, len(s), 60))))
    out["fasta_crlf"] = recs
    recs = []
    for i in range(30):
        s = _rand(rs, int(rs.randint(1, 200)))
        if i % 2:
            s = s.lower()
        elif i % 3 == 0:
            s = s[:len(s) // 2] + b"NRYn" + s[len(s) // 2:].lower()
        recs.append((b"@l%d\n%s\n+\n%s\n" % (i, s, _qual(rs, len(s))), s))
    out["lower_case"] = recs
    recs = list(out["fastq4"][:10])
    recs.insert(3, (b"@empty\n\n+\n\n", b""))
    recs.insert(8, (b"@empty2\n\n+\n\n", b""))
    out["empty_sequence"] = recs
    recs = list(out["fastq4"][20:30])
    recs[-1] = (recs[-1][0][:-1], recs[-1][1])          # the last record without its newline
    out["no_final_newline"] = recs
    recs = list(out["fasta60"][:10])
    recs[-1] = (recs[-1][0][:-1], recs[-1][1])
    out["fasta_no_final_newline"] = recs
    return out


CASES = _cases()


def _written_text(recs, chosen):
    """the Python filter: the text of every record with bases whose flat form was chosen (an empty record's own empty quality
    line belongs to no record and is never written)"""
    return b"".join(t for t, f in recs if f and f in chosen)


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_writer_equals_filter(L, tmp_path, case, gz):
    recs = CASES[case]
    text = b"".join(t for t, _ in recs)
    # the flat forms above are the loader's: ss_fastx_to_flat is the grammar the writer has to agree with
    flat, n = L.fastx_to_flat(text)
    assert flat == b"".join(f + b"\n" for _, f in recs) and n == len(recs)
    src = tmp_path / ("in.txt.gz" if gz else "in.txt")
    src.write_bytes(gzip.compress(text, 6) if gz else text)
    with_bases = [f for _, f in recs if f]
    for which, chosen in (("every third", set(with_bases[::3])), ("all", set(with_bases)), ("none", set()),
                          ("first and last", {with_bases[0], with_bases[-1]})):
        out = tmp_path / "out.txt"
        c = L.extract_write([str(src)], _keys_of(L, sorted(chosen)), [str(out)])
        want = _written_text(recs, chosen)
        assert out.read_bytes() == want, (case, which)
        assert c["read"] == len(recs) and c["written"] == sum(1 for _, f in recs if f and f in chosen), (case, which, c)
        assert c["mate1_only"] == 0 and c["mate2_only"] == 0
        assert not os.path.exists(str(out) + ".tmp")
        out.unlink()


def test_identical_reads_share_a_fate(L, tmp_path):
    text = b"@a\nACGTT\n+\nIIIII\n@b\nGGGGG\n+\nIIIII\n@c\nACGTT\n+\n55555\n"
    (tmp_path / "in.fq").write_bytes(text)
    c = L.extract_write([str(tmp_path / "in.fq")], _keys_of(L, [b"ACGTT"]), [str(tmp_path / "o.fq")])
    assert (tmp_path / "o.fq").read_bytes() == b"@a\nACGTT\n+\nIIIII\n@c\nACGTT\n+\n55555\n" and c["written"] == 2


def test_walker_agrees_with_the_loader_on_damaged_text(L, tmp_path):
    """byte flips, dropped-in markers and cuts: with every digest of the loader's flat block selected, the writer writes exactly
    as many records as that block has records with bases"""
    rs = np.random.RandomState(23)
    seeds = [b"".join(t for t, _ in CASES[c][:6]) for c in ("fastq4", "fastq_multiline", "fasta60", "fastq_crlf", "empty_sequence")]
    src, out = tmp_path / "in.txt", tmp_path / "out.txt"
    for it in range(150):
        t = bytearray(seeds[it % len(seeds)])
        for _ in range(int(rs.randint(1, 4))):
            kind, at = int(rs.randint(0, 4)), int(rs.randint(0, len(t)))
            if kind == 0:
                t[at] = int(rs.randint(0, 256))
            elif kind == 1:
                t.insert(at, b"\n@+>\rN"[int(rs.randint(0, 6))])
            elif kind == 2:
                del t[at:at + int(rs.randint(1, 5))]
            else:
                del t[at:]
            if not t:
                t = bytearray(b"\n")
        flat, _ = L.fastx_to_flat(bytes(t))
        n = sum(1 for p in flat.split(b"\n") if p)
        src.write_bytes(bytes(t))
        c = L.extract_write([str(src)], L.flat_record_keys(flat), [str(out)])
        assert c["written"] == n, (it, bytes(t))
        got = out.read_bytes()
        assert L.fastx_to_flat(got)[0] == b"".join(p + b"\n" for p in flat.split(b"\n") if p), (it, bytes(t))


# ---------------------------------------------------------------------------------------------- pairs


def _pair(n=40, seed=29):
    rs = np.random.RandomState(seed)
    m1, m2 = [], []
    for i in range(n):
        a, b = _rand(rs, 100), _rand(rs, 90)
        m1.append((b"@p%d/1\n%s\n+\n%s\n" % (i, a, _qual(rs, 100)), a))
        m2.append((b"@p%d/2\n%s\n+\n%s\n" % (i, b, _qual(rs, 90)), b))
    return m1, m2


def test_pairs_either_mate(L, tmp_path):
    m1, m2 = _pair()
    p1, p2 = tmp_path / "r1.fq", tmp_path / "r2.fq"
    p1.write_bytes(b"".join(t for t, _ in m1))
    p2.write_bytes(b"".join(t for t, _ in m2))
    only1, only2, both = [2, 11, 39], [0, 5, 17, 30], [7, 8]
    chosen = [m1[i][1] for i in only1 + both] + [m2[i][1] for i in only2 + both]
    o1, o2 = tmp_path / "o1.fq", tmp_path / "o2.fq"
    c = L.extract_write([str(p1), str(p2)], _keys_of(L, chosen), [str(o1), str(o2)])
    keep = sorted(only1 + only2 + both)
    assert o1.read_bytes() == b"".join(m1[i][0] for i in keep)
    assert o2.read_bytes() == b"".join(m2[i][0] for i in keep)
    assert c == dict(read=80, written=2 * len(keep), mate1_only=len(only1), mate2_only=len(only2))
    # each rule on its own
    for sel, want in (([m1[4][1]], dict(read=80, written=2, mate1_only=1, mate2_only=0)),
                      ([m2[4][1]], dict(read=80, written=2, mate1_only=0, mate2_only=1)),
                      ([m1[4][1], m2[4][1]], dict(read=80, written=2, mate1_only=0, mate2_only=0))):
        c = L.extract_write([str(p1), str(p2)], _keys_of(L, sel), [str(o1), str(o2)])
        assert c == want and o1.read_bytes() == m1[4][0] and o2.read_bytes() == m2[4][0]


def test_failures_leave_no_file(L, tmp_path):
    m1, m2 = _pair(12)
    p1, p2 = tmp_path / "r1.fq", tmp_path / "r2.fq"
    p1.write_bytes(b"".join(t for t, _ in m1))
    p2.write_bytes(b"".join(t for t, _ in m2[:-1]))       # one record short
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    o1, o2 = out_dir / "o1.fq", out_dir / "o2.fq"
    keys = _keys_of(L, [m1[0][1], m1[11][1]])
    with pytest.raises(L.SSError) as e:
        L.extract_write([str(p1), str(p2)], keys, [str(o1), str(o2)])
    assert e.value.code == L.SS_EIO
    assert os.listdir(out_dir) == []
    with pytest.raises(L.SSError) as e:                   # an unreadable input
        L.extract_write([str(p1), str(tmp_path / "missing.fq")], keys, [str(o1), str(o2)])
    assert e.value.code == L.SS_EIO and os.listdir(out_dir) == []
    cram = tmp_path / "x.cram"
    cram.write_bytes(b"CRAM\x03\x00" + bytes(64))
    with pytest.raises(L.SSError) as e:
        L.extract_write([str(cram)], keys, [str(o1)])
    assert e.value.code == L.SS_EINVAL and os.listdir(out_dir) == []
    from tests import bamio
    bam = tmp_path / "x.bam"
    bam.write_bytes(bamio.bgzf(bamio.header(), [bamio.record("q", "ACGTACGT")], level=6))
    assert L.input_kind(str(bam)) == "bam"
    with pytest.raises(L.SSError) as e:
        L.extract_write([str(bam)], keys, [str(o1)])
    assert e.value.code == L.SS_EINVAL and os.listdir(out_dir) == []
    with pytest.raises(L.SSError) as e:                   # an output that cannot be made
        L.extract_write([str(p1)], keys, [str(out_dir / "no_such_dir" / "o.fq")])
    assert e.value.code == L.SS_EIO and os.listdir(out_dir) == []


# ---------------------------------------------------------------------------------------------- the base-quality mask


def test_mask_is_part_of_the_flat_form(L, tmp_path):
    """with -q 20 the loader keeps the MASKED bases, so that is the form whose digest finds the record again"""
    text = b"@a\nACGTACGT\n+\nII#IIII+\n@b\nGGGGCCCC\n+\nIIIIIIII\n"
    src, out = tmp_path / "in.fq", tmp_path / "out.fq"
    src.write_bytes(text)
    try:
        L.set_min_base_qual(20)
        assert L.fastx_to_flat(text)[0] == b"ACNTACGN\nGGGGCCCC\n"
        c = L.extract_write([str(src)], _keys_of(L, [b"ACNTACGN"]), [str(out)])
        assert c["written"] == 1 and out.read_bytes() == b"@a\nACGTACGT\n+\nII#IIII+\n"       # (the ORIGINAL text)
        c = L.extract_write([str(src)], _keys_of(L, [b"ACGTACGT"]), [str(out)])
        assert c["written"] == 0 and out.read_bytes() == b""
    finally:
        L.set_min_base_qual(0)
    c = L.extract_write([str(src)], _keys_of(L, [b"ACGTACGT"]), [str(out)])
    assert c["written"] == 1


# ---------------------------------------------------------------------------------------------- the flag


def _parsers():
    from strainscan_amd import StrainScan
    out = []
    for multi in (False, True):
        ap = argparse.ArgumentParser(prog="x")
        StrainScan.add_arguments(ap, multi=multi)
        out.append(ap)
    return out


def test_flag_parsing(capsys):
    for ap in _parsers():
        base = ["-i", "r.fq", "-d", "DB"]
        assert ap.parse_args(base).extract_reads == 0                       # absent by default
        assert ap.parse_args(base + ["-x", "16"]).extract_reads == 16
        assert ap.parse_args(base + ["--extract_reads", "1"]).extract_reads == 1
        for bad in ("0", "-3", "abc", "1.5", ""):
            with pytest.raises(SystemExit) as e:
                ap.parse_args(base + ["-x", bad])
            assert e.value.code == 2, bad
    capsys.readouterr()


def test_commands_refuse_a_bad_value_before_any_input_is_opened(tmp_path):
    import sys
    for mod in ("strainscan_amd.StrainScan", "strainscan_amd.multi_db"):
        for bad in ("0", "-3", "abc"):
            r = subprocess.run([sys.executable, "-m", mod, "-i", str(tmp_path / "no_such.fq"), "-d", str(tmp_path / "no_db"), "-o",
                                str(tmp_path / "out"), "-x", bad], capture_output=True, text=True, cwd=ROOT, timeout=300)
            assert r.returncode == 2 and "-x" in r.stderr, (mod, bad, r.stderr[-500:])
            assert not (tmp_path / "out").exists()


def test_set_extract_reads_and_the_idle_collector(tmp_path):
    import strainscan_amd
    from strainscan_amd import read_reports
    assert read_reports.EXTRACT_READS["n"] == 0                                       # off by default
    read_reports.collect_extract_reads("tree", None, [str(tmp_path / "no_such.fq")])  # off: nothing is looked at
    try:
        strainscan_amd.set_extract_reads(16, str(tmp_path))
        assert read_reports.EXTRACT_READS["n"] == 16 and read_reports.EXTRACT_READS["dir"] == str(tmp_path) and read_reports.EXTRACT_READS["skipped"] is None
        for bad in (-1, 1.5, "3", True):
            with pytest.raises(ValueError):
                strainscan_amd.set_extract_reads(bad)
        assert read_reports.EXTRACT_READS["n"] == 16
    finally:
        strainscan_amd.set_extract_reads(0)
    assert read_reports.EXTRACT_READS["n"] == 0 and read_reports.EXTRACT_READS["dir"] is None
    read_reports.collect_extract_reads("tree", None, [str(tmp_path / "no_such.fq")])
    assert os.listdir(tmp_path) == []


def test_record_type(tmp_path):
    from strainscan_amd import read_reports
    (tmp_path / "a").write_bytes(b"\n>s\nACGT\n")
    (tmp_path / "b").write_bytes(b"@r\nACGT\n+\nIIII\n")
    (tmp_path / "c.gz").write_bytes(gzip.compress(b">s\nACGT\n"))
    (tmp_path / "d.gz").write_bytes(gzip.compress(b"@r\nACGT\n+\nIIII\n"))
    assert [read_reports.fastx_record_type(str(tmp_path / n)) for n in ("a", "b", "c.gz", "d.gz")] == ["fasta", "fastq", "fasta", "fastq"]


# ---------------------------------------------------------------------------------------------- the walker under sanitizers


def test_record_walker_fuzz_sanitized(tmp_path):
    """tests/extract_fuzz.cpp, a stand-alone program (host code, g++) under AddressSanitizer + UBSan: a few thousand damaged
    FASTQ / FASTA texts walked record by record and written with every digest selected, without a single bad access."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "extract_fuzz"
    r = subprocess.run(["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "extract_fuzz.cpp"), "-o", str(exe), "-lz"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(tmp_path), "2000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "extract_fuzz ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
