"""--pairs on the host: the fragment-aware writer (ss_extract_write_pairs) against a Python filter of the same pairs, named by the
digest of the joined record (tests/pairs_model.py); its failures leaving nothing behind; the flag's handling; the new symbols.
What the device joins is tests/test_pairs_gpu.py's."""
import argparse
import ctypes
import gzip
import os
import re

import numpy as np
import pytest

from tests import pairs_model as pm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    return _lib


def _rand(rs, n):
    return np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, size=n)].tobytes()


def _qual(rs, n, low=False):
    return np.frombuffer(b"#+05678ABCDEFGHIJ" if low else b"5678ABCDEFGHIJ", np.uint8)[rs.randint(0, 17 if low else 14, size=n)].tobytes()


def _wrap(s, w, eol=b"\n"):
    return b"".join(s[i:i + w] + eol for i in range(0, len(s), w))


def _record(fmt, name, s, rs, low=False):
    if fmt == "fastq":
        return b"@%s\n%s\n+\n%s\n" % (name, s, _qual(rs, len(s), low))
    if fmt == "fastq_wrapped":
        return b"@%s\n" % name + (_wrap(s, 50) or b"\n") + b"+\n" + (_wrap(_qual(rs, len(s), low), 50) or b"\n")
    if fmt == "fasta":
        return b">%s\n%s\n" % (name, s) if s else b">%s\n" % name
    if fmt == "fasta_wrapped":
        return b">%s\n" % name + _wrap(s, 60)
    if fmt == "fastq_crlf":
        return b"@%s\r\n%s\r\n+\r\n%s\r\n" % (name, s, _qual(rs, len(s), low))
    raise ValueError(fmt)


def _pair_seqs(seed):
    """the mates of 64 pairs: random ones, a pair with an empty mate 1, one with an empty mate 2, one with both empty, a pair that
    stands three times, pairs that differ in mate 2 only, and the two pairs that join to the same bytes (AN + C, A + NC)"""
    rs = np.random.RandomState(seed)
    pairs = [(_rand(rs, int(rs.randint(1, 200))), _rand(rs, int(rs.randint(1, 200)))) for _ in range(52)]
    pairs.insert(5, (b"", _rand(rs, 80)))
    pairs.insert(11, (_rand(rs, 90), b""))
    pairs.insert(17, (b"", b""))
    twin = (_rand(rs, 100), _rand(rs, 100))
    for at in (2, 23, 40):
        pairs.insert(at, twin)
    m1 = _rand(rs, 120)
    pairs.insert(30, (m1, _rand(rs, 120)))
    pairs.insert(31, (m1, _rand(rs, 120)))
    pairs.insert(50, (m1, _rand(rs, 119)))
    pairs.insert(8, (b"AN", b"C"))
    pairs.insert(44, (b"A", b"NC"))
    pairs.append((_rand(rs, 150), _rand(rs, 150)))
    assert len(pairs) == 64
    return pairs


FORMATS = {"fastq": ("fastq", "fastq"), "fasta": ("fasta", "fasta"), "fasta_wrapped": ("fasta_wrapped", "fasta_wrapped"),
           "crlf": ("fastq_crlf", "fastq_crlf"), "wrapped_fastq_and_fasta": ("fastq_wrapped", "fasta")}


def _sample(L, fmts, seed, low=False):
    """-> (texts of file 1, texts of file 2, flats of file 1, flats of file 2): record by record; the flat forms are the loader's
    (ss_fastx_to_flat on the whole file, under whatever base-quality mask is set)"""
    rs = np.random.RandomState(seed)
    texts = ([], [])
    for i, mates in enumerate(_pair_seqs(seed)):
        for m in range(2):
            texts[m].append(_record(fmts[m], b"p%d/%d" % (i, m + 1), mates[m], rs, low))
    flats = []
    for m in range(2):
        flat, n = L.fastx_to_flat(b"".join(texts[m]))
        assert n == len(texts[m])
        flats.append(pm.lines_of(flat))
        assert len(flats[m]) == n
    return texts[0], texts[1], flats[0], flats[1]


def _check_writer(L, tmp_path, t1, t2, f1, f2, gz):
    ext = ".gz" if gz else ""
    srcs = [tmp_path / ("in_1.txt" + ext), tmp_path / ("in_2.txt" + ext)]
    for p, t in zip(srcs, (t1, t2)):
        p.write_bytes(gzip.compress(b"".join(t), 6) if gz else b"".join(t))
    joined = pm.join_lines(f1, f2)
    keys = pm.pair_digests(L, f1, f2)
    assert keys.shape == (len(joined), 2)
    # (equal joined records, and only they, share a digest)
    assert len({tuple(k) for k in keys.tolist()}) == len(set(joined))
    n = len(joined)
    outs = [tmp_path / "out_1.txt", tmp_path / "out_2.txt"]
    bare = [(not a.strip(), not b.strip()) for a, b in zip(f1, f2)]          # (a CRLF file's empty line is a lone '\r')
    for which, idx in (("all", range(n)), ("none", []), ("every third", range(0, n, 3)), ("an empty mate 1", [bare.index((True, False))]),
                       ("an empty mate 2", [bare.index((False, True))]), ("both empty", [bare.index((True, True))]), ("first and last", [0, n - 1])):
        idx = list(idx)
        chosen = {joined[i] for i in idx}
        want = [i for i in range(n) if joined[i] in chosen]
        c = L.extract_write_pairs([str(p) for p in srcs], keys[idx] if idx else np.zeros((0, 2), np.uint64), [str(o) for o in outs])
        assert outs[0].read_bytes() == b"".join(t1[i] for i in want), which
        assert outs[1].read_bytes() == b"".join(t2[i] for i in want), which
        assert c == dict(read=2 * n, written=2 * len(want), pairs=len(want)), (which, c)
        assert sorted(os.listdir(tmp_path)) == sorted(p.name for p in srcs + outs)
        for o in outs:
            o.unlink()
    return joined


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
@pytest.mark.parametrize("case", sorted(FORMATS))
def test_writer_equals_filter(L, tmp_path, case, gz):
    t1, t2, f1, f2 = _sample(L, FORMATS[case], 31)
    joined = _check_writer(L, tmp_path, t1, t2, f1, f2, gz)
    if case != "crlf":
        # the shapes the docstring of _pair_seqs promises, found again in the loader's flat forms
        assert joined.count(b"N") == 1 and joined.count(b"ANNC") == 2 and max(joined.count(r) for r in joined) == 3
        assert any(f1[i] == f1[j] and f2[i] != f2[j] and len(f1[i]) == 120 for i in range(len(f1)) for j in range(i))


def test_writer_under_the_quality_mask(L, tmp_path):
    plain = _sample(L, FORMATS["fastq"], 32, low=True)
    L.set_min_base_qual(20)
    try:
        t1, t2, f1, f2 = _sample(L, FORMATS["fastq"], 32, low=True)
        assert (t1, t2) == plain[:2] and f1 != plain[2] and sum(r.count(b"N") for r in f1) > 100
        _check_writer(L, tmp_path, t1, t2, f1, f2, False)
        # the unmasked digests name nothing but the pairs the mask left alone
        keys = pm.pair_digests(L, plain[2], plain[3])
        srcs = [str(tmp_path / "in_1.txt"), str(tmp_path / "in_2.txt")]
        c = L.extract_write_pairs(srcs, keys, [str(tmp_path / "o1"), str(tmp_path / "o2")])
        same = set(pm.join_lines(f1, f2)) & set(pm.join_lines(plain[2], plain[3]))
        assert c["pairs"] == sum(1 for r in pm.join_lines(f1, f2) if r in same) < len(f1)
    finally:
        L.set_min_base_qual(0)


def test_failures_leave_nothing(L, tmp_path):
    t1, t2, f1, f2 = _sample(L, FORMATS["fastq"], 33)
    a, b, short = tmp_path / "a.fq", tmp_path / "b.fq", tmp_path / "short.fq"
    a.write_bytes(b"".join(t1))
    b.write_bytes(b"".join(t2))
    short.write_bytes(b"".join(t2[:-1]))
    bam = tmp_path / "x.bam"
    bam.write_bytes(b"BAM\1" + b"\0" * 60)
    keys = pm.pair_digests(L, f1, f2)
    before = sorted(os.listdir(tmp_path))
    fn = L.lib().ss_extract_write_pairs

    def call(ins, outs, n_in=2):
        c = (ctypes.c_uint64 * 4)()
        return fn((ctypes.c_char_p * len(ins))(*[os.fsencode(str(p)) for p in ins]), n_in, L.ptr(keys), keys.shape[0],
                  (ctypes.c_char_p * len(outs))(*[os.fsencode(str(p)) for p in outs]), c)

    outs = [tmp_path / "o1.fq", tmp_path / "o2.fq"]
    assert call([a, short], outs) == L.SS_EIO                      # unequal record counts (every pair before the end was selected)
    assert call([short, b], outs) == L.SS_EIO
    assert call([a, tmp_path / "missing.fq"], outs) == L.SS_EIO
    assert call([a, bam], outs) == L.SS_EINVAL and call([bam, b], outs) == L.SS_EINVAL
    assert call([a], outs[:1], n_in=1) == L.SS_EINVAL              # exactly two
    assert call([a, b], [outs[0], tmp_path / "no such dir" / "o2.fq"]) == L.SS_EIO
    assert sorted(os.listdir(tmp_path)) == before
    with pytest.raises(ValueError):
        L.extract_write_pairs([str(a)], keys, [str(outs[0])])
    assert call([a, b], outs) == L.SS_OK and outs[0].read_bytes() == a.read_bytes() and outs[1].read_bytes() == b.read_bytes()


def test_joined_flat_digests_are_the_writers(L, tmp_path):
    """ss_flat_record_keys over the Python-joined flat block (what the joined set reads back as) names exactly the pairs: each
    digest alone writes its pair and the pairs equal to it"""
    t1, t2, f1, f2 = _sample(L, FORMATS["wrapped_fastq_and_fasta"], 34)
    srcs = [tmp_path / "in_1.txt", tmp_path / "in_2.txt"]
    srcs[0].write_bytes(b"".join(t1))
    srcs[1].write_bytes(b"".join(t2))
    flat1, flat2 = (L.fastx_to_flat(p.read_bytes())[0] for p in srcs)
    keys = L.flat_record_keys(pm.join_flat(flat1, flat2))
    assert (keys == pm.pair_digests(L, f1, f2)).all() and keys.shape[0] == len(t1)
    joined = pm.join_lines(f1, f2)
    outs = [str(tmp_path / "o1"), str(tmp_path / "o2")]
    for i in range(len(joined)):
        c = L.extract_write_pairs([str(p) for p in srcs], keys[i:i + 1], outs)
        want = [j for j in range(len(joined)) if joined[j] == joined[i]]
        assert c["pairs"] == len(want) and open(outs[0], "rb").read() == b"".join(t1[j] for j in want), i
        assert open(outs[1], "rb").read() == b"".join(t2[j] for j in want), i


def test_pair_writer_fuzz_sanitized(tmp_path):
    """tests/pairs_fuzz.cpp, a stand-alone program (host code, g++) under AddressSanitizer + UBSan: a few thousand pairs of damaged
    texts through ss_extract_write_pairs -- unequal record counts leave nothing, equal ones are written record for record (an
    empty FASTQ record with its empty quality line), one digest writes the pairs that join to its bytes"""
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "pairs_fuzz"
    r = subprocess.run(["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "pairs_fuzz.cpp"), "-o", str(exe), "-lz"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    (tmp_path / "scratch").mkdir()
    r = subprocess.run([str(exe), str(tmp_path / "scratch"), "3000"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "pairs_fuzz ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    m = re.search(r"(\d+) pairs of texts written, (\d+) with unequal record counts", r.stdout)
    assert int(m.group(1)) > 500 and int(m.group(2)) > 500


def test_an_empty_fastq_record_keeps_its_quality_line(L, tmp_path):
    """a record without bases is `@name, empty line, +, empty line`: all four lines are written, also in CRLF text (whose empty
    line is a lone '\\r', so the record has a base as far as the loader goes) and where the quality line is missing"""
    t1 = [b"@a\nACGT\n+\nIIII\n", b"@e1\n\n+\n\n", b"@e2\r\n\r\n+\r\n\r\n", b"@e3\n\n+\n", b"@z\nA\n+\nI\n"]
    t2 = [b"@a\nAC\n+\nII\n", b"@f1\nGG\n+\nII\n", b"@f2\nTT\n+\nII\n", b"@f3\nCC\n+\nII\n", b"@z\n\n+\n\n"]
    (tmp_path / "r1.fq").write_bytes(b"".join(t1))
    (tmp_path / "r2.fq").write_bytes(b"".join(t2))
    f1, f2 = (pm.lines_of(L.fastx_to_flat(b"".join(t))[0]) for t in (t1, t2))
    assert f1 == [b"ACGT", b"", b"\r", b"", b"A"] and f2 == [b"AC", b"GG", b"TT", b"CC", b""]
    outs = [str(tmp_path / "o1.fq"), str(tmp_path / "o2.fq")]
    c = L.extract_write_pairs([str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq")], pm.pair_digests(L, f1, f2), outs)
    assert c == dict(read=10, written=10, pairs=5)
    assert open(outs[0], "rb").read() == b"".join(t1) and open(outs[1], "rb").read() == b"".join(t2)


# ---------------------------------------------------------------------------------------------- the flag


def test_the_command_line_refuses_pairs_alone(tmp_path, capsys):
    from strainscan_amd import StrainScan, multi_db, read_reports as rr
    out = tmp_path / "out"
    db = tmp_path / "DB"
    (db / "Tree_database").mkdir(parents=True)
    base = ["-i", str(tmp_path / "r1.fq"), "-d", str(db), "-o", str(out)]
    try:
        for main in (StrainScan.main, multi_db.main):
            for argv, word in ((base + ["--pairs", "--read_support"], "-j"),
                               (base + ["--pairs", "-j", str(tmp_path / "r2.fq")], "--read_support"),
                               (base + ["--pairs", "-j", str(tmp_path / "r2.fq"), "--by_strain"], "--read_support")):
                with pytest.raises(SystemExit) as e:
                    main(argv)
                assert e.value.code == 2
                assert word in capsys.readouterr().err
                assert not out.exists() and not rr.PAIRS["on"]
    finally:
        rr.reset_all()
    for multi in (False, True):
        ap = argparse.ArgumentParser(prog="x")
        StrainScan.add_arguments(ap, multi=multi)
        a = ap.parse_args(["-i", "a", "-d", "D"])
        assert a.pairs is False
        StrainScan.refuse_pairs_alone(ap, a)
        for report in (["--read_support"], ["-x", "3"], ["--bootstrap", "5"], ["--classify_reads", "2"]):
            a = ap.parse_args(["-i", "a", "-j", "b", "-d", "D", "--pairs"] + report)
            assert a.pairs is True
            StrainScan.refuse_pairs_alone(ap, a)


def test_set_pairs_and_reset_all():
    import strainscan_amd
    from strainscan_amd import StrainScan, read_reports as rr
    rr.reset_all()
    try:
        assert rr.PAIRS == {"on": False, "skipped": None}
        strainscan_amd.set_pairs(True)
        assert rr.PAIRS["on"] is True
        strainscan_amd.set_pairs(0)
        assert rr.PAIRS["on"] is False
        StrainScan.apply_pairs(True)
        rr.PAIRS["skipped"] = "why"
        rr.reset_all()
        assert rr.PAIRS == {"on": False, "skipped": None}
    finally:
        rr.reset_all()


def test_the_gate_says_one_line_and_silences_every_report(tmp_path, capsys):
    """where the pairs cannot be joined (here: one file) the hooks say one line, once, and collect nothing"""
    import types
    from strainscan_amd import read_reports as rr
    rr.reset_all()
    try:
        rr.pairs_reset(True)
        rr.read_support_reset(True)
        rr.extract_reads_reset(2, str(tmp_path))
        rr.bootstrap_reset(5)
        rr.classify_reads_reset(1)
        rr.extract_class_reset(["unclassified", "called"])
        for _ in range(2):
            rr.tree_scanned(types.SimpleNamespace(is_external=True), ["no such file"])
            rr.table_scanned("C1", object(), ["no such file"])
            rr.cluster_reported("C1", "no such dir", "no such report", 31, ["no such file"])
            rr.collect_called_classes([1], "no such dir", True, ["no such file"])
        err = capsys.readouterr().err.split("\n")
        assert len(err) == 2 and err[0].startswith("pairs: ") and err[0].endswith(" and no per-read report was written") and err[1] == ""
        rr.write_all(str(tmp_path))
        assert os.listdir(tmp_path) == []
        # off: the hooks look at nothing and say nothing
        rr.reset_all()
        rr.tree_scanned(types.SimpleNamespace(is_external=True), ["no such file"])
        rr.table_scanned("C1", object(), ["no such file"])
        assert capsys.readouterr().err == ""
    finally:
        rr.reset_all()


def test_header_and_library_carry_the_symbols():
    from strainscan_amd import _lib
    hdr = open(os.path.join(REPO, "include", "strainscan_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ("ss_reads_join_pairs_dev", "ss_reads_join_pairs_calls", "ss_reads_load_pairs", "ss_extract_write_pairs"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert hasattr(lib, sym) and sym in _lib.SIGNATURES, sym
    for name in ("join_pairs_dev", "load_pairs"):
        assert hasattr(_lib.ReadSet, name)
    assert callable(_lib.extract_write_pairs) and callable(_lib.join_pairs_calls)
