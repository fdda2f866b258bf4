"""The host half of --read_calls, which needs no device: the writer (ss_read_calls_write) against the text of
tests/read_calls_model.py, its failures leaving nothing behind, the flag's refusals, the symbols, the conditions that keep the
device test (tests/test_read_calls_gpu.py) from passing vacuously, and the writer under AddressSanitizer + UBSan as a stand-alone
program (tests/read_calls_fuzz.cpp)."""
import argparse
import gzip
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import class_cases as cc, class_model as cm, read_calls_cases as rcc, read_calls_model as rcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_VALUE = np.array([-1, 7, 12, 300, 5000000000], np.int64)      # nodes 1..4 (an id beyond 32 bits among them)


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    return _lib


def _rand(rs, n):
    return np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, size=n)].tobytes()


def _qual(rs, n):
    return np.frombuffer(b"5678ABCDEFGHIJ", np.uint8)[rs.randint(0, 14, size=n)].tobytes()


def _wrap(s, w, eol):
    return b"".join(s[i:i + w] + eol for i in range(0, len(s), w))


def _texts():
    """name -> (text, records with a sequence, records)"""
    rs = np.random.RandomState(31)
    out = {}
    t = []
    for i in range(40):
        s = _rand(rs, int(rs.randint(1, 200)))
        q = _qual(rs, len(s))
        if i == 7:
            q = b"@" + q[1:]                         # a quality line that begins like a header
        name = {3: b"@with space and more", 4: b"@with\ttab", 5: b"@", 6: b"@ blank first"}.get(i, b"@r%d/1" % i)
        t.append(name + b"\n" + s + b"\n+\n" + q + b"\n")
    out["fastq4"] = (b"".join(t), 40, 40)
    t = []
    for i in range(30):
        s = _rand(rs, int(rs.randint(1, 400)))
        t.append(b"@m%d x\n" % i + _wrap(s, 50, b"\n") + b"+m%d\n" % i + _wrap(_qual(rs, len(s)), 50, b"\n"))
    out["fastq_wrapped"] = (b"".join(t), 30, 30)
    out["fasta_wrapped"] = (b"".join(b">s%d wrapped at 60\n" % i + _wrap(_rand(rs, int(rs.randint(1, 500))), 60, b"\n") for i in range(30)), 30, 30)
    t = []
    for i in range(24):
        s = _rand(rs, int(rs.randint(1, 200)))
        t.append(b"@c%d crlf\r\n%s\r\n+\r\n%s\r\n" % (i, s, _qual(rs, len(s))))
    out["fastq_crlf"] = (b"".join(t), 24, 24)
    out["fasta_crlf"] = (b"".join(b">c%d\r\n" % i + _wrap(_rand(rs, int(rs.randint(61, 200))), 60, b"\r\n") for i in range(20)), 20, 20)
    body = [b"@r%d\n%s\n+\n%s\n" % (i, s, _qual(rs, len(s))) for i, s in enumerate(_rand(rs, int(rs.randint(1, 99))) for _ in range(12))]
    empty = lambda n: b"@%s\n\n+\n\n" % n      # noqa: E731
    out["empty_first_middle_last"] = (empty(b"e0") + b"".join(body[:6]) + empty(b"e1 mid") + b"".join(body[6:]) + empty(b"e2"), 12, 15)
    out["fasta_empty"] = (b">a\n\n>b\nACGT\n>c\n>d\nAC\nGT\n>e\n", 2, 5)
    out["no_records"] = (b"", 0, 0)
    out["only_stray_lines"] = (b"\n\nstray\n\n", 0, 0)
    out["no_final_newline"] = (b"".join(body[:4])[:-1], 4, 4)
    return out


TEXTS = _texts()


def _random_calls(n, seed, n_nodes=4):
    rs = np.random.RandomState(seed)
    lists = []
    for i in range(n):
        k = int(rs.randint(0, n_nodes + 1)) if i % 5 else 0
        lists.append(sorted((int(v), int(rs.randint(1, 1 << 20))) for v in rs.choice(np.arange(1, n_nodes + 1), k, replace=False)))
    first = np.zeros(n + 1, np.uint64)
    first[1:] = np.cumsum([len(x) for x in lists])
    flat = [e for x in lists for e in x]
    return dict(classes=rs.randint(0, n_nodes + 1, size=n).astype(np.uint32), scores=rs.randint(0, 1 << 31, size=n).astype(np.uint32),
                first=first, list_node=np.array([v for v, _ in flat], np.uint32), list_hits=np.array([c for _, c in flat], np.uint32))


# ---------------------------------------------------------------------------------------------- the model's own walk


def test_the_models_walk_is_the_loaders(L):
    """the records the model's walk finds are those of ss_fastx_to_flat, sequence for sequence"""
    for name, (text, with_seq, records) in TEXTS.items():
        recs = rcm.walk_records(text)
        flat, n = L.fastx_to_flat(text)
        assert len(recs) == records == n, name
        assert flat == b"".join(f + b"\n" for _, f, _ in recs), name
        assert sum(1 for _, f, _ in recs if f) == with_seq, name
    names = [n for n, _, _ in rcm.walk_records(TEXTS["fastq4"][0])]
    assert names[3:8] == [b"with", b"with", b"", b"", b"r7/1"]
    assert [(n, ln) for n, _, ln in rcm.walk_records(TEXTS["fastq_crlf"][0])][0][0] == b"c0"
    assert all(b"\r" in f and ln == len(f) - f.count(b"\r") for _, f, ln in rcm.walk_records(TEXTS["fasta_crlf"][0]))


def test_hand_written_table(L, tmp_path):
    text = b"@r1 x\nACGT\n+\nIIII\n@\n\n+\n\n@r3\tz\r\nAC\r\n+\r\nII\r\n"
    calls = dict(classes=np.array([2, 0], np.uint32), scores=np.array([5, 1], np.uint32), first=np.array([0, 2, 3], np.uint64),
                 list_node=np.array([1, 4, 1], np.uint32), list_hits=np.array([3, 70000, 1], np.uint32))
    want = b"name\tnode\tscore\tlength\thits\nr1\t12\t5\t4\t7:3 5000000000:70000\n\t-1\t0\t0\t-\nr3\t-1\t1\t2\t7:1\n"
    assert rcm.table_text([text], calls, NODE_VALUE) == [want]
    (tmp_path / "a.fq").write_bytes(text)
    c = L.read_calls_write([str(tmp_path / "a.fq")], [str(tmp_path / "o.tsv")], calls, NODE_VALUE)
    assert (tmp_path / "o.tsv").read_bytes() == want
    assert c == dict(read=3, written=3, classified=1, empty=1)


# ---------------------------------------------------------------------------------------------- the writer


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
@pytest.mark.parametrize("case", sorted(TEXTS))
def test_writer_equals_the_model(L, tmp_path, case, gz):
    text, with_seq, records = TEXTS[case]
    src = tmp_path / ("in.txt.gz" if gz else "in.txt")
    src.write_bytes(gzip.compress(text, 6) if gz else text)
    out = tmp_path / "calls.tsv"
    for seed in (1, 2):
        calls = _random_calls(with_seq, seed)
        c = L.read_calls_write([str(src)], [str(out)], calls, NODE_VALUE)
        want, = rcm.table_text([text], calls, NODE_VALUE)
        assert out.read_bytes() == want, case
        assert want.count(b"\n") == records + 1
        assert c == dict(read=records, written=records, classified=int((calls["classes"] != 0).sum()), empty=records - with_seq), (case, c)
        assert sorted(os.listdir(tmp_path)) == sorted([src.name, "calls.tsv"])
        out.unlink()


def test_a_file_of_several_chunks_on_several_threads(L, tmp_path, monkeypatch):
    """20 MB of four-line FASTQ: three chunks of the loader's chunk rule, walked by 1, 3 and 16 threads -- the same bytes, the
    model's; records without a sequence in every chunk"""
    rs = np.random.RandomState(43)
    seq = _rand(rs, 70000 * 150)
    recs = []
    for i in range(70000):
        s = b"" if i % 997 == 5 else seq[150 * i:150 * i + 150 - i % 3]
        recs.append(b"@read%d/1 len=%d\n%s\n+\n%s\n" % (i, len(s), s, b"I" * len(s)))
    text = b"".join(recs)
    assert len(text) > (16 << 20)
    with_seq = 70000 - len(range(5, 70000, 997))
    src, out = tmp_path / "big.fq", tmp_path / "calls.tsv"
    src.write_bytes(text)
    calls = _random_calls(with_seq, 7)
    want, = rcm.table_text([text], calls, NODE_VALUE)
    for threads in ("1", "3", "16"):
        monkeypatch.setenv("SS_HOST_THREADS", threads)
        c = L.read_calls_write([str(src)], [str(out)], calls, NODE_VALUE)
        assert out.read_bytes() == want, threads
        assert c == dict(read=70000, written=70000, classified=int((calls["classes"] != 0).sum()), empty=70000 - with_seq)
        out.unlink()
    for n in (with_seq - 1, with_seq + 1):
        with pytest.raises(L.SSError) as e:
            L.read_calls_write([str(src)], [str(out)], _random_calls(n, 7), NODE_VALUE)
        assert e.value.code == L.SS_EIO and sorted(os.listdir(tmp_path)) == ["big.fq"]


def test_record_count_mismatch_leaves_nothing(L, tmp_path):
    text, with_seq, _ = TEXTS["empty_first_middle_last"]
    src = tmp_path / "in.fq"
    src.write_bytes(text)
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    for n in (with_seq - 1, with_seq + 1):
        with pytest.raises(L.SSError) as e:
            L.read_calls_write([str(src)], [str(out_dir / "calls.tsv")], _random_calls(n, 3), NODE_VALUE)
        assert e.value.code == L.SS_EIO and os.listdir(out_dir) == [], n
    with pytest.raises(L.SSError) as e:                   # an output that cannot be made
        L.read_calls_write([str(src)], [str(out_dir / "no_such_dir" / "calls.tsv")], _random_calls(with_seq, 3), NODE_VALUE)
    assert e.value.code == L.SS_EIO and os.listdir(out_dir) == []
    with pytest.raises(L.SSError) as e:                   # an unreadable input
        L.read_calls_write([str(tmp_path / "missing.fq")], [str(out_dir / "calls.tsv")], _random_calls(with_seq, 3), NODE_VALUE)
    assert e.value.code == L.SS_EIO and os.listdir(out_dir) == []
    from tests import bamio
    bam = tmp_path / "x.bam"
    bam.write_bytes(bamio.bgzf(bamio.header(), [bamio.record("q", "ACGTACGT")], level=6))
    with pytest.raises(L.SSError) as e:
        L.read_calls_write([str(bam)], [str(out_dir / "calls.tsv")], _random_calls(1, 3), NODE_VALUE)
    assert e.value.code == L.SS_EINVAL and os.listdir(out_dir) == []
    # arrays that contradict themselves are refused before any file is made
    good = _random_calls(with_seq, 3)
    for key, at, value in (("first", 2, 10 ** 9), ("classes", 0, 5), ("list_node", 0, 0), ("list_node", 0, 5)):
        bad = {k: v.copy() for k, v in good.items()}
        bad[key][at] = value
        with pytest.raises(L.SSError) as e:
            L.read_calls_write([str(src)], [str(out_dir / "calls.tsv")], bad, NODE_VALUE)
        assert e.value.code == L.SS_EINVAL and os.listdir(out_dir) == [], (key, at)


def test_two_files_of_a_joined_set(L, tmp_path):
    """record j of both files takes entry j: an empty mate is a record like any other, with its own length 0"""
    rs = np.random.RandomState(37)
    m1, m2 = [], []
    for i in range(25):
        a, b = _rand(rs, 100), _rand(rs, 90)
        if i == 4:
            a = b""
        if i == 24:
            b = b""
        m1.append(b"@p%d/1 a\n%s\n+\n%s\n" % (i, a, _qual(rs, len(a))))
        m2.append(b"@p%d/2 b\n%s\n+\n%s\n" % (i, b, _qual(rs, len(b))))
    t1, t2 = b"".join(m1), b"".join(m2)
    (tmp_path / "r1.fq").write_bytes(t1)
    (tmp_path / "r2.fq").write_bytes(t2)
    ins = [str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq")]
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    outs = [str(out_dir / "c1.tsv"), str(out_dir / "c2.tsv")]
    calls = _random_calls(25, 5)
    c = L.read_calls_write(ins, outs, calls, NODE_VALUE)
    want = rcm.table_text([t1, t2], calls, NODE_VALUE)
    got = [open(o, "rb").read() for o in outs]
    assert got == want
    assert c == dict(read=50, written=50, classified=2 * int((calls["classes"] != 0).sum()), empty=2)
    rows = [[ln.split(b"\t") for ln in g.split(b"\n")[1:-1]] for g in got]
    assert all(a[1:3] + a[4:] == b[1:3] + b[4:] for a, b in zip(*rows))      # the mates share node, score and hits
    assert rows[0][4][3] == b"0" and rows[1][4][3] == b"90" and rows[1][24][3] == b"0"
    for o in outs:
        os.unlink(o)
    for n in (24, 26):                                    # the set has a fragment fewer, one more
        with pytest.raises(L.SSError) as e:
            L.read_calls_write(ins, outs, _random_calls(n, 5), NODE_VALUE)
        assert e.value.code == L.SS_EIO and os.listdir(out_dir) == []
    (tmp_path / "r2.fq").write_bytes(b"".join(m2[:-1]))   # the files differ in records
    with pytest.raises(L.SSError) as e:
        L.read_calls_write(ins, outs, _random_calls(25, 5), NODE_VALUE)
    assert e.value.code == L.SS_EIO and os.listdir(out_dir) == []


# ---------------------------------------------------------------------------------------------- the flag


def test_flag_parsing_and_state(tmp_path, capsys):
    import strainscan_amd
    from strainscan_amd import StrainScan, read_reports as rr
    for multi in (False, True):
        ap = argparse.ArgumentParser(prog="x")
        StrainScan.add_arguments(ap, multi=multi)
        base = ["-i", "r.fq", "-d", "DB"]
        assert ap.parse_args(base).read_calls is False
        args = ap.parse_args(base + ["--read_calls"])
        assert args.read_calls is True
        with pytest.raises(SystemExit) as e:
            StrainScan.refuse_read_calls_alone(ap, args)
        assert e.value.code == 2
        StrainScan.refuse_read_calls_alone(ap, ap.parse_args(base + ["--read_calls", "--classify_reads", "2"]))      # (r.fq: no BAM)
    assert "--classify_reads" in capsys.readouterr().err
    assert rr.READ_CALLS["on"] is False
    try:
        strainscan_amd.set_read_calls(True, str(tmp_path))
        assert rr.READ_CALLS == dict(on=True, dir=str(tmp_path), skipped=None, files=[])
        with rr.database_scope("lab", "elsewhere"):
            assert rr.READ_CALLS["dir"] == "elsewhere"
        assert rr.READ_CALLS["dir"] == str(tmp_path)
    finally:
        rr.reset_all()
    assert rr.READ_CALLS == dict(on=False, dir=None, skipped=None, files=[])
    rr._write_read_calls(None, None, None, 1, [], [str(tmp_path / "no_such.fq")])      # off: nothing is looked at
    assert os.listdir(tmp_path) == []


def test_commands_refuse_before_any_input_is_opened(tmp_path):
    from tests import bamio
    bam = tmp_path / "x.bam"
    bam.write_bytes(bamio.bgzf(bamio.header(), [bamio.record("q", "ACGTACGT")], level=6))
    for mod in ("strainscan_amd.StrainScan", "strainscan_amd.multi_db"):
        common = [sys.executable, "-m", mod, "-d", str(tmp_path / "no_db"), "-o", str(tmp_path / "out")]
        r = subprocess.run(common + ["-i", str(tmp_path / "no_such.fq"), "--read_calls"], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 2 and "--read_calls needs --classify_reads" in r.stderr, (mod, r.stderr[-500:])
        r = subprocess.run(common + ["-i", str(bam), "--read_calls", "--classify_reads", "1"], capture_output=True, text=True, cwd=ROOT,
                           timeout=300)
        assert r.returncode == 2 and "--tag_bam" in r.stderr and "x.bam" in r.stderr, (mod, r.stderr[-500:])
        assert not (tmp_path / "out").exists()


def test_the_symbols_are_declared():
    hdr = open(os.path.join(ROOT, "include", "strainscan_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from strainscan_amd import _lib
    for name in ("ss_reads_calls", "ss_reads_calls_calls", "ss_reads_load_ordered", "ss_read_calls_write"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
    assert "ss_calls.hip" in open(os.path.join(ROOT, "strainscan_amd", "csrc", "Makefile")).read()


# ---------------------------------------------------------------------------------------------- the device test's inputs


@pytest.fixture(scope="module")
def modelled():
    """table -> [(record bytes, calls at M = 3 of its block: class, score, tie, list)] over every block of the device test"""
    g = cc.source()
    par = cc.parents()
    out = {}
    for tname in cc.TABLES:
        k, _, keys, row_node = cc.table(tname, g)
        rows = []
        for block in rcc.blocks(g).values():
            per, _ = cm.record_hits(block, keys, row_node, k)
            det = cm.classes_detail(block, keys, row_node, par, k, 3, per)
            recs = [r for r in block.split(b"\n") if r]
            assert len(recs) == len(det)
            rows += [(r, d[0], d[1], d[2], lst) for r, d, lst in zip(recs, det, rcm.record_lists(per))]
        out[tname] = rows
    return out


@pytest.mark.parametrize("tname", list(cc.TABLES))
def test_the_device_test_inputs_are_not_vacuous(modelled, tname):
    """what tests/test_read_calls_gpu.py is about is in its inputs, for every table: the staged path at its capacity and one
    node short of it, the general path just beyond and far beyond, a count that 16 bits do not hold, a long record with few nodes
    (general path, short list), a tie, and a list without a class"""
    rows = modelled[tname]
    sizes = [len(lst) for _, _, _, _, lst in rows]
    print(tname, "records", len(rows), "entries", sum(sizes), "largest list", max(sizes), "largest entry", max(c for r in rows for _, c in r[4]))
    assert 0 in sizes                                                                     # an empty list
    for n in (7, 8, 9):
        assert n in sizes, n
    assert max(sizes) >= 16
    assert any(c > 65535 for r in rows for _, c in r[4])                                  # a list entry above 65535
    assert any(len(r[0]) > 4096 and 1 <= len(r[4]) <= 8 for r in rows)                    # more than 4096 positions, at most 8 nodes
    assert any(r[3] and r[1] for r in rows)                                               # a class that came from a tie
    assert any(r[1] == 0 and r[2] < 3 and r[4] for r in rows)                             # a score below M = 3 with a non-empty list
    assert all([v for v, _ in r[4]] == sorted({v for v, _ in r[4]}) and all(v >= 1 and c >= 1 for v, c in r[4]) for r in rows)


# ---------------------------------------------------------------------------------------------- the writer under sanitizers


def test_writer_fuzz_sanitized(tmp_path):
    """tests/read_calls_fuzz.cpp, a stand-alone program (host code, g++) under AddressSanitizer + UBSan: a few thousand damaged
    texts with consistent and inconsistent arrays, without a single bad access, and no failure leaves a file."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "read_calls_fuzz"
    r = subprocess.run(["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "read_calls_fuzz.cpp"), "-o", str(exe), "-lz"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([str(exe), str(work), "2000"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "read_calls_fuzz ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    m = re.search(r"(\d+) tables written, (\d+) calls refused", r.stdout)
    assert int(m.group(1)) > 300 and int(m.group(2)) > 1500      # (one call in eight is consistent by design)
