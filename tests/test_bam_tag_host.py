"""`--tag_bam` without a device: the model (tests/bam_tag_model.py) on a stream whose output is spelled out byte by byte, its aux
field walk, the new entry points in the header and the library, the command line's refusals, and the tagged-record copy of
strainscan_amd/csrc/ss_tag_copy.h played on the host under AddressSanitizer + UBSan (tests/tag_copy_check.cpp).  What the device
does is tests/test_bam_tag_gpu.py's."""
import argparse
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import bam_tag_model as btm, bamio, rs_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = bamio.header()


def test_two_records_byte_for_byte():
    seq = "ACGT" * 7 + "ACG"
    s = HDR + bamio.record("r", seq, flag=4, aux=b"XAAx") + bamio.record("q", "AC", flag=0x100, aux=b"snA!")
    fixed = bytes.fromhex("ffffffff ffffffff 02 ff 4812 0000")                 # ref, pos, l_read_name, mapq, bin, n_cigar_op
    mate = bytes.fromhex("ffffffff ffffffff 00000000")                       # next ref, next pos, tlen
    kept_in = (bytes.fromhex("55000000") + fixed + bytes.fromhex("0400 1f000000") + mate + b"r\0" + bytes.fromhex("1248" * 7 + "1240") +
               b"\x1e" * 31 + b"XAAx")
    other = bytes.fromhex("29000000") + fixed + bytes.fromhex("0001 02000000") + mate + b"q\0" + bytes.fromhex("12") + b"\x1e" * 2 + b"snA!"
    assert s == HDR + kept_in + other
    kept_out = (bytes.fromhex("63000000") + kept_in[4:] + b"sni" + bytes.fromhex("4d000000") + b"sci" + bytes.fromhex("01000000"))
    keys = rs_model.encode_kmers([seq.encode()], 31)
    args = (keys, np.array([1], np.uint32), np.array([0, 0], np.uint32), 1, 31)
    body, c, direct, hits, kmers = btm.model(s, *args, 1, np.array([-1, 77], np.int32))
    assert body == kept_out + other and len(body) == len(s) - len(HDR) + 14
    assert c == [2, 1, 1, 0, 1, 0] and direct.tolist() == [0, 1] and hits.tolist() == [0, 1] and kmers.tolist() == [0, 1]
    assert btm.read_tags(body) == [(4, b"r", 77, 1), (0x100, b"q", None, None)]
    assert btm.offsets(s) == [(0, 103, True), (103, 148, False)]
    # below M: class 0, its value, and the score all the same; other tags
    body, c, direct, _, _ = btm.model(s, *args, 2, np.array([-1, 77], np.int32), tags=b"XaXb")
    assert body == kept_out[:-14] + b"Xai" + bytes.fromhex("ffffffff") + b"Xbi" + bytes.fromhex("01000000") + other
    assert c == [2, 1, 0, 0, 1, 0] and direct.tolist() == [1, 0]
    # the kept record bears a tag / is damaged: no body; on the record that is not kept neither matters
    for aux, n in ((b"sci\0\0\0\0", 1), (b"XAAx" + b"snZ\0", 1), (b"XZZ", 0), (b"snA!" + b"XZZ", 0)):
        body, c, _, _, _ = btm.model(HDR + bamio.record("r", seq, flag=4, aux=aux) + other, *args, 1, np.array([-1, 77], np.int32))
        assert body is None and c[3] == n, aux
    assert btm.model(HDR + kept_in + bamio.record("q", "AC", flag=0x800, aux=b"XZZ"), *args, 1, np.array([-1, 77], np.int32))[0] is not None
    # pairs: both mates get the fragment's class and score
    pair = HDR + bamio.record("p", seq, flag=0x41) + bamio.record("x", "ACGT", flag=4) + bamio.record("p", bamio.revcomp(seq), flag=0x91)
    body, c, direct, _, _ = btm.model(pair, *args, 2, np.array([-1, 77], np.int32), pairs=True)
    assert btm.read_tags(body) == [(0x41, b"p", 77, 2), (4, b"x", -1, 0), (0x91, b"p", 77, 2)] and c == [3, 3, 2, 0, 2, 0]
    body, c, direct, _, _ = btm.model(pair, *args, 2, np.array([-1, 77], np.int32))
    assert btm.read_tags(body) == [(0x41, b"p", -1, 1), (4, b"x", -1, 0), (0x91, b"p", -1, 1)] and c == [3, 3, 0, 0, 3, 0]


def test_aux_walk_of_the_model():
    ok = [b"XAAs", b"XccS", b"XCCn", b"XssSN", b"XSSsn", b"XiisnSC", b"XIIscsn", b"XffSNSC", b"XZZsnsc\0", b"XHH5A\0", b"XzZ\0"]
    ok += [b"XBB" + sub + struct.pack("<I", c) + b"s" * (c * size) for sub, size in ((b"c", 1), (b"C", 1), (b"s", 2), (b"S", 2), (b"i", 4),
                                                                                        (b"I", 4), (b"f", 4)) for c in (0, 1, 5)]
    for f in ok:
        assert btm.aux_walk(f, b"snsc") == btm.AUX_OK, f
        assert [x[:2] for x in btm.aux_fields(f)] == [(f[:2], f[2])]
    every = b"".join(ok)
    assert btm.aux_walk(b"", b"snsc") == btm.AUX_OK and btm.aux_walk(every, b"snsc") == btm.AUX_OK and len(btm.aux_fields(every)) == len(ok)
    for t in (b"snix123", b"scZab\0", b"snA!", b"scBc\1\0\0\0x"):
        for aux in (t, t + every, every + t, ok[0] + t + every):
            assert btm.aux_walk(aux, b"snsc") == btm.AUX_TAGGED, aux
            assert btm.aux_walk(aux, b"XaXb") == btm.AUX_OK
    assert btm.aux_walk(b"nsiabcd" + b"SNiabcd", b"snsc") == btm.AUX_OK       # other names: the order and the case of the letters count
    # the three malformed forms: an unknown type, a Z without its NUL, a B whose count runs past the end -- and a field cut short
    for bad in (b"XXz1234", b"XX\0123", b"XXd1234", b"XZZabc", b"XHHabc", b"XBBi\5\0\0\0" + b"x" * 19, b"XBBs\xff\xff\xff\xff" + b"ab",
                b"XBBA\1\0\0\0x", b"XBBc\1\0", b"XiIabc", b"XAAxY", b"XA", b"X"):
        for aux in (bad, every + bad, b"snA!" + bad):                         # (damaged wins over tagged)
            assert btm.aux_walk(aux, b"snsc") == btm.AUX_DAMAGED, aux
    for f in ok:
        for cut in range(1, len(f)):
            assert btm.aux_walk(f[:cut], b"snsc") == btm.AUX_DAMAGED, (f, cut)


NEW = ("ss_bam_tag_stream", "ss_bam_tag_file", "ss_bam_tag_calls", "ss_bam_tag_timing")


def test_new_symbols_are_declared_and_exported():
    from strainscan_amd import _lib
    header = open(os.path.join(REPO, "include", "strainscan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, code), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert re.search(r"#define SS_BAM_TAG_BYTES 14\b", code) and _lib.BAM_TAG_BYTES == btm.TAG_BYTES == 14
    assert len(_lib.SIGNATURES["ss_bam_tag_stream"][1]) == 17 and len(_lib.SIGNATURES["ss_bam_tag_file"][1]) == 14
    assert _lib.BAM_TAG_COUNTERS == btm.COUNTERS and len(_lib.BAM_TAG_STEPS) == 8
    # host-only refusals: a NULL where a pointer must stand, before any device is touched
    assert lib.ss_bam_tag_calls(None) == _lib.SS_EINVAL and lib.ss_bam_tag_timing(None) == _lib.SS_EINVAL
    assert _lib.bam_tag_calls() >= 0 and set(_lib.bam_tag_timing()) == set(_lib.BAM_TAG_STEPS)
    import strainscan_amd
    assert callable(strainscan_amd.set_tag_bam)


def test_command_line_refusals(tmp_path, capsys):
    """--tag_bam without --classify_reads, and with a FASTQ input: exit status 2 before anything is opened or made"""
    from strainscan_amd import StrainScan, multi_db, read_reports
    bam, fq, out = tmp_path / "s.bam", tmp_path / "s.fq", tmp_path / "out"
    bam.write_bytes(bamio.bgzf(HDR, [bamio.record("r", "ACGT" * 10)]))
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    ap = argparse.ArgumentParser()
    StrainScan.add_arguments(ap)
    assert ap.parse_args(["-i", str(bam), "-d", "db"]).tag_bam is False                                   # off by default
    StrainScan.refuse_tag_bam_alone(ap, ap.parse_args(["-i", str(fq), "-d", "db"]))                       # ... and then nothing is looked at
    StrainScan.refuse_tag_bam_alone(ap, ap.parse_args(["-i", str(bam), "-d", "db", "--classify_reads", "2", "--tag_bam"]))
    StrainScan.refuse_tag_bam_alone(ap, ap.parse_args(["-i", str(bam), "-j", str(bam), "-d", "db", "--classify_reads", "2", "--tag_bam"]))
    for argv in (["-i", str(bam), "--tag_bam"], ["-i", str(fq), "--classify_reads", "2", "--tag_bam"],
                 ["-i", str(bam), "-j", str(fq), "--classify_reads", "2", "--tag_bam"],
                 ["-i", str(tmp_path / "absent.bam"), "--classify_reads", "2", "--tag_bam"]):
        for main, dbs in ((StrainScan.main, ["-d", str(tmp_path / "no_db")]), (multi_db.main, ["-d", str(tmp_path / "a"), "-d", str(tmp_path / "b")])):
            with pytest.raises(SystemExit) as e:
                main(argv + dbs + ["-o", str(out)])
            assert e.value.code == 2, argv
            assert "--tag_bam needs" in capsys.readouterr().err
    assert sorted(os.listdir(tmp_path)) == ["s.bam", "s.fq"]
    assert read_reports.TAG_BAM["on"] is False
    read_reports.tag_bam_reset(True, str(out))
    assert read_reports.TAG_BAM == dict(on=True, dir=str(out), skipped=None, files=[])
    read_reports.reset_all()
    assert read_reports.TAG_BAM["on"] is False and read_reports.TAG_BAM["dir"] is None


def test_tag_copy_sweep_sanitized(tmp_path):
    """Exhaustive: D mod 16 x record lengths 36..83 x tagged / untagged x the record at the start, inside and at the end of a source
    block of exactly that size, against a memcpy composition; guard bytes around every span stay untouched; a load outside a source
    block, or an undefined shift, stops the program.  And aux_walk on every field type and the malformed forms, on heap blocks of
    exactly the fields' bytes."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "tag_copy_check"
    r = subprocess.run(["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(REPO, "strainscan_amd", "csrc"), os.path.join(REPO, "tests", "tag_copy_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "tag_copy_check ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    m = re.search(r"(\d+) copies, (\d+) walks", r.stdout)
    assert int(m.group(1)) >= 48 * 16 * 2 * 3 * 4 and int(m.group(2)) > 150      # lengths x offsets x tagged x values x positions
