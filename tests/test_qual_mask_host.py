"""The base-quality mask (-q / --min_base_qual), CPU side: the Python statement of the mask against the real `jellyfish count -Q`
(tests/golden/qual_mask.json, made by tests/golden/make_golden_qual.py), the three new symbols, the commands' refusals, the cache
keys, and the host decoders (in-memory grammar, streaming reader with cut records, host BAM decoder) against that statement."""
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import bamio
from tests import qualmask as qm
from tests import scenarios_fuzz as sf
from tests import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(REPO, "tests", "golden", "qual_mask.json")))


@pytest.fixture
def threshold():
    """set(q) for the test's duration; the process-wide setting is 0 again afterwards."""
    from strainscan_amd import _lib
    yield _lib.set_min_base_qual
    _lib.set_min_base_qual(0)


def _case(g, root):
    return (sf.fmt_case if g["source"] == "fmt" else qm.real_case)(g["seed"], str(root))


def test_golden_set_cannot_pass_by_counting_nothing():
    cases = GOLDEN["cases"]
    assert len(cases) >= 20
    shapes = {k.split("+")[0] for g in cases for k in g["kinds"]}
    assert {"fq4", "fq4_at", "fq_wrap", "fq4_crlf", "fq_plus_name"} <= shapes
    assert any(len(g["kinds"]) == 2 and {k[:2] for k in g["kinds"]} == {"fq", "fa"} for g in cases)
    assert any(k.endswith("+gz") for g in cases for k in g["kinds"])
    for g in cases:
        assert qm.qual_known_deviation(g["kinds"]) is None
        base = [k.split("+")[0] for k in g["kinds"]]
        if any((b.startswith("fq") and b != "fq4") or b == "real" for b in base):
            assert 0 < g["counts_sum"] < g["counts_sum_no_q"], g
    assert {g["q"] for g in cases if g["source"] == "fmt"} <= {1, 2, 3}
    assert {g["q"] for g in cases if g["source"] == "real"} == {10, 20, 30}


@pytest.mark.parametrize("idx", range(len(GOLDEN["cases"])))
def test_mask_definition_equals_jellyfish_Q(idx, tmp_path):
    """The CPU oracle on mask_fastx(X, Q) gives the counts the real `jellyfish count -Q chr(33 + Q)` gave on X, row for row."""
    g = GOLDEN["cases"][idx]
    info, paths, blobs, kinds = _case(g, tmp_path)
    assert kinds == g["kinds"]
    kfa = open(os.path.join(info["db_dir"], "Tree_database", "kmer.fa"), "rb").read()
    assert synth.sha256_of(kfa, *blobs) == g["sha256"], "the scenario's inputs are not the ones jellyfish saw"
    counts, _ = orc.jellyfish_count(kfa, [qm.mask_fastx(b, g["q"]) for b in blobs], k=31, upper=True)
    assert int(counts.sum()) == g["counts_sum"]
    assert synth.sha256_of(counts.astype(np.uint32).tobytes()) == g["counts_sha256"]
    plain, _ = orc.jellyfish_count(kfa, blobs, k=31, upper=True)
    assert int(plain.sum()) == g["counts_sum_no_q"]


def test_symbols_in_header_and_binding():
    from strainscan_amd import _lib
    hdr = open(os.path.join(REPO, "include", "strainscan_hip.h")).read()
    for name, proto in (("ss_set_min_base_qual", r"int\s+ss_set_min_base_qual\s*\(\s*int\s+q\s*\)"),
                        ("ss_get_min_base_qual", r"int\s+ss_get_min_base_qual\s*\(\s*void\s*\)"),
                        ("ss_mask_counters", r"int\s+ss_mask_counters\s*\(\s*uint64_t\s+out\[2\]\s*\)")):
        assert re.search(proto, hdr), name
        assert name in _lib.SIGNATURES
    L = _lib.lib()
    assert L.ss_get_min_base_qual() == 0, "the mask is off by default"
    for bad in (-1, 94, 1000):
        assert L.ss_set_min_base_qual(bad) == _lib.SS_ERANGE and L.ss_get_min_base_qual() == 0
    try:
        for q in (1, 20, 93):
            assert L.ss_set_min_base_qual(q) == _lib.SS_OK and L.ss_get_min_base_qual() == q
    finally:
        L.ss_set_min_base_qual(0)
    import strainscan_amd
    for bad in (94, -1, "x", 2.5, None, True):
        with pytest.raises(ValueError):
            strainscan_amd.set_min_base_qual(bad)
    assert strainscan_amd.get_min_base_qual() == 0


@pytest.mark.parametrize("command", ["strainscan", "strainscan-multi"])
@pytest.mark.parametrize("value", ["94", "-1", "x"])
def test_commands_refuse_a_bad_threshold_before_any_input(command, value, tmp_path):
    """exit status 2, the value named on stderr, and neither -i nor -d is touched (they do not exist) nor -o created"""
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", command), "-i", str(tmp_path / "no_such.fq"), "-d", str(tmp_path / "no_db"),
                        "-o", str(out), "-q=" + value], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=str(tmp_path))
    assert r.returncode == 2, (r.returncode, r.stderr.decode())
    assert "-q/--min_base_qual" in r.stderr.decode() and "0..93" in r.stderr.decode()
    assert not out.exists()


@pytest.mark.parametrize("command", ["strainscan", "strainscan-multi"])
def test_help_names_the_flag(command):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", command), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0
    text = " ".join(r.stdout.decode().split())
    assert "--min_base_qual Q" in text and "jellyfish count -Q" in text and "default: 0" in text


def test_cache_keys_know_the_threshold(tmp_path, threshold):
    from strainscan_amd import db
    p = tmp_path / "a.fq"
    p.write_bytes(b"@r\nACGT\n+\nIIII\n")
    r0, s0 = db._reads_key([str(p)], 0, 1), db._scan_key([str(p)])
    threshold(20)
    r20, s20 = db._reads_key([str(p)], 0, 1), db._scan_key([str(p)])
    threshold(30)
    r30, s30 = db._reads_key([str(p)], 0, 1), db._scan_key([str(p)])
    threshold(0)
    assert len({r0, r20, r30}) == 3 and len({s0, s20, s30}) == 3
    assert db._reads_key([str(p)], 0, 1) == r0 and db._scan_key([str(p)]) == s0


@pytest.mark.parametrize("seed", [1, 5, 8, 16, 23, 31, 46, 51])
def test_host_grammar_and_reader_equal_the_definition(seed, tmp_path, threshold):
    """ss_fastx_to_flat and the streaming reader (buffers so small that records are cut, one longer than the buffer among
    them where the scenario has its `long` record) with the threshold on X == the same calls without it on mask(X);
    ss_mask_counters moves by the definition's count; threshold 0 leaves X as it is."""
    from strainscan_amd import _lib
    info, paths, blobs, kinds = sf.fmt_case(seed, str(tmp_path))
    for q in (0, 2, 25):
        want_n, want_flat, masked_paths = 0, b"", []
        for i, (p, b) in enumerate(zip(paths, blobs)):
            c = [0]
            m = qm.mask_fastx(b, q, c)
            want_n += c[0]
            want_flat += _lib.fastx_to_flat(m)[0]
            mp = str(tmp_path / ("m%d_%d_%s" % (q, i, os.path.basename(p))))
            with (gzip.open(mp, "wb") if p.endswith(".gz") else open(mp, "wb")) as f:
                f.write(m)
            masked_paths.append(mp)
        if q == 0:
            assert want_flat == b"".join(_lib.fastx_to_flat(b)[0] for b in blobs)
        want_blocks = {cap: list(_lib.read_flat_blocks(masked_paths, cap=cap)) for cap in (4096, 5000, 1 << 20)}
        threshold(q)
        c0 = _lib.mask_counters()["masked"]
        got = b"".join(_lib.fastx_to_flat(b)[0] for b in blobs)
        assert _lib.mask_counters()["masked"] - c0 == want_n
        assert got == want_flat, (kinds, q)
        for cap, want in want_blocks.items():
            c0 = _lib.mask_counters()["masked"]
            assert list(_lib.read_flat_blocks(paths, cap=cap)) == want, (kinds, q, cap)
            assert _lib.mask_counters()["masked"] - c0 == want_n
        threshold(0)


def test_reader_truncated_inputs(tmp_path, threshold):
    """A record whose qualities end with the file (or are missing altogether) keeps the bases no quality was read for."""
    from strainscan_amd import _lib
    for i, text in enumerate((b"@a\nACGTACGT\n+\n!!II", b"@a\nACGTACGT\n+\n", b"@a\nACGTACGT", b"@a\nACGT\nACGT\n+\n!I\n!I\n!!!!\n@b\nAC\n+\nI!\n",
                              b"@a\n\n+\n\n@b\nACGT\n+\n!III\n", b"@a\r\nACGT\r\n+\r\nI!II\r\n")):
        p = tmp_path / ("t%d.fq" % i)
        p.write_bytes(text)
        m = tmp_path / ("t%d_masked.fq" % i)
        m.write_bytes(qm.mask_fastx(text, 10))
        want = list(_lib.read_flat_blocks([str(m)], cap=4096))
        want_flat = _lib.fastx_to_flat(qm.mask_fastx(text, 10))
        threshold(10)
        assert list(_lib.read_flat_blocks([str(p)], cap=4096)) == want, text
        assert _lib.fastx_to_flat(text) == want_flat, text
        threshold(0)
    assert qm.mask_fastx(b"@a\nACGT\nACGT\n+\n!I\n!I\n!!!!\n", 10) == b"@a\nNCNT\nNNNN\n+\n!I\n!I\n!!!!\n"


def test_host_bam_decoder_masks_in_stored_order(threshold):
    """ss_bam_decode: qual[i] < Q -> N, reverse-strand records and long reads included; records without qualities are
    left alone and counted once each."""
    from strainscan_amd import _lib
    rs = np.random.RandomState(11)
    reads = [synth.rand_seq(rs, int(rs.choice([150, 150, 37, 1, 2500]))) for _ in range(400)]
    bs = qm.BamSample(12, qm.FastqSample(13, reads), decoys=0.1, extras=True)
    stream = bamio.header() + b"".join(bs.records(0))
    plain = b"".join(r + b"\n" for r in reads)
    for q in (0, 10, 20, 30, 93):
        threshold(q)
        c0 = _lib.mask_counters()
        flat, n = _lib.bam_decode(stream)
        c1 = _lib.mask_counters()
        want, n_masked, n_noq = bs.kept_reads(q), bs.masked(q), bs.no_qual() if q else 0
        assert n == len(reads) and flat == b"".join(r + b"\n" for r in want)
        threshold(0)
        assert _lib.bam_decode(bamio.header() + b"".join(bs.records(q)))[0] == flat          # mask(X) without a threshold
        assert (c1["masked"] - c0["masked"], c1["bam_no_qual"] - c0["bam_no_qual"]) == (n_masked, n_noq)
        if q == 0:
            assert flat == plain
        else:
            assert n_noq > 0 and 0 < n_masked < len(plain)
    threshold(0)
