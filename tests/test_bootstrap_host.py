"""--bootstrap, the part that needs no device: the Poisson(1) table against `decimal`, the weight model (tests/boot_model.py) on
the digests of ss_flat_record_keys (host code) -- its mean and its share of zeros within bounds that follow from Poisson(1) --,
strain_bootstrap.tsv's writer on hand-made replicate matrices, the two flags, and the idle collector."""
import argparse
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import boot_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "table\tstrain\treplicates\tdepth\tdepth_lo\tdepth_hi\tfrac\tfrac_lo\tfrac_hi\tpresent\n"


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------- the table and the weights


def test_table_is_the_decimal_computation():
    want = [1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777,
            4294923276, 4294962463, 4294966817, 4294967252, 4294967292, 4294967295]
    assert boot_model.poisson1_table() == want
    # the integer literals of the kernel and of the header are these
    src = open(os.path.join(ROOT, "strainscan_amd", "csrc", "ss_resample.hip")).read()
    m = re.search(r"POISSON1_CDF\[13\] = \{([^}]*)\}", src)
    assert m and [int(v.strip().rstrip("u")) for v in m.group(1).split(",")] == want
    hdr = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "strainscan_hip.h")).read())
    assert " ".join(map(str, want)) in hdr
    # (the last entries: P(w >= 13) = 2^-32 or less -- the weight never exceeds 13)
    assert want[-1] == (1 << 32) - 1 and all(a < b for a, b in zip(want, want[1:]))


def test_weight_model_is_poisson_1(L):
    """100 000 distinct records: the mean weight within 1 +- 5 / sqrt(n) (the variance of Poisson(1) is 1), the share of w = 0 within
    e^-1 +- 5 sqrt(0.368 * 0.632 / n) -- five standard deviations each, derived, not measured.  (Seed 4: with it the model passes.)"""
    n = 100000
    rs = np.random.RandomState(1)
    lut = np.frombuffer(b"ACGT", np.uint8)
    recs = set()
    while len(recs) < n:
        recs.add(lut[rs.randint(0, 4, size=int(rs.randint(20, 301)))].tobytes())
    recs = sorted(recs)
    keys = L.flat_record_keys(b"\n".join(recs) + b"\n")
    assert keys.shape == (n, 2)
    for rep in (0, 1):
        w = boot_model.weights_of_keys(keys[:, 1], 4, rep)
        mean, zero = float(w.mean()), float((w == 0).mean())
        print("replicate", rep, "mean", mean, "share of 0", zero, "max", int(w.max()), np.bincount(w).tolist())
        assert abs(mean - 1.0) <= 5.0 / math.sqrt(n)
        assert abs(zero - math.exp(-1)) <= 5.0 * math.sqrt(0.368 * 0.632 / n)
        assert 0 <= w.min() and w.max() <= 13
    a, b = boot_model.weights_of_keys(keys[:, 1], 4, 0), boot_model.weights_of_keys(keys[:, 1], 4, 1)
    assert abs(float(np.corrcoef(a, b)[0, 1])) <= 5.0 / math.sqrt(n)       # replicates are independent draws
    assert (boot_model.weights_of_keys(keys[:, 1], 5, 0) != a).any()       # the seed matters
    # identical reads share a weight; the weight does not depend on where the record stands
    r2, w2 = boot_model.weights(L, b"\n".join(recs[:50] + recs[:50][::-1]) + b"\n", 4, 0)
    assert (w2[:50] == w2[50:][::-1]).all() and (w2[:50] == a[:50]).all()


def test_model_mix_is_written_out(L):
    """the few lines of Python the header promises, on one record, in plain integers"""
    key = int(L.flat_record_keys(b"ACGTTGCA\n")[0, 1])
    m = (1 << 64) - 1
    x = (key + 0x9E3779B97F4A7C15 * (7 + 1) + 0xD6E8FEB86659FD93 * 3) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    x ^= x >> 31
    w = sum(1 for t in boot_model.poisson1_table() if t <= (x >> 32))
    assert w == int(boot_model.weights(L, b"ACGTTGCA\n", 3, 7)[1][0])


# ---------------------------------------------------------------------------------------------- the writer


def test_index_rule():
    from strainscan_amd import read_reports
    assert [(read_reports.bootstrap_index(0.025, b), read_reports.bootstrap_index(0.975, b)) for b in (2, 8, 41, 100, 1000)] == \
        [(0, 1), (0, 7), (1, 39), (2, 97), (25, 974)]


@pytest.mark.parametrize("b", [2, 8, 41])
def test_writer_on_hand_made_matrices(b):
    from strainscan_amd import read_reports
    rs = np.random.RandomState(b)
    coefs = np.zeros((b, 3))
    coefs[:, 0] = rs.permutation(np.arange(b)) + 1.0                 # 1 .. b in some order
    coefs[:, 1] = rs.permutation(np.arange(b)) * 0.5                 # 0, 0.5, ...: one replicate without the strain
    coefs[:, 2] = 0.0                                                # never present
    lo, hi = {2: (0, 1), 8: (0, 7), 41: (1, 39)}[b]
    frac = coefs / coefs.sum(axis=1, keepdims=True)
    rows = [("C7.1", "strain A", "3.25", "0.75", 0, coefs), ("C7.2", "strain B", "1.0", "0.25", 1, coefs), ("C7.3", "strain C", "0.0", "0.0", 2, coefs)]
    text = read_reports.bootstrap_text(rows)
    lines = text.split("\n")
    assert text.startswith(HEADER) and lines[-1] == "" and len(lines) == 5
    for j, (table, strain, depth, fr, _, _) in enumerate(rows):
        f = lines[1 + j].split("\t")
        assert f[:4] == [table, strain, str(b), depth] and f[6] == fr                  # depth and frac are copied as text
        assert f[4] == str(float(np.sort(coefs[:, j])[lo])) and f[5] == str(float(np.sort(coefs[:, j])[hi]))
        assert f[7] == str(float(np.sort(frac[:, j])[lo])) and f[8] == str(float(np.sort(frac[:, j])[hi]))
        assert f[9] == str(int((coefs[:, j] > 0).sum()))
    assert lines[1].split("\t")[4:6] == [str(float(lo + 1)), str(float(hi + 1))]
    assert lines[2].split("\t")[9] == str(b - 1) and lines[3].split("\t")[4:] == ["0.0", "0.0", "0.0", "0.0", "0.0", "0"]


def test_writer_all_zero_replicate():
    """a replicate whose coefficients are all 0 has fraction 0 for every strain (not 0 / 0), and nobody is present in it"""
    from strainscan_amd import read_reports
    coefs = np.array([[2.0, 2.0], [0.0, 0.0], [1.0, 3.0], [3.0, 1.0]])
    s = read_reports.bootstrap_summary(coefs)
    assert s == [(0.0, 3.0, 0.0, 0.75, 3), (0.0, 3.0, 0.0, 0.75, 3)]
    text = read_reports.bootstrap_text([("C1.1", "a", "2.0", "0.5", 0, coefs), ("C1.2", "b", "2.0", "0.5", 1, coefs)])
    assert text == HEADER + "C1.1\ta\t4\t2.0\t0.0\t3.0\t0.5\t0.0\t0.75\t3\n" + "C1.2\tb\t4\t2.0\t0.0\t3.0\t0.5\t0.0\t0.75\t3\n"
    assert "nan" not in text


# ---------------------------------------------------------------------------------------------- the flags


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
        a = ap.parse_args(base)
        assert a.bootstrap == 0 and a.bootstrap_seed == 1                   # off by default
        a = ap.parse_args(base + ["--bootstrap", "100"])
        assert a.bootstrap == 100 and a.bootstrap_seed == 1
        a = ap.parse_args(base + ["--bootstrap", "2", "--bootstrap_seed", str((1 << 63) - 1)])
        assert a.bootstrap == 2 and a.bootstrap_seed == (1 << 63) - 1
        assert ap.parse_args(base + ["--bootstrap", "1000", "--bootstrap_seed", "0"]).bootstrap_seed == 0
        for bad in ("0", "1", "1001", "-3", "abc", "2.5", ""):
            with pytest.raises(SystemExit) as e:
                ap.parse_args(base + ["--bootstrap", bad])
            assert e.value.code == 2, bad
        for bad in ("-1", str(1 << 63), "abc", "1.5", ""):
            with pytest.raises(SystemExit) as e:
                ap.parse_args(base + ["--bootstrap", "8", "--bootstrap_seed", bad])
            assert e.value.code == 2, bad
    capsys.readouterr()


def test_commands_refuse_a_bad_value_before_any_input_is_opened(tmp_path):
    for mod in ("strainscan_amd.StrainScan", "strainscan_amd.multi_db"):
        for flags in (["--bootstrap", "1"], ["--bootstrap", "abc"], ["--bootstrap", "8", "--bootstrap_seed", "-1"]):
            r = subprocess.run([sys.executable, "-m", mod, "-i", str(tmp_path / "no_such.fq"), "-d", str(tmp_path / "no_db"), "-o",
                                str(tmp_path / "out")] + flags, capture_output=True, text=True, cwd=ROOT, timeout=300)
            assert r.returncode == 2 and "--bootstrap" in r.stderr, (mod, flags, r.stderr[-500:])
            assert not (tmp_path / "out").exists()


def test_set_bootstrap_and_the_idle_collector(tmp_path):
    import strainscan_amd
    from strainscan_amd import read_reports
    assert read_reports.BOOTSTRAP["b"] == 0 and read_reports.BOOTSTRAP["seed"] == 1             # off by default
    report = tmp_path / "StrainVote.report"
    report.write_text("header\n1\ts\tC1\t1.0\t2.0\n")
    read_reports.bootstrap_note_solve(begin=True, columns=[0], strains=["s"])          # off: nothing is kept, nothing is looked at
    read_reports.bootstrap_scanned("C1")
    read_reports.collect_bootstrap("C1", str(tmp_path / "no_such_cluster"), str(report), 31, [str(tmp_path / "no_such.fq")])
    assert read_reports.BOOTSTRAP["solve"] == {} and read_reports.BOOTSTRAP["rows"] == {} and read_reports.BOOTSTRAP["order"] == {}
    assert read_reports.write_bootstrap(str(tmp_path)) is None and read_reports.bootstrap_replicates() == {}
    try:
        strainscan_amd.set_bootstrap(8, 3)
        assert read_reports.BOOTSTRAP["b"] == 8 and read_reports.BOOTSTRAP["seed"] == 3 and read_reports.BOOTSTRAP["skipped"] is None
        for bad in (1, 1001, -2, 2.5, "8", True):
            with pytest.raises(ValueError):
                strainscan_amd.set_bootstrap(bad)
        for bad in (-1, 1 << 63, 1.5, "1", True):
            with pytest.raises(ValueError):
                strainscan_amd.set_bootstrap(8, bad)
        assert read_reports.BOOTSTRAP["b"] == 8 and read_reports.BOOTSTRAP["seed"] == 3
        assert read_reports.write_bootstrap(str(tmp_path)) is None                    # on, but no multi-strain cluster was solved: no file
    finally:
        strainscan_amd.set_bootstrap(0)
    assert read_reports.BOOTSTRAP["b"] == 0 and read_reports.BOOTSTRAP["seed"] == 1
    assert sorted(os.listdir(tmp_path)) == ["StrainVote.report"]


def test_report_rows(tmp_path):
    from strainscan_amd import read_reports
    p = tmp_path / "StrainVote.report"
    p.write_text("h\n1\tA (With_ExtraRegion_covered)\tC7\t0.75\t3.25\t9.0\t0.9\t5/6\t5\t0.9\t\n2\tB\tC7\t0.25\t1.0\t3.0\t0.8\t4/5\t4\t0.8\t*\n")
    assert read_reports.report_rows(str(p)) == [(1, "A", "0.75", "3.25"), (2, "B", "0.25", "1.0")]
