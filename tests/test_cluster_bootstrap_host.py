"""--bootstrap_clusters, the part that needs no device: cluster_bootstrap.tsv's writer on a hand-made main dict and replicate list,
the flag in both commands' parsers, the package entry point and the idle collector, and the new symbols of the built library."""
import argparse
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "cluster\tcalled\treplicates\tpresent\tdepth\tdepth_lo\tdepth_hi\tcov\tcov_lo\tcov_hi\n"


def _rows(text):
    assert text.startswith(HEADER) and text.endswith("\n")
    return [line.split("\t") for line in text[len(HEADER):].split("\n")[:-1]]


def test_writer_on_a_hand_made_list():
    from strainscan_amd import read_reports as rr
    main = {12: (8.0, 0.9), 5: (2.5, 0.5)}
    reps = [{12: (7.0, 0.8), 5: (2.0, 0.4)},
            {12: (9.0, 0.95)},
            {},                                               # a failed replicate: it called no cluster
            {12: (8.5, 0.85), 5: (3.0, 0.6), 40: (1.0, 0.25)}]
    rows = _rows(rr.cluster_bootstrap_text(main, reps))
    # ascending leaf id; B = 4: the bounds are the values at index 0 and 3 of the ascending replicate values, absent = 0.0
    assert rows == [["C5", "1", "4", "2", "2.5", "0.0", "3.0", "0.5", "0.0", "0.6"],
                    ["C12", "1", "4", "3", "8.0", "0.0", "9.0", "0.9", "0.0", "0.95"],
                    ["C40", "0", "4", "1", "-", "0.0", "1.0", "-", "0.0", "0.25"]]
    # present in all replicates: the bounds are real values
    rows = _rows(rr.cluster_bootstrap_text({3: (4.0, 0.7)}, [{3: (5.0, 0.6)}, {3: (3.0, 0.8)}]))
    assert rows == [["C3", "1", "2", "2", "4.0", "3.0", "5.0", "0.7", "0.6", "0.8"]]
    # a main cluster that no replicate called keeps its row
    rows = _rows(rr.cluster_bootstrap_text({3: (4.0, 0.7)}, [{}, {}]))
    assert rows == [["C3", "1", "2", "0", "4.0", "0.0", "0.0", "0.7", "0.0", "0.0"]]
    assert rr.cluster_bootstrap_text({}, []) == HEADER


@pytest.mark.parametrize("b, lo, hi", [(2, 0, 1), (3, 0, 2), (40, 1, 38)])
def test_quantile_index(b, lo, hi):
    """floor(q (B - 1) + 0.5) at q = 0.025 and 0.975, strain_bootstrap.tsv's rule: replicate r has depth r + 1 and coverage
    (r + 1) / 100, so the value names its index"""
    from strainscan_amd import read_reports as rr
    assert (rr.bootstrap_index(0.025, b), rr.bootstrap_index(0.975, b)) == (lo, hi)
    reps = [{9: (float(r + 1), (r + 1) / 100.0)} for r in reversed(range(b))]
    (row,) = _rows(rr.cluster_bootstrap_text({9: (1.0, 0.5)}, reps))
    assert row == ["C9", "1", str(b), str(b), "1.0", str(float(lo + 1)), str(float(hi + 1)), "0.5", str((lo + 1) / 100.0), str((hi + 1) / 100.0)]


def _parsers():
    from strainscan_amd import StrainScan
    out = []
    for multi in (False, True):
        ap = argparse.ArgumentParser(prog="x")
        StrainScan.add_arguments(ap, multi=multi)
        out.append(ap)
    return out


def test_flag_parsing(capsys):
    from strainscan_amd import StrainScan
    for ap in _parsers():                                     # (the second is strainscan-multi's)
        base = ["-i", "r.fq", "-d", "DB"]
        assert ap.parse_args(base).bootstrap_clusters == 0    # off by default
        a = ap.parse_args(base + ["--bootstrap_clusters", "100", "--bootstrap_seed", "7"])
        assert a.bootstrap_clusters == 100 and a.bootstrap_seed == 7 and a.bootstrap == 0
        a = ap.parse_args(base + ["--bootstrap_clusters", "2", "--bootstrap", "1000"])
        assert a.bootstrap_clusters == 2 and a.bootstrap == 1000
        for bad in ("0", "1", "1001", "x", "2.5", "-4", ""):
            with pytest.raises(SystemExit) as e:
                ap.parse_args(base + ["--bootstrap_clusters", bad])
            assert e.value.code == 2, bad
        # --pairs admits it as a report of its own
        a = ap.parse_args(base + ["-j", "r2.fq", "--pairs", "--bootstrap_clusters", "4"])
        StrainScan.refuse_pairs_alone(ap, a)
        with pytest.raises(SystemExit) as e:
            StrainScan.refuse_pairs_alone(ap, ap.parse_args(base + ["-j", "r2.fq", "--pairs"]))
        assert e.value.code == 2
    capsys.readouterr()


def test_commands_refuse_a_bad_value_before_any_input_is_opened(tmp_path):
    for mod in ("strainscan_amd.StrainScan", "strainscan_amd.multi_db"):
        for bad in ("1", "1001", "x", "2.5"):
            r = subprocess.run([sys.executable, "-m", mod, "-i", str(tmp_path / "no_such.fq"), "-d", str(tmp_path / "no_db"), "-o",
                                str(tmp_path / "out"), "--bootstrap_clusters", bad], capture_output=True, text=True, cwd=ROOT, timeout=300)
            assert r.returncode == 2 and "--bootstrap_clusters" in r.stderr, (mod, bad, r.stderr[-500:])
            assert not (tmp_path / "out").exists()


def test_entry_point_and_the_idle_collector(tmp_path):
    import strainscan_amd
    from strainscan_amd import read_reports as rr
    assert rr.CLUSTER_BOOTSTRAP["b"] == 0 and rr.CLUSTER_BOOTSTRAP["seed"] == 1          # off by default
    # off: nothing is looked at (no such database, no such file), nothing is kept, nothing is written
    rr.collect_cluster_bootstrap({3: {"cls_ab": 1.0, "cls_cov": 0.5}}, str(tmp_path / "no_db"), 0, 0, [str(tmp_path / "no_such.fq")])
    assert rr.CLUSTER_BOOTSTRAP["rows"] == {} and rr.CLUSTER_BOOTSTRAP["skipped"] == {}
    assert rr.write_cluster_bootstrap(str(tmp_path)) is None and rr.cluster_bootstrap_replicates() == [] and rr.cluster_bootstrap_failed() == 0
    try:
        strainscan_amd.set_bootstrap_clusters(8, 3)
        assert rr.CLUSTER_BOOTSTRAP["b"] == 8 and rr.CLUSTER_BOOTSTRAP["seed"] == 3 and rr.BOOTSTRAP["b"] == 0
        for bad in (1, 1001, -2, 2.5, "8", True):
            with pytest.raises(ValueError):
                strainscan_amd.set_bootstrap_clusters(bad)
        for bad in (-1, 1 << 63, 1.5, "1", True):
            with pytest.raises(ValueError):
                strainscan_amd.set_bootstrap_clusters(8, bad)
        assert rr.CLUSTER_BOOTSTRAP["b"] == 8 and rr.CLUSTER_BOOTSTRAP["seed"] == 3
        assert rr.write_cluster_bootstrap(str(tmp_path)) is None                          # on, but no walk was resampled: no file
        rr.reset_all()                                                                    # the commands end with it
        assert rr.CLUSTER_BOOTSTRAP["b"] == 0
    finally:
        strainscan_amd.set_bootstrap_clusters(0)
    assert rr.CLUSTER_BOOTSTRAP["b"] == 0 and rr.CLUSTER_BOOTSTRAP["seed"] == 1
    assert os.listdir(tmp_path) == []
    assert rr.cluster_bootstrap_walk_seed(7, 3) != rr.cluster_bootstrap_walk_seed(7, 4) != rr.cluster_bootstrap_walk_seed(8, 3)


def test_the_ladder_is_the_reference_one():
    """identify_with_ladder and the replicates' walks read one table of cutoffs (StrainScan.py:192-217)"""
    from strainscan_amd import StrainScan
    assert StrainScan.LADDER_CUTOFFS == {0: ([0.1, 0.4, 1], [0.05, 0.05, 1]), 1: ([0.01, 0.05, 1],), 2: ([0.005, 0.01, 1],)}
    with pytest.raises(ValueError):
        StrainScan.identify_with_ladder(("no_such.fq", ""), "no_db", 3, 0)


def test_new_symbols_are_exported():
    """the built library exports the two calls, and the binding declares them (lib() resolves every declared symbol)"""
    import ctypes
    from strainscan_amd import _lib
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ss_scan_reads_resampled", "ss_scan_reads_resampled_calls"):
        assert getattr(so, name) is not None
        assert name in _lib.SIGNATURES
    assert _lib.SCAN_REPLICATES_MAX == 16
    with open(os.path.join(ROOT, "include", "strainscan_hip.h")) as f:
        assert "#define SS_SCAN_REPLICATES_MAX 16" in f.read()
