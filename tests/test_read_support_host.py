"""--read_support without a device: the flag on both commands, the ge* columns from a 65-bin histogram, the exact text of
read_support.tsv for a fixed collector state."""
import argparse
import os

import pytest


def _parser(multi):
    from strainscan_amd import StrainScan
    ap = argparse.ArgumentParser()
    StrainScan.add_arguments(ap, multi=multi)
    return ap


@pytest.mark.parametrize("multi", [False, True])
def test_parser_accepts_the_flag_and_defaults_to_off(multi):
    base = ["-i", "r.fq", "-d", "DB"]
    assert _parser(multi).parse_args(base).read_support is False
    assert _parser(multi).parse_args(base + ["--read_support"]).read_support is True
    with pytest.raises(SystemExit):
        _parser(multi).parse_args(base + ["--read_support", "1"])       # store_true: it takes no value


def test_multi_command_parses_the_flag(tmp_path):
    from strainscan_amd import multi_db
    for n in ("a", "b"):
        os.makedirs(str(tmp_path / n / "Tree_database"))
    argv = ["-i", "r.fq", "-d", str(tmp_path / "a"), "-d", str(tmp_path / "b")]
    assert multi_db.parse_args(argv)[0].read_support is False
    assert multi_db.parse_args(argv + ["--read_support"])[0].read_support is True


def test_ge_columns_from_a_histogram():
    from strainscan_amd import read_reports
    h = [0] * 65
    h[0], h[1], h[2], h[3], h[4], h[7], h[8], h[15], h[16], h[31], h[32], h[63], h[64] = 100, 9, 8, 7, 6, 5, 4, 3, 2, 1, 10, 20, 30
    # ge1 = everything but bin 0; ge2 drops bin 1; ge4 drops bins 2, 3; ge8 drops 4..7; ge16 drops 8..15; ge32 drops 16..31; ge64 = bin 64
    assert read_reports.read_support_ge(h) == [105, 96, 81, 70, 63, 60, 30]
    assert read_reports.read_support_ge([5] + [0] * 64) == [0] * 7
    all_in_last = [0] * 64 + [12]
    assert read_reports.read_support_ge(all_in_last) == [12] * 7
    with pytest.raises(AssertionError):
        read_reports.read_support_ge([0] * 64)


def test_tsv_text_of_a_fixed_collector_state(tmp_path):
    from strainscan_amd import read_reports
    h_tree = [90, 4, 3, 2] + [0] * 60 + [1]
    h_c = [10] + [0] * 63 + [90]
    read_reports.read_support_reset(True)
    try:
        read_reports.READ_SUPPORT["rows"][None] = {"tree": ("tree", 1234, 100, 321, h_tree), "C7": ("C7", 999999, 100, 12345, h_c)}
        read_reports.READ_SUPPORT["rows"]["other"] = {"tree": ("tree", 1, 2, 3, [2] + [0] * 64)}
        path = read_reports.write_read_support(str(tmp_path))
        assert path == str(tmp_path / "read_support.tsv")
        assert open(path).read() == ("table\tkmers\treads\thits\tge1\tge2\tge4\tge8\tge16\tge32\tge64\n"
                                     "tree\t1234\t100\t321\t10\t6\t1\t1\t1\t1\t1\n"
                                     "C7\t999999\t100\t12345\t90\t90\t90\t90\t90\t90\t90\n")
        os.makedirs(str(tmp_path / "o"))
        assert open(read_reports.write_read_support(str(tmp_path / "o"), "other")).read().split("\n")[1] == "tree\t1\t2\t3\t0\t0\t0\t0\t0\t0\t0"
        # nothing is written for a scope without rows, after a skip, or with the flag off
        os.makedirs(str(tmp_path / "p"))
        assert read_reports.write_read_support(str(tmp_path / "p"), "none") is None
        read_reports.READ_SUPPORT["skipped"] = "why"
        assert read_reports.write_read_support(str(tmp_path / "p")) is None
        read_reports.READ_SUPPORT["skipped"] = None
        read_reports.READ_SUPPORT["on"] = False
        assert read_reports.write_read_support(str(tmp_path / "p")) is None
        assert os.listdir(str(tmp_path / "p")) == []
    finally:
        read_reports.read_support_reset()
    assert read_reports.READ_SUPPORT == {"on": False, "rows": {}, "skipped": None}
    assert read_reports.SCOPE["label"] is None


def test_package_setter_turns_the_collector_on_and_off():
    import strainscan_amd
    from strainscan_amd import read_reports
    strainscan_amd.set_read_support(True)
    try:
        assert read_reports.READ_SUPPORT["on"] is True
    finally:
        strainscan_amd.set_read_support(False)
    assert read_reports.READ_SUPPORT["on"] is False and read_reports.READ_SUPPORT["rows"] == {}


def test_collector_is_a_no_op_while_off():
    from strainscan_amd import read_reports
    read_reports.read_support_reset()
    read_reports.collect_read_support("tree", object(), ["no such file"])       # (would fail on either argument if it looked at them)
    assert read_reports.READ_SUPPORT["rows"] == {}
