"""strainscan_amd/read_reports.py on the host: the hooks the scans and the solver call, the one skip routine and its exact lines on
stderr, and the one scope of strainscan-multi.  What the collectors compute on the device is tests/test_*_cli_gpu.py's."""
import os
import types

import numpy as np
import pytest

IDLE = {"READ_SUPPORT": {"on": False, "rows": {}, "skipped": None},
        "EXTRACT_READS": {"n": 0, "dir": None, "done": {}, "skipped": None, "files": []},
        "BY_STRAIN": {"on": False, "rows": {}},
        "BOOTSTRAP": {"b": 0, "seed": 1, "solve": {}, "rows": {}, "order": {}, "skipped": None}}
K_TOO_SMALL = "needs page-index tables (17 <= k <= 31), this run's k is 15,"
NOT_RESIDENT = "needs the sample resident on the device (SS_READS_RESIDENT_GB)"
CLOSING = {"read_support": "and was not computed", "extract_reads": "and nothing was extracted",
           "bootstrap": "and no intervals were computed"}


@pytest.fixture
def rr():
    from strainscan_amd import read_reports
    read_reports.reset_all()
    yield read_reports
    read_reports.reset_all()


def _states(rr):
    return {name: getattr(rr, name) for name in IDLE}


def test_the_idle_hooks_look_at_nothing(rr, tmp_path):
    rr.table_scanned("tree", object(), ["no such file"])                 # (would fail on either argument if it looked at them)
    rr.cluster_reported("C1", str(tmp_path / "no_such_cluster"), str(tmp_path / "no_such.report"), 31, ["no such file"])
    rr.write_all(str(tmp_path / "no_such_dir"))
    assert _states(rr) == IDLE and rr.SCOPE["label"] is None
    assert os.listdir(tmp_path) == []


def _collect(rr, report, k, paths, tmp_path, table="C1"):
    """Turn `report` on and run its collector on a table of k-mer size k, as far as the host can take it."""
    if report == "read_support":
        rr.read_support_reset(True)
        rr.collect_read_support(table, types.SimpleNamespace(k=k), paths)
    elif report == "extract_reads":
        rr.extract_reads_reset(4, str(tmp_path))
        rr.collect_extract_reads(table, types.SimpleNamespace(k=k), paths)
    else:
        rr.bootstrap_reset(8, 3)
        rr.bootstrap_note_solve(begin=True, columns=[0], strains=["s"])
        (tmp_path / "StrainVote.report").write_text("header\n1\ts\tC1\t1.0\t2.0\n")
        rr.collect_bootstrap(table, str(tmp_path / "no_such_cluster"), str(tmp_path / "StrainVote.report"), k, paths)


@pytest.mark.parametrize("why", ["k", "resident"])
@pytest.mark.parametrize("report", ["read_support", "extract_reads", "bootstrap"])
def test_a_skip_says_its_line_once_and_nothing_is_written(rr, report, why, tmp_path, capsys, monkeypatch):
    from strainscan_amd import db
    if why == "k":                          # (the k-check comes before the reads are touched)
        k, paths, reason = 15, ["no such file"], K_TOO_SMALL
    else:
        monkeypatch.setattr(db, "RESIDENT_LIMIT_BYTES", 0)
        (tmp_path / "s.fq").write_text("@r\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\n" + "I" * 36 + "\n")
        k, paths, reason = 31, [str(tmp_path / "s.fq"), ""], NOT_RESIDENT
    state = getattr(rr, report.upper())
    _collect(rr, report, k, paths, tmp_path)
    assert capsys.readouterr().err == "%s: %s %s\n" % (report, reason, CLOSING[report])
    assert state["skipped"] == reason
    getattr(rr, "_%s_skip" % report)("another reason")                  # a second skip of the same report prints nothing ...
    _collect_again = {"read_support": lambda: rr.collect_read_support("C2", types.SimpleNamespace(k=k), paths),
                      "extract_reads": lambda: rr.collect_extract_reads("C2", types.SimpleNamespace(k=k), paths),
                      "bootstrap": lambda: rr.collect_bootstrap("C2", "no_such_cluster", str(tmp_path / "StrainVote.report"), k, paths)}
    _collect_again[report]()                                              # ... and neither does another table
    assert capsys.readouterr().err == "" and state["skipped"] == reason
    if report == "read_support":            # rows that would be written, were it not for the skip
        rr.READ_SUPPORT["rows"][None] = {"C1": ("C1", 1, 2, 3, [2] + [0] * 64)}
        assert rr.write_read_support(str(tmp_path)) is None
    elif report == "bootstrap":
        rr.BOOTSTRAP["rows"][None] = {"C1": dict(strains=["s"], coefs=np.ones((8, 1)), called=[(1, "s", "2.0", "1.0", 0)])}
        assert rr.write_bootstrap(str(tmp_path)) is None
    rr.write_all(str(tmp_path))
    assert sorted(set(os.listdir(tmp_path)) - {"s.fq", "StrainVote.report"}) == []


class _Reads:
    """a resident set that answers ReadSet.support with fixed numbers"""

    def support(self, kdb, n_bins):
        return np.array([7, 2, 1] + [0] * (n_bins - 3), np.uint64), 4

    def info(self):
        return {"n_records": 10}


def _strain_rows(cls, hits):
    return [("%s.1" % cls, "s", 5, 10, hits, [10 - hits, hits] + [0] * 63)]


def _bootstrap_rows(depth):
    return dict(strains=["s", "t"], coefs=np.arange(16, dtype=np.float64).reshape(8, 2) * depth,
                called=[(1, "s", str(depth), "0.5", 0), (2, "t", str(depth), "0.5", 1)])


def test_rows_go_to_the_scope_they_were_collected_under(rr, tmp_path, monkeypatch):
    from strainscan_amd import db
    monkeypatch.setattr(db, "resident_reads", lambda paths: _Reads())
    kdb = types.SimpleNamespace(k=31, info=lambda: {"n_distinct": 99})
    rr.read_support_reset(True)
    rr.by_strain_reset(True)
    rr.bootstrap_reset(8, 3)
    rr.extract_reads_reset(0, "base")       # (-x itself off: its collector needs the device; its directory is part of the scope)

    def collect(cls, hits, depth):          # the hook, and by hand what the device would have added under the same scope
        rr.table_scanned(cls, kdb, ["no such file"])
        rr.BY_STRAIN["rows"].setdefault(rr.SCOPE["label"], {})[cls] = _strain_rows(cls, hits)
        rr.BOOTSTRAP["rows"].setdefault(rr.SCOPE["label"], {})[cls] = _bootstrap_rows(depth)

    collect("C1", 1, 1.0)
    with rr.database_scope("a", "dir_a"):
        assert rr.SCOPE["label"] == "a" and rr.EXTRACT_READS["dir"] == "dir_a"
        collect("C2", 2, 2.0)
    assert rr.SCOPE["label"] is None and rr.EXTRACT_READS["dir"] == "base"
    with pytest.raises(KeyError):
        with rr.database_scope("b", "dir_b"):
            raise KeyError("the database failed")
    assert rr.SCOPE["label"] is None and rr.EXTRACT_READS["dir"] == "base"
    assert rr.BOOTSTRAP["order"] == {None: ["C1"], "a": ["C2"]}

    texts = {}
    for scope, cls in ((None, "C1"), ("a", "C2"), ("b", None)):
        d = tmp_path / str(scope)
        d.mkdir()
        rr.write_all(str(d), scope)
        texts[scope] = {f: (d / f).read_text() for f in sorted(os.listdir(d))}
    assert texts["b"] == {}
    files = [rr.READ_SUPPORT_FILE, rr.BOOTSTRAP_FILE, rr.STRAIN_SUPPORT_FILE]
    assert sorted(texts[None]) == sorted(texts["a"]) == sorted(files)
    assert texts[None][rr.READ_SUPPORT_FILE] == rr.read_support_text([("C1", 99, 10, 4, [7, 2, 1] + [0] * 62)])
    assert texts["a"][rr.READ_SUPPORT_FILE] == rr.read_support_text([("C2", 99, 10, 4, [7, 2, 1] + [0] * 62)])
    assert texts[None][rr.STRAIN_SUPPORT_FILE] == rr.strain_support_text(_strain_rows("C1", 1))
    assert texts["a"][rr.STRAIN_SUPPORT_FILE] == rr.strain_support_text(_strain_rows("C2", 2))
    for scope, cls, other in ((None, "C1", "C2"), ("a", "C2", "C1")):
        lines = texts[scope][rr.BOOTSTRAP_FILE].split("\n")[1:-1]
        assert [line.split("\t")[0] for line in lines] == [cls + ".1", cls + ".2"]
        assert all(other not in t for t in texts[scope].values())


def test_the_tree_in_the_scan_order_changes_nothing(rr, tmp_path):
    """table_scanned notes every table it is told of, the tree included; strain_bootstrap.tsv lists only tables with rows."""
    rr.bootstrap_reset(8, 3)
    rows = {"C7": _bootstrap_rows(1.0), "C3": _bootstrap_rows(2.0), "C5": _bootstrap_rows(3.0)}
    texts = []
    for tables in (["C7", "C3"], ["tree", "C7", "C3"]):
        rr.BOOTSTRAP.update(rows={None: dict(rows)}, order={})
        for t in tables:
            rr.table_scanned(t, object(), ["no such file"])              # (--read_support and -x are off: nothing is looked at)
        assert rr.BOOTSTRAP["order"] == {None: tables}
        d = tmp_path / str(len(tables))
        d.mkdir()
        texts.append(open(rr.write_bootstrap(str(d))).read())
    assert texts[0] == texts[1]
    assert [line.split("\t")[0] for line in texts[0].split("\n")[1:-1]] == ["C7.1", "C7.2", "C3.1", "C3.2", "C5.1", "C5.2"]
