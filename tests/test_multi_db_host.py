"""`strainscan-multi` without a GPU: the command line (labels, LABEL=DIR, the flags handed to every database), the refusals
that end in exit status 2 before any read is opened, databases.tsv, and the driver's bookkeeping of how each database ended
(the per-database work replaced by stand-ins)."""
import builtins
import os

import pytest

from strainscan_amd import multi_db


def _db(root, name, tree=True):
    d = os.path.join(str(root), name)
    os.makedirs(os.path.join(d, "Tree_database") if tree else d, exist_ok=True)
    return d


@pytest.fixture
def no_reads_opened(monkeypatch, tmp_path):
    """A read path that must never be opened (nor even stat'ed for its content)."""
    reads = str(tmp_path / "reads.fq")
    real_open = builtins.open

    def guarded(path, *a, **k):
        assert os.path.abspath(str(path)) != os.path.abspath(reads), "a read file was opened"
        return real_open(path, *a, **k)

    monkeypatch.setattr(builtins, "open", guarded)
    return reads


def test_parse_database_labels(tmp_path):
    d = _db(tmp_path, "ecoli")
    assert multi_db.parse_database(d) == ("ecoli", d)
    assert multi_db.parse_database(d + "/") == ("ecoli", d + "/")
    assert multi_db.parse_database("E=" + d) == ("E", d)
    assert multi_db.parse_database("two=parts=" + d) == ("two", "parts=" + d)
    odd = _db(tmp_path, "a=b")                             # an existing directory whose name holds '=' is a directory
    assert multi_db.parse_database(odd) == ("a=b", odd)
    for bad in ("=" + d, "x/y=" + d, "..=" + d, "lbl="):
        with pytest.raises(multi_db.Refused):
            multi_db.parse_database(bad)


def test_arguments_reach_every_database(tmp_path):
    a, b = _db(tmp_path, "akk"), _db(tmp_path, "sau")
    args, dbs, opts = multi_db.parse_args(["-i", "r1.fq", "-j", "r2.fq", "-d", a, "-d", "S=" + b, "-o", "OUT", "-k", "25",
                                           "-l", "1", "-b", "1", "-e", "1", "-s", "7"])
    assert dbs == [("akk", a), ("S", b)]
    assert (args.input_fq, args.input_fq2, args.out_dir) == ("r1.fq", "r2.fq", "OUT")
    assert opts == dict(ksize="25", ldep=1, sprob=1, pmode=0, emode=1, msn=7)      # -k stays text, as StrainScan.main passes it
    _, _, opts = multi_db.parse_args(["-i", "r.fq", "-d", a])
    assert opts == dict(ksize=31, ldep=0, sprob=0, pmode=0, emode=0, msn=40)


def _refused(argv, capsys):
    with pytest.raises(SystemExit) as e:
        multi_db.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_refusals_exit_2_before_any_read_is_opened(tmp_path, no_reads_opened, capsys):
    a, b = _db(tmp_path, "akk"), _db(tmp_path, "sau")
    out = str(tmp_path / "OUT")
    base = ["-i", no_reads_opened, "-o", out]
    assert "plasmid" in _refused(base + ["-d", a, "-p", "1"], capsys)
    assert "plasmid" in _refused(base + ["-d", a, "-p", "2"], capsys)
    assert "Tree_database" in _refused(base + ["-d", a, "-d", _db(tmp_path, "bare", tree=False)], capsys)
    assert "Tree_database" in _refused(base + ["-d", str(tmp_path / "missing")], capsys)
    os.symlink(a, str(tmp_path / "akk_link"))
    assert "same database" in _refused(base + ["-d", a, "-d", "X=" + str(tmp_path / "akk_link")], capsys)
    assert "same database" in _refused(base + ["-d", a, "-d", "Y=" + a + "/."], capsys)
    other = _db(tmp_path / "elsewhere", "akk")
    assert "labelled 'akk'" in _refused(base + ["-d", a, "-d", other], capsys)
    assert "labelled 'S'" in _refused(base + ["-d", "S=" + a, "-d", "S=" + b], capsys)
    assert "label" in _refused(base + ["-d", "x/y=" + a], capsys)
    assert not os.path.exists(out)                         # nothing was written either
    # ... and the same command line with the clash resolved by a label gets through the checks
    _, dbs, _ = multi_db.parse_args(base + ["-d", a, "-d", "A2=" + other])
    assert dbs == [("akk", a), ("A2", other)]


def test_databases_tsv_format(tmp_path):
    rows = [("akk", str(tmp_path / "akk"), "reports"), ("sau", "rel/sau", "no_clusters"),
            ("E", str(tmp_path / "e"), "single_cluster"), ("x", str(tmp_path / "x"), "error:IndexError")]
    p = str(tmp_path / multi_db.TSV)
    multi_db.write_table(p, rows)
    text = open(p).read()
    assert text.endswith("\n") and text.count("\n") == 4 and "\r" not in text
    lines = [ln.split("\t") for ln in text.splitlines()]
    assert [ln[0] for ln in lines] == ["akk", "sau", "E", "x"]
    assert [ln[2] for ln in lines] == ["reports", "no_clusters", "single_cluster", "error:IndexError"]
    assert all(len(ln) == 3 and os.path.isabs(ln[1]) for ln in lines)
    assert lines[1][1] == os.path.abspath("rel/sau")
    assert multi_db.read_table(p) == [tuple(ln) for ln in lines]


class _Pins:
    def __init__(self, specs, reads=None):
        _Pins.seen = (list(specs), reads)

    def __enter__(self):
        return [object() for _ in _Pins.seen[0]]

    def __exit__(self, *exc):
        return False


def test_driver_records_how_each_database_ended(tmp_path, monkeypatch, capsys):
    """Statuses in command-line order; an error is printed with its label and the databases after it still run; exit 1."""
    from strainscan_amd import StrainScan, Vote_Strain_L2_Lasso_new_sp, db as ssdb
    names = ["ok", "none", "single", "boom", "after"]
    dbs = {n: _db(tmp_path, n) for n in names}
    open(os.path.join(dbs["single"], "Memory_DB"), "w").close()
    reads = tmp_path / "r.fq"
    reads.write_text("@r\nACGT\n+\nIIII\n")
    calls = []

    def layer1(fq1, fq2, d, od, ldep, sprob):
        calls.append(("l1", os.path.basename(d), os.path.relpath(od, str(tmp_path / "OUT")), ldep, sprob))
        name = os.path.basename(d)
        if name == "none":
            raise SystemExit
        if name == "boom":
            raise IndexError("index 0 is out of bounds")
        return {1: {}}, 0

    def layer2(fq1, fq2, d, od, ksize, res, l2, msn, pmode, emode):
        calls.append(("l2", os.path.basename(d), ksize, msn, emode))
        if os.path.basename(d) == "single":
            raise SystemExit

    monkeypatch.setattr(ssdb, "pinned_images", _Pins)
    monkeypatch.setattr(ssdb, "scan_images", lambda imgs, paths: True)
    monkeypatch.setattr(StrainScan, "identify_layer1", layer1)
    monkeypatch.setattr(Vote_Strain_L2_Lasso_new_sp, "vote_strain_L2_batch", layer2)
    seeded = []
    out = str(tmp_path / "OUT")
    rows = multi_db.identify_databases((str(reads), ""), [dbs[n] for n in names], out, ksize="25", ldep=1, sprob=1, emode=1,
                                       msn=9, before_each=seeded.append)
    assert seeded == [0, 1, 2, 3, 4]
    assert [r[2] for r in rows] == ["reports", "no_clusters", "single_cluster", "error:IndexError", "reports"]
    assert [c[1] for c in calls if c[0] == "l1"] == names
    assert [c[1] for c in calls if c[0] == "l2"] == ["ok", "single", "after"]
    assert all(c[2] == c[1] and c[3:] == (1, 1) for c in calls if c[0] == "l1")
    assert all(c[2:] == ("25", 9, 1) for c in calls if c[0] == "l2")
    assert all(os.path.isdir(os.path.join(out, n)) for n in names)
    specs, rd = _Pins.seen
    assert rd == [str(reads)]
    assert specs == [(dbs[n] + "/Tree_database", n != "single") for n in names]      # Memory_DB: identify_low_mem's keys
    assert multi_db.read_table(os.path.join(out, multi_db.TSV)) == [(n, os.path.abspath(dbs[n]), st) for n, _, st in rows]
    err = capsys.readouterr().err
    assert "database boom" in err and "IndexError" in err and "Traceback" in err
    # the command: exit status 1 after an error, 0 when every database ended as a single run would
    from strainscan_amd import dist as sdist
    monkeypatch.setattr(sdist, "init_from_env", lambda: (0, 1))
    assert multi_db.main(["-i", str(reads), "-o", out] + sum((["-d", dbs[n]] for n in names), [])) == 1
    assert multi_db.main(["-i", str(reads), "-o", out, "-d", dbs["ok"], "-d", dbs["none"], "-d", dbs["single"]]) == 0
    assert [r[2] for r in multi_db.read_table(os.path.join(out, multi_db.TSV))] == ["reports", "no_clusters", "single_cluster"]
