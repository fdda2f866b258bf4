"""`strainscan --divergence M` on the mid-size database and its M_mix sample (the inputs of tests/test_classify_strains_cli_gpu.py).

strain_divergence.tsv equals the model (tests/gap_model.py) computed from the StrainVote.report files the run wrote, each cluster's
all_strains_re.npz / id2strain_re.pkl / all_kmer.fasta and the sample's sequences; with --pairs it equals the model on the joined
fragments; every other output file and the result lines of stdout are those of the run without the flag; without the flag the new
call does not run; the file appears under each label of strainscan-multi; a sample that is not resident gets one line and no file."""
import os
import pickle

import numpy as np
import pytest

from tests import gap_model as gm, rs_model
from tests.test_extract_cli_gpu import _files, _ok, _result_lines, _run, _with_cache, pair      # noqa: F401

pytestmark = pytest.mark.gpu

M = 4
FILE = "strain_divergence.tsv"


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def runs(L, mid_dbs, pair, tmp_path_factory):
    """`strainscan --read_support` on DB_M with the pair: plain, with --divergence, and with --pairs
    -> name: (err, stdout, stderr, out dir, gaps calls made)"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("div_cli")

    def go():
        out = {}
        for name, extra in (("plain", []), ("flag", ["--divergence", str(M)]), ("pairs", ["--divergence", str(M), "--pairs"])):
            before = L.gaps_calls()
            od = str(root / name)
            err, _, text, errs = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od,
                                                        "--read_support"] + extra)
            out[name] = (err, text, errs, od, L.gaps_calls() - before)
        return out
    return _with_cache(root, go)


def _called(report):
    rows = [ln.split("\t") for ln in open(report).read().split("\n")[1:] if ln.strip()]
    return [(int(r[0]), r[1]) for r in rows]


def _model(db_dir, out_dir, pair, fragments):
    """-> (the file's text, [(cluster, report numbers, totals)]) from the reports in out_dir; fragments: the records are the pairs
    joined with an N, else the reads of both files"""
    import scipy.sparse as sp
    rs_rows = [ln.split("\t")[0] for ln in open(os.path.join(out_dir, "read_support.tsv")).read().split("\n")[1:] if ln]
    if fragments:
        text = b"".join(a[1] + b"N" + b[1] + b"\n" for a, b in zip(*pair["recs"]))
    else:
        text = b"".join(s + b"\n" for m in range(2) for _, s in pair["recs"][m])
    clusters = []
    for cls in [t for t in rs_rows if t != "tree"]:                 # clusters in the order they were scanned
        report = os.path.join(out_dir, cls, "StrainVote.report")
        if not os.path.exists(report):
            continue
        called = _called(report)
        cdir = os.path.join(db_dir, "Kmer_Sets_L2", "Kmer_Sets", cls)
        with open(os.path.join(cdir, "id2strain_re.pkl"), "rb") as f:
            sid = pickle.load(f)
        col_of = {name: c for c, name in (sid.items() if isinstance(sid, dict) else enumerate(sid))}
        dense = np.asarray(sp.load_npz(os.path.join(cdir, "all_strains_re.npz")).todense())
        row_called = np.zeros(dense.shape[0], bool)
        for _, name in called:
            row_called |= dense[:, col_of[name]] != 0
        with open(os.path.join(cdir, "all_kmer.fasta"), "rb") as f:
            kmers = [km.upper() for km in rs_model.kmers_of_fasta(f.read())]
        assert len(kmers) == dense.shape[0]
        tot, _ = gm.gaps_model(text, rs_model.encode_kmers(kmers, 31), row_called, 31, M)
        clusters.append((cls, [n for n, _ in called], tot))
    return gm.report_text(clusters), clusters


def _check(run, db_dir, pair, fragments):
    err, _, errs, od, calls = run
    assert _ok(err), err
    want, clusters = _model(db_dir, od, pair, fragments)
    got = open(os.path.join(od, FILE)).read()
    print(got)
    assert got == want
    assert got.split("\n")[0].split("\t") == list(gm.COLUMNS)
    assert len(clusters) >= 2 and any(len(c[1]) == 2 for c in clusters)      # a cluster with two called strains
    assert any(c[2]["kmers_called"] < c[2]["kmers"] for c in clusters) and all(c[2]["assessed"] > 0 for c in clusters)
    # one call per cluster with a report; one line per cluster on stderr
    assert calls == len(clusters)
    lines = [ln for ln in errs.split("\n") if ln.startswith("divergence:")]
    n_rec = len(pair["recs"][0]) * (1 if fragments else 2)
    assert sorted(lines) == sorted("divergence: %s\tM=%d\trecords %d\tassessed %d\tsites %d\tdetectable %d" %
                                   (cls, M, n_rec, t["assessed"], t["sites"], t["detectable"]) for cls, _, t in clusters), lines
    return got, clusters


def test_file_is_the_model(runs, mid_dbs, pair):
    _check(runs["flag"], mid_dbs["DB_M"]["db_dir"], pair, False)


def test_pairs_are_walked_as_fragments(runs, mid_dbs, pair):
    got, clusters = _check(runs["pairs"], mid_dbs["DB_M"]["db_dir"], pair, True)
    plain = open(os.path.join(runs["flag"][3], FILE)).read()
    assert got != plain
    # the tables, their called strains and their k-mers do not depend on --pairs
    assert [ln.split("\t")[:4] for ln in got.split("\n")] == [ln.split("\t")[:4] for ln in plain.split("\n")]


def test_other_outputs_are_unchanged_and_flag_off_runs_nothing(runs):
    e0, t0, errs0, d0, calls0 = runs["plain"]
    assert _ok(e0) and calls0 == 0
    assert not [ln for ln in errs0.split("\n") if ln.startswith("divergence:")]
    a = _files(d0)
    assert FILE not in a and "read_support.tsv" in a
    for name in ("flag", "pairs"):
        e1, t1, _, d1, calls1 = runs[name]
        assert _ok(e1) and type(e0) is type(e1) and calls1 > 0
        b = {k: v for k, v in _files(d1).items() if k != FILE}
        assert sorted(a) == sorted(b), name
        if name == "flag":                                             # (--pairs changes read_support.tsv's rows by itself)
            assert all(a[k] == b[k] for k in a)
        assert t0 == t1 or _result_lines(t0) == _result_lines(t1)
    assert _result_lines(t0)


def test_multi_db_writes_under_each_label(L, runs, mid_dbs, pair, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbm, dbmem = mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]
    od = str(tmp_path / "flag")
    e1, rc1, _, _ = _run(multi_db.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", dbm, "-d", "mem=" + dbmem, "-o", od,
                                         "--read_support", "--divergence", str(M)])
    assert e1 is None and rc1 == 0
    # the two databases hold the same genomes: each label's file is the single run's, which the model has checked
    want = open(os.path.join(runs["flag"][3], FILE), "rb").read()
    got_all = _files(od)
    for label in (os.path.basename(os.path.normpath(dbm)), "mem"):
        assert got_all[os.path.join(label, FILE)] == want, label
    assert not os.path.exists(os.path.join(od, FILE))


def test_sample_not_resident(L, runs, mid_dbs, pair, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    from strainscan_amd import db as ssdb
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    monkeypatch.setattr(ssdb, "RESIDENT_LIMIT_BYTES", 0)
    before = L.gaps_calls()
    od = str(tmp_path / "out")
    err, _, text, errs = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od,
                                                "--divergence", str(M)])
    lines = [ln for ln in errs.split("\n") if ln.startswith("divergence:")]
    assert len(lines) == 1 and "resident on the device" in lines[0], lines
    e0 = runs["plain"][0]
    assert _ok(err) and type(err) is type(e0) and L.gaps_calls() == before
    assert FILE not in _files(od)
    assert _result_lines(runs["plain"][1]) == _result_lines(text)
