"""`strainscan --classify_strains M` with --extract_strains, on the mid-size database and its M_mix sample (two strains of C7, three
of C19, one of C23 and a singleton: the reports the run writes show a cluster with two called strains).

strain_classes.tsv and strain_sets.tsv equal the model (tests/strain_set_model.py) computed from the StrainVote.report files the run
wrote, each cluster's all_strains_re.npz / id2strain_re.pkl / all_kmer.fasta and the sample's sequences; every
extracted/strain_C<id>.<n>_*.fastq holds the model's pairs as whole FASTQ records in file order, for `unique` and for `compatible`;
with --pairs the files are the model's on the joined fragments and a cluster's reads_share column sums to the pairs; every other
output file and the result lines of stdout are those of the run without the flags; without the flags the new calls do not run; a
bad value of either flag, and --extract_strains alone, end with exit status 2."""
import os
import pickle

import numpy as np
import pytest

from tests import rs_model, strain_set_model as sm
from tests.test_extract_cli_gpu import DIR, _files, _ok, _result_lines, _run, _with_cache, pair      # noqa: F401

pytestmark = pytest.mark.gpu

M = 4
CLASSES, SETS = "strain_classes.tsv", "strain_sets.tsv"


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _is_new_file(rel):
    parts = rel.split(os.sep)
    return parts[-1] in (CLASSES, SETS) or (DIR in parts and parts[-1].startswith("strain_"))


@pytest.fixture(scope="module")
def runs(L, mid_dbs, pair, tmp_path_factory):
    """`strainscan --read_support` on DB_M with the pair: plain, with --classify_strains and each --extract_strains, and with --pairs
    -> name: (err, stdout, stderr, out dir, classify_strains calls made, select_strains calls made)"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("cs_cli")
    flags = ["--classify_strains", str(M)]

    def go():
        out = {}
        for name, extra in (("plain", []), ("unique", flags + ["--extract_strains", "unique"]),
                            ("compatible", flags + ["--extract_strains", "compatible"]), ("pairs", flags + ["--extract_strains", "unique", "--pairs"])):
            before = L.classify_strains_calls(), L.select_strains_calls()
            od = str(root / name)
            err, _, text, errs = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od,
                                                        "--read_support"] + extra)
            out[name] = (err, text, errs, od, L.classify_strains_calls() - before[0], L.select_strains_calls() - before[1])
        return out
    return _with_cache(root, go)


def _called(report):
    rows = [ln.split("\t") for ln in open(report).read().split("\n")[1:] if ln.strip()]
    return [(int(r[0]), r[1]) for r in rows]


_MODEL = {}


def _model(db_dir, out_dir, pair, fragments):
    """-> (classes text, sets text, {cluster: (called, result, [sets of the records of each text])}) from the reports in out_dir;
    fragments: the records are the pairs joined with an N, else the reads of both files"""
    if (out_dir, fragments) in _MODEL:
        return _MODEL[out_dir, fragments]
    import scipy.sparse as sp
    rs_rows = [ln.split("\t")[0] for ln in open(os.path.join(out_dir, "read_support.tsv")).read().split("\n")[1:] if ln]
    if fragments:
        texts = [b"".join(a[1] + b"N" + b[1] + b"\n" for a, b in zip(*pair["recs"]))]
    else:
        texts = [b"".join(s + b"\n" for _, s in pair["recs"][m]) for m in range(2)]
    clusters, detail = [], {}
    for cls in [t for t in rs_rows if t != "tree"]:                 # clusters in the order they were scanned
        report = os.path.join(out_dir, cls, "StrainVote.report")
        if not os.path.exists(report):
            continue
        called = _called(report)
        assert 1 <= len(called) <= 16
        cdir = os.path.join(db_dir, "Kmer_Sets_L2", "Kmer_Sets", cls)
        with open(os.path.join(cdir, "id2strain_re.pkl"), "rb") as f:
            sid = pickle.load(f)
        col_of = {name: c for c, name in (sid.items() if isinstance(sid, dict) else enumerate(sid))}
        dense = np.asarray(sp.load_npz(os.path.join(cdir, "all_strains_re.npz")).todense())
        masks = np.zeros(dense.shape[0], np.uint16)
        for j, (_, name) in enumerate(called):
            masks |= ((dense[:, col_of[name]] != 0).astype(np.uint16) << np.uint16(j))
        with open(os.path.join(cdir, "all_kmer.fasta"), "rb") as f:
            kmers = [km.upper() for km in rs_model.kmers_of_fasta(f.read())]
        assert len(kmers) == dense.shape[0]
        keys = rs_model.encode_kmers(kmers, 31)
        parts = [sm.classify_strains_model(t, keys, masks, len(called), 31, M) for t in texts]
        total = dict(parts[0])
        for p in parts[1:]:
            for key in ("unique", "tied", "strain_hits", "set_reads"):
                total[key] = total[key] + p[key]
        clusters.append((cls, [name for _, name in called], total))
        detail[cls] = (called, total, [p["sets"] for p in parts])
    # (the model numbers the strains 1..L; the command names them by the report's column 1, which the run's reports number 1..L)
    assert all([n for n, _ in c[0]] == list(range(1, len(c[0]) + 1)) for c in detail.values())
    _MODEL[out_dir, fragments] = (sm.classes_text(clusters), sm.sets_text(clusters), detail)
    return _MODEL[out_dir, fragments]


def _check_files(od, detail, pair, how, fragments):
    """every extracted/strain_* file against the model -> {name: pairs written}"""
    ex = os.path.join(od, DIR)
    want_names = sorted("strain_%s.%d_%d.fastq" % (cls, n, m) for cls, (called, _, _) in detail.items() for n, _ in called for m in (1, 2))
    assert sorted(f for f in os.listdir(ex) if f.startswith("strain_")) == want_names
    sizes = {}
    for cls, (called, _, sets) in detail.items():
        for j, (n, _) in enumerate(called):
            hit = [(s == (1 << j)) if how == "unique" else ((s >> j) & 1) != 0 for s in (np.asarray(x, np.int64) for x in sets)]
            keep = np.nonzero(hit[0] if fragments else (hit[0] | hit[1]))[0]      # (-x's rule: a pair when either mate is selected)
            for m in range(2):
                got = open(os.path.join(ex, "strain_%s.%d_%d.fastq" % (cls, n, m + 1)), "rb").read()
                want = b"".join(pair["recs"][m][i][0] for i in keep)
                assert got == want, (cls, n, m + 1, len(got), len(want))
            sizes["%s.%d" % (cls, n)] = int(keep.size)
    return sizes


@pytest.mark.parametrize("how", ["unique", "compatible"])
def test_reports_and_strain_files_are_the_models(runs, mid_dbs, pair, how):
    err, _, errs, od, calls, scalls = runs[how]
    assert _ok(err), err
    want_classes, want_sets, detail = _model(mid_dbs["DB_M"]["db_dir"], od, pair, False)
    print({c: v[0] for c, v in detail.items()})
    assert any(len(v[0]) == 2 for v in detail.values()), detail.keys()      # two strains called in one cluster
    got_classes, got_sets = open(os.path.join(od, CLASSES)).read(), open(os.path.join(od, SETS)).read()
    print(got_classes)
    print(got_sets)
    assert got_classes == want_classes and got_sets == want_sets
    assert got_classes.split("\n")[0] == "table\tstrain\tkmers\thits\treads_unique\treads_tied\treads_share"
    assert got_sets.split("\n")[0] == "table\tset\tstrains\treads"
    n_reads = 2 * len(pair["recs"][0])
    for cls, (called, r, _) in detail.items():
        share = [float(ln.split("\t")[6]) for ln in got_classes.split("\n")[1:] if ln and ln.split("\t")[0].split(".")[0] == cls]
        assert len(share) == len(called) + 1 and abs(sum(share) - n_reads) < 0.01 * len(share), (cls, share)
        if len(called) >= 2:
            assert int(r["tied"][0]) > 0 and int(r["unique"][1:].sum()) > 0 and int(r["unique"][0]) > 0, cls      # every kind is there
    sizes = _check_files(od, detail, pair, how, False)
    print(how, sizes, "of", len(pair["recs"][0]))
    two = [c for c, v in detail.items() if len(v[0]) == 2][0]
    assert all(0 < sizes["%s.%d" % (two, n)] < len(pair["recs"][0]) for n, _ in detail[two][0]), sizes
    # one classification and one selection per cluster with a report; one line per cluster on stderr
    assert calls == len(detail) and scalls == len(detail)
    lines = [ln for ln in errs.split("\n") if ln.startswith("classify_strains:")]
    assert sorted(ln.split("\t")[0].split(" ")[1] for ln in lines) == sorted(detail), lines
    for ln in lines:
        cls = ln.split("\t")[0].split(" ")[1]
        r = detail[cls][1]
        assert ln.split("\t")[1:] == ["M=%d" % M, "records %d" % n_reads, "unique %d" % int(r["unique"][1:].sum()), "tied %d" % int(r["tied"][0]),
                                      "unassigned %d" % int(r["unique"][0]), "sets %d" % int((r["set_reads"][1:] > 0).sum())], ln


def test_compatible_holds_unique(runs):
    a, b = _files(os.path.join(runs["unique"][3], DIR)), _files(os.path.join(runs["compatible"][3], DIR))
    new = [k for k in a if k.startswith("strain_")]
    assert new and all(len(a[k]) <= len(b[k]) for k in new) and any(len(a[k]) < len(b[k]) for k in new)
    for name in (CLASSES, SETS):
        assert open(os.path.join(runs["unique"][3], name)).read() == open(os.path.join(runs["compatible"][3], name)).read()


def test_pairs_are_assigned_as_fragments(runs, mid_dbs, pair):
    err, _, errs, od, calls, _ = runs["pairs"]
    assert _ok(err), err
    want_classes, want_sets, detail = _model(mid_dbs["DB_M"]["db_dir"], od, pair, True)
    got_classes = open(os.path.join(od, CLASSES)).read()
    assert got_classes == want_classes and open(os.path.join(od, SETS)).read() == want_sets
    n_pairs = len(pair["recs"][0])
    for cls, (called, _, _) in detail.items():
        share = [float(ln.split("\t")[6]) for ln in got_classes.split("\n")[1:] if ln and ln.split("\t")[0].split(".")[0] == cls]
        assert len(share) == len(called) + 1 and abs(sum(share) - n_pairs) < 0.01 * len(share), (cls, share)
    assert got_classes != open(os.path.join(runs["unique"][3], CLASSES)).read()
    _check_files(od, detail, pair, "unique", True)
    assert calls == len(detail)


def test_other_outputs_are_unchanged_and_flag_off_runs_nothing(runs):
    e0, t0, errs0, d0, calls0, scalls0 = runs["plain"]
    assert _ok(e0) and calls0 == 0 and scalls0 == 0
    assert not [ln for ln in errs0.split("\n") if ln.startswith(("classify_strains:", "extract_strains:"))]
    a = _files(d0)
    assert not [k for k in a if _is_new_file(k)] and "read_support.tsv" in a
    for name in ("unique", "compatible"):
        e1, t1, _, d1, calls1, scalls1 = runs[name]
        assert _ok(e1) and type(e0) is type(e1) and calls1 > 0 and scalls1 > 0
        b = {k: v for k, v in _files(d1).items() if not _is_new_file(k)}
        assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a), name
        assert t0 == t1 or _result_lines(t0) == _result_lines(t1)
    assert _result_lines(t0)


@pytest.mark.parametrize("extra", [["--classify_strains", "0"], ["--classify_strains", "-1"], ["--classify_strains", "two"],
                                   ["--classify_strains", "1.5"], ["--classify_strains", "2", "--extract_strains", "all"],
                                   ["--classify_strains", "2", "--extract_strains", ""], ["--extract_strains", "unique"]])
def test_bad_values_end_with_status_2(L, mid_dbs, pair, tmp_path, extra):
    from strainscan_amd import StrainScan, multi_db
    before = L.classify_strains_calls()
    for main, d in ((StrainScan.main, ["-d", mid_dbs["DB_M"]["db_dir"]]), (multi_db.main, ["-d", mid_dbs["DB_M"]["db_dir"]])):
        od = str(tmp_path / main.__module__.split(".")[-1])
        err, _, _, errs = _run(main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-o", od] + d + extra)
        assert isinstance(err, SystemExit) and err.code == 2, (err, errs[-500:])
        assert not os.path.exists(od)                                  # before any input is opened, before anything is made
    assert L.classify_strains_calls() == before


def test_pairs_may_go_with_classify_strains_alone():
    import argparse
    from strainscan_amd import StrainScan
    ap = argparse.ArgumentParser()
    StrainScan.add_arguments(ap)
    args = ap.parse_args(["-i", "a.fq", "-j", "b.fq", "-d", "db", "--pairs", "--classify_strains", "3"])
    StrainScan.refuse_pairs_alone(ap, args)                            # (no error)
    assert args.classify_strains == 3 and args.extract_strains is None
    with pytest.raises(SystemExit) as e:
        StrainScan.refuse_pairs_alone(ap, ap.parse_args(["-i", "a.fq", "-j", "b.fq", "-d", "db", "--pairs"]))
    assert e.value.code == 2


def test_multi_db_writes_under_each_label(L, runs, mid_dbs, pair, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbm, dbmem = mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]
    od = str(tmp_path / "flag")
    e1, rc1, _, _ = _run(multi_db.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", dbm, "-d", "mem=" + dbmem, "-o", od,
                                         "--read_support", "--classify_strains", str(M), "--extract_strains", "unique"])
    assert e1 is None and rc1 == 0
    # the two databases hold the same genomes: each label's files are the single run's, which the model has checked
    want = {k: v for k, v in _files(runs["unique"][3]).items() if _is_new_file(k)}
    assert CLASSES in want and SETS in want and len(want) >= 6
    got_all = _files(od)
    for label in (os.path.basename(os.path.normpath(dbm)), "mem"):
        got = {os.path.relpath(k, label): v for k, v in got_all.items() if k.startswith(label + os.sep) and _is_new_file(k)}
        assert sorted(got) == sorted(want) and all(got[k] == want[k] for k in want), label
    assert not os.path.exists(os.path.join(od, CLASSES)) and not os.path.exists(os.path.join(od, DIR))


def test_sample_not_resident(L, runs, mid_dbs, pair, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    from strainscan_amd import db as ssdb
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    monkeypatch.setattr(ssdb, "RESIDENT_LIMIT_BYTES", 0)
    before = L.classify_strains_calls()
    od = str(tmp_path / "out")
    err, _, text, errs = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od,
                                                "--classify_strains", str(M), "--extract_strains", "unique"])
    lines = [ln for ln in errs.split("\n") if ln.startswith("classify_strains:")]
    assert len(lines) == 1 and "resident on the device" in lines[0], lines
    e0 = runs["plain"][0]
    assert _ok(err) and type(err) is type(e0) and L.classify_strains_calls() == before
    assert not [k for k in _files(od) if _is_new_file(k)]
    assert _result_lines(runs["plain"][1]) == _result_lines(text)
