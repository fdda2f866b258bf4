"""`strainscan --classify_reads M --extract_class LIST` / `strainscan-multi ...`: extracted/class_<item>_1.<ext> (and _2) hold exactly
the input's records, as original text in file order, whose flat bases the model (tests/class_model.py, tests/select_class_model.py)
puts in the item's clade -- a pair when either mate is there; `called` writes the clusters of final_report.txt; the numbers of each
stderr line are the row's reads_clade of read_classes.tsv; read_classes.tsv, stdout's result lines, -x's files and every other file
are what a run without the flag writes; without the flag nothing new runs; refusals end with status 2 before any input is opened;
where nothing can be extracted one line says why."""
import os
import re

import numpy as np
import pytest

from tests import bamio, class_model as cm, rs_model, select_class_model as scm, synth
from tests.test_bam_select_gpu import HDR
from tests.test_extract_cli_gpu import DIR, _files, _ok, _result_lines, _run, _with_cache, pair      # noqa: F401

pytestmark = pytest.mark.gpu

TSV = "read_classes.tsv"
NO_NODE = "99999"


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def tree_model(db_dir, k=31):
    """the tree's table and forest from the database's files alone -> dict(keys, row_node, parent, node_ids, num, leaves, parent_of)"""
    tdb = os.path.join(db_dir, "Tree_database")
    with open(os.path.join(tdb, "kmer.fa"), "rb") as f:
        kmers = [km.upper() for km in rs_model.kmers_of_fasta(f.read())]
    parent_of = {}
    with open(os.path.join(tdb, "tree_structure.txt")) as f:
        for ln in f:
            t = ln.rstrip("\n").split("\t")
            parent_of[int(t[0])] = None if t[1] == "N" else int(t[1])
    listed = sorted(int(f) for f in os.listdir(os.path.join(tdb, "kmers")) if f.isdigit())
    node_ids = sorted(set(listed) | set(parent_of))
    num = {nid: v for v, nid in enumerate(node_ids, 1)}
    owner = {}                                   # row -> the node that lists it, 0 once two different nodes do
    for nid in listed:
        with open(os.path.join(tdb, "kmers", str(nid))) as f:
            for r in set(map(int, f.readline().split())):
                owner[r] = num[nid] if owner.get(r, num[nid]) == num[nid] else 0
    parent = [0] * (len(node_ids) + 1)
    for nid in node_ids:
        if parent_of.get(nid) is not None:
            parent[num[nid]] = num[parent_of[nid]]
    return dict(keys=rs_model.encode_kmers(kmers, k), row_node=np.array([owner.get(r, 0) for r in range(len(kmers))], np.int64), parent=parent,
                node_ids=node_ids, num=num, leaves={nid for nid in parent_of if nid not in set(parent_of.values())},
                parent_of={nid: parent_of.get(nid) for nid in node_ids}, k=k)


def classes_of(tm, flat, m=1):
    return cm.classes_per_record(flat, tm["keys"], tm["row_node"], tm["parent"], tm["k"], m)


def clade_of(tm, item):
    return 0 if item == "unclassified" else tm["num"][int(item.lstrip("C"))]


def fastq_records(data):
    lines = data.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]


@pytest.fixture(scope="module")
def mix(mid_dbs):
    fq, data = mid_dbs["reads"]["M_mix"]
    return fq, synth.flat_bases_from_fastx(data), fastq_records(data)


@pytest.fixture(scope="module")
def tm(mid_dbs):
    return tree_model(mid_dbs["DB_M"]["db_dir"])


@pytest.fixture(scope="module")
def mix_classes(tm, mix):
    return classes_of(tm, mix[1])


@pytest.fixture(scope="module")
def items(tm, mix_classes):
    """the list of the main run: unclassified, called, the root, the leaf with the most reads of its own, an id that is no node"""
    root = next(nid for nid in tm["node_ids"] if tm["parent_of"][nid] is None and nid not in tm["leaves"])
    direct = np.bincount(mix_classes, minlength=len(tm["node_ids"]) + 1)
    leaf = max(tm["leaves"], key=lambda nid: int(direct[tm["num"][nid]]))
    assert direct[tm["num"][leaf]] > 0 and direct[0] > 0 and int(NO_NODE) not in tm["num"]
    return dict(root=str(root), leaf="C%d" % leaf, text="unclassified,called,%d,C%d,%s" % (root, leaf, NO_NODE))


@pytest.fixture(scope="module")
def runs(L, mid_dbs, mix, items, tmp_path_factory):
    """`strainscan` on DB_M with M_mix -> name: (err, stdout, stderr, out dir, select_class calls made, classify calls made)"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("xc_cli")

    def go():
        out = {}
        for name, extra in (("cls", ["--classify_reads", "1"]), ("flag", ["--classify_reads", "1", "--extract_class", items["text"]]),
                            ("x", ["--classify_reads", "1", "-x", "1"]),
                            ("xflag", ["--classify_reads", "1", "-x", "1", "--extract_class", items["text"]])):
            before, cbefore = L.select_class_calls(), L.classify_calls()
            od = str(root / name)
            err, _, text, errs = _run(StrainScan.main, ["-i", mix[0], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od] + extra)
            out[name] = (err, text, errs, od, L.select_class_calls() - before, L.classify_calls() - cbefore)
        return out
    return _with_cache(root, go)


def _called(od):
    """the clusters of final_report.txt"""
    with open(os.path.join(od, "final_report.txt")) as f:
        rows = [ln.split("\t") for ln in f.read().split("\n")[1:] if ln.strip()]
    return sorted({r[2] for r in rows if re.fullmatch(r"C\d+", r[2])})


def _stderr_lines(errs):
    out = {}
    for ln in errs.split("\n"):
        m = re.match(r"extract_class: (\S+)\tM=1\tselected on the device (\d+)\twritten (\d+)$", ln)
        if m:
            assert m.group(1) not in out, ln
            out[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    return out


def test_files_equal_the_model(runs, tm, mix, mix_classes, items):
    err, _, errs, od, calls, ccalls = runs["flag"]
    assert _ok(err), err
    called = _called(od)
    want_items = sorted({"unclassified", items["root"], items["leaf"]} | set(called))
    ex = os.path.join(od, DIR)
    assert sorted(os.listdir(ex)) == sorted("class_%s_1.fastq" % it for it in want_items)
    rows = {r[0]: r for r in (ln.split("\t") for ln in open(os.path.join(od, TSV)).read().split("\n")[1:-1])}
    lines = _stderr_lines(errs)
    assert sorted(lines) == want_items
    for it in want_items:
        c = clade_of(tm, it)
        want = b"".join(rec for rec, cls in zip(mix[2], mix_classes) if scm.in_clade(tm["parent"], int(cls), c))
        got = open(os.path.join(ex, "class_%s_1.fastq" % it), "rb").read()
        n = want.count(b"\n") // 4
        print(it, "clade", c, "records", n, "of", len(mix[2]), "stderr", lines[it])
        assert got == want, (it, len(got), len(want))
        assert lines[it] == (n, n) and n == int(rows[it.lstrip("C")][6])           # both numbers: the row's reads_clade
    assert 0 < lines["unclassified"][0] < len(mix[2]) and 0 < lines[items["leaf"]][0] < lines[items["root"]][0]
    # `called`: exactly the clusters of final_report.txt, at least one of them with reads
    assert called and any(lines[c][0] > 0 for c in called)
    # one device call where read_classes.tsv's numbers are collected, in place of the classify call; a second one for `called`
    # unless the listed leaf was the only cluster called
    assert ccalls == 0 and calls == (2 if set(called) - {items["leaf"]} else 1)
    # the id that is no node: one line, and the others were written
    no_node = [ln for ln in errs.split("\n") if ln.startswith("extract_class: %s " % NO_NODE)]
    assert len(no_node) == 1 and "names no node" in no_node[0]


def test_other_files_are_unchanged_and_flag_off_runs_nothing(runs):
    e0, t0, errs0, d0, calls0, ccalls0 = runs["cls"]
    e1, t1, _, d1, _, _ = runs["flag"]
    assert _ok(e0) and _ok(e1) and type(e0) is type(e1)
    assert calls0 == 0 and ccalls0 == 1 and "extract_class" not in errs0
    assert not os.path.exists(os.path.join(d0, DIR))
    a, b = _files(d0), {k: v for k, v in _files(d1).items() if DIR not in k.split(os.sep)}
    assert TSV in a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert _result_lines(t0) and _result_lines(t0) == _result_lines(t1)
    # with -x 1 beside it: -x's own files are those of the run without --extract_class
    ex, t2, _, d2, _, _ = runs["x"]
    exf, t3, _, d3, _, _ = runs["xflag"]
    assert _ok(ex) and _ok(exf)
    a, b = _files(d2), _files(d3)
    mine = [k for k in b if os.path.basename(k).startswith("class_")]
    assert mine and all(os.path.dirname(k) == DIR for k in mine) and not [k for k in a if os.path.basename(k).startswith("class_")]
    assert any(os.path.dirname(k) == DIR for k in a)
    rest = {k: v for k, v in b.items() if k not in mine}
    assert sorted(a) == sorted(rest) and all(a[k] == rest[k] for k in a)
    assert _result_lines(t2) == _result_lines(t3)
    assert {k: b[k] for k in mine} == {k: v for k, v in _files(d1).items() if k in mine}


def test_a_pair_is_written_when_either_mate_is_in_the_class(L, mid_dbs, tm, pair, items, tmp_path, monkeypatch):      # noqa: F811
    from strainscan_amd import StrainScan
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    od = str(tmp_path / "out")
    err, _, _, errs = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od,
                                             "--classify_reads", "1", "--extract_class", "unclassified,%s,%s" % (items["root"], items["leaf"])])
    assert _ok(err), err
    cls = [classes_of(tm, b"".join(s + b"\n" for _, s in pair["recs"][m])) for m in range(2)]
    assert len(cls[0]) == len(cls[1]) == len(pair["recs"][0])
    lines = _stderr_lines(errs)
    sizes = {}
    for it in ("unclassified", items["root"], items["leaf"]):
        c = clade_of(tm, it)
        keep = [i for i in range(len(cls[0])) if scm.in_clade(tm["parent"], int(cls[0][i]), c) or scm.in_clade(tm["parent"], int(cls[1][i]), c)]
        got = [open(os.path.join(od, DIR, "class_%s_%d.fastq" % (it, m + 1)), "rb").read() for m in range(2)]
        for m in range(2):
            assert got[m] == b"".join(pair["recs"][m][i][0] for i in keep), (it, m + 1)
        assert got[0].count(b"\n") == got[1].count(b"\n") == 4 * len(keep)                  # the two files stay in step
        assert lines[it][1] == 2 * len(keep) and lines[it][0] <= lines[it][1]
        sizes[it] = len(keep)
    print("pairs", len(cls[0]), sizes)
    # a pair can stand under two classes: one mate unclassified, the other in the root's clade
    both = sum(1 for i in range(len(cls[0])) if (cls[0][i] == 0) != (cls[1][i] == 0))
    assert both > 0 and sizes["unclassified"] + sizes[items["root"]] >= len(cls[0]) + both
    assert sorted(os.listdir(os.path.join(od, DIR))) == sorted("class_%s_%d.fastq" % (it, m) for it in sizes for m in (1, 2))


def test_refusals_end_with_status_2(L, mid_dbs, mix, tmp_path):
    from strainscan_amd import StrainScan, multi_db
    before = L.select_class_calls()
    base = ["-i", mix[0], "-d", mid_dbs["DB_M"]["db_dir"], "-o", str(tmp_path / "out")]
    for main, b in ((StrainScan.main, base), (multi_db.main, base + ["-d", "mem=" + mid_dbs["DB_Mmem"]["db_dir"]])):
        for extra in (["--extract_class", "unclassified"], ["--classify_reads", "1", "--extract_class", "C1,C1"],
                      ["--classify_reads", "1", "--extract_class", "foo"], ["--classify_reads", "1", "--extract_class", "1,,2"]):
            err, _, _, errs = _run(main, b + extra)
            assert isinstance(err, SystemExit) and err.code == 2, (extra, err)
            assert "extract_class" in errs
    assert not os.path.exists(str(tmp_path / "out")) and L.select_class_calls() == before


def test_multi_db_writes_one_directory_per_label(L, runs, mid_dbs, mix, items, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbm, dbmem = mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]
    base = ["-i", mix[0], "-d", dbm, "-d", "mem=" + dbmem, "--classify_reads", "1"]
    before = L.select_class_calls()
    e0, rc0, t0, _ = _run(multi_db.main, base + ["-o", str(tmp_path / "plain")])
    assert L.select_class_calls() == before
    e1, rc1, t1, errs = _run(multi_db.main, base + ["-o", str(tmp_path / "flag"), "--extract_class", items["text"]])
    assert e0 is None and e1 is None and rc0 == 0 and rc1 == 0
    a, b = _files(str(tmp_path / "plain")), _files(str(tmp_path / "flag"))
    # the two databases hold the same genomes and the same tree: each label's directory is the single run's, which the model has checked
    want = _files(os.path.join(runs["flag"][3], DIR))
    assert want
    for label in (os.path.basename(os.path.normpath(dbm)), "mem"):
        got = {os.path.relpath(k, os.path.join(label, DIR)): v for k, v in b.items() if k.startswith(os.path.join(label, DIR) + os.sep)}
        assert sorted(got) == sorted(want) and all(got[k] == want[k] for k in want), label
    assert not os.path.exists(str(tmp_path / "flag" / DIR))
    rep = {k: v for k, v in b.items() if DIR not in k.split(os.sep)}
    assert sorted(a) == sorted(rep) and all(a[k] == rep[k] for k in a)
    assert _result_lines(t0) == _result_lines(t1)
    assert len([ln for ln in errs.split("\n") if ln.startswith("extract_class: %s " % NO_NODE)]) == 2      # once per database


def test_a_bam_sample_is_classified_and_nothing_is_extracted(L, mid_dbs, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    names, seqs = bamio.fastq_reads(mid_dbs["reads"]["M_mix"][1])
    recs = bamio.sample_records(21, list(zip(names, seqs)), aligned=True, decoys=0.0, extras=False)
    (tmp_path / "S.bam").write_bytes(bamio.bgzf(HDR, recs, level=1))
    outs = {}
    for name, extra in (("cls", []), ("flag", ["--extract_class", "unclassified,called"])):
        before = L.select_class_calls()
        od = str(tmp_path / name)
        err, _, text, errs = _run(StrainScan.main, ["-i", str(tmp_path / "S.bam"), "-d", mid_dbs["DB_M"]["db_dir"], "-o", od, "--classify_reads", "1"]
                                  + extra)
        assert _ok(err), err
        outs[name] = (type(err), _result_lines(text), errs, _files(od))
        assert L.select_class_calls() == before
    lines = [ln for ln in outs["flag"][2].split("\n") if ln.startswith("extract_class:")]
    assert len(lines) == 1 and "BAM" in lines[0] and lines[0].endswith(" and nothing was extracted"), lines
    assert "extract_class" not in outs["cls"][2]
    assert TSV in outs["flag"][3] and not [k for k in outs["flag"][3] if "class_" in k or DIR in k.split(os.sep)]
    assert outs["flag"][0] is outs["cls"][0] and outs["flag"][1] == outs["cls"][1] and outs["flag"][3] == outs["cls"][3]
