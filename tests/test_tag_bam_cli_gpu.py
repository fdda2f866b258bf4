"""`strainscan -i S.bam --classify_reads M --tag_bam` / `strainscan-multi ...`: OUT/classified_<i>.bam is the input written back --
its header, and every record in file order with 14 bytes appended to each kept one -- the histogram of its sn tags is the
reads_direct column of read_classes.tsv, the names under a node's clade are those --extract_class writes from the same reads as
FASTQ, with --pairs both mates carry the fragment's class; stdout and every other file are what the run without the flag writes,
and without the flag nothing new runs; where no file can be written one line says why."""
import gzip
import os
import re

import pytest

from tests import bam_pairs_model, bam_tag_model, bamio, select_class_model as scm
from tests.test_bam_pairs_cli_gpu import sample      # noqa: F401
from tests.test_bam_select_gpu import HDR
from tests.test_extract_class_cli_gpu import TSV
from tests.test_extract_cli_gpu import DIR, _files, _ok, _result_lines, _run, _with_cache, pair      # noqa: F401
from tests.test_pairs_cli_gpu import sample as fq_sample, tm      # noqa: F401

pytestmark = pytest.mark.gpu

OUT = "classified_1.bam"


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def single(mid_dbs, tmp_path_factory):
    """the M_mix reads as one BAM with unique names (half of the records 0x10, two aux fields on every record, a few records
    without bases), and the same reads -- upper case, as a BAM stores them -- as FASTQ"""
    root = tmp_path_factory.mktemp("tag_bam_sample")
    names, seqs = bamio.fastq_reads(mid_dbs["reads"]["M_mix"][1])
    assert len(set(names)) == len(names)
    recs = bamio.sample_records(21, list(zip(names, seqs)), aligned=True, decoys=0.0, extras=True)
    bam, fq = root / "S.bam", root / "S.fq"
    bam.write_bytes(bamio.bgzf(HDR, recs, level=1))
    fq.write_bytes(bamio.fastq(seqs, names))
    return dict(bam=str(bam), fq=str(fq), stream=HDR + b"".join(recs), names=names)


@pytest.fixture(scope="module")
def runs(L, mid_dbs, single, tmp_path_factory):
    """name -> (err, stdout, stderr, out dir, bam_tag calls made)"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("tag_bam_cli")
    db = mid_dbs["DB_M"]["db_dir"]

    def go():
        out = {}
        for name, extra in (("off", []), ("on", ["--tag_bam"])):
            c0 = L.bam_tag_calls()
            od = str(root / name)
            err, _, text, errs = _run(StrainScan.main, ["-i", single["bam"], "-d", db, "-o", od, "--classify_reads", "1"] + extra)
            out[name] = (err, text, errs, od, L.bam_tag_calls() - c0)
        return out
    return _with_cache(root, go)


def _direct(od):
    """read_classes.tsv -> {node id or -1: reads_direct}"""
    rows = [ln.split("\t") for ln in open(os.path.join(od, TSV)).read().split("\n")[1:-1]]
    return {(-1 if r[0] == "unclassified" else int(r[0])): int(r[5]) for r in rows}


def _tag_lines(errs):
    return [ln for ln in errs.split("\n") if ln.startswith("tag_bam:")]


def _histogram(values):
    h = {}
    for v in values:
        h[v] = h.get(v, 0) + 1
    return h


def test_tagged_bam_is_the_input_with_the_classes_of_read_classes(runs, single):
    err, _, errs, od, calls = runs["on"]
    assert _ok(err), err
    assert calls == 1
    data = open(os.path.join(od, OUT), "rb").read()
    stream = gzip.decompress(data)
    assert data.endswith(bamio.EOF) and stream[:len(HDR)] == HDR == single["stream"][:len(HDR)]
    # the records, the last 14 bytes of each kept one stripped and its block_size put back, are the input's
    body, back, p = stream[len(HDR):], [], 0
    src = bam_pairs_model.walk(single["stream"])
    for r in src:
        k = bam_pairs_model.kept(r)
        size = r["size"] + (14 if k else 0)
        rec = body[p:p + size]
        back.append((rec[:4] if not k else (int.from_bytes(rec[:4], "little") - 14).to_bytes(4, "little")) + rec[4:r["size"]])
        p += size
    assert p == len(body) and b"".join(back) == single["stream"][len(HDR):]
    assert bamio.decode(data) == bamio.decode(single["stream"])
    tags = bam_tag_model.read_tags(body)
    kept = [t for t, r in zip(tags, src) if bam_pairs_model.kept(r)]
    assert all(t[2] is not None and t[3] is not None for t in kept) and len(kept) == len(single["names"])
    want = _direct(od)
    hist = _histogram(t[2] for t in kept)
    print("sn histogram", sorted(hist.items()))
    assert hist == {k: v for k, v in want.items() if v} and len(hist) > 3 and hist[-1] > 0
    assert all(t[3] >= 1 for t in kept if t[2] != -1) and any(t[3] > 1 for t in kept)
    lines = _tag_lines(errs)
    assert len(lines) == 1
    m = re.fullmatch(r"tag_bam: (\S+)\tM=1\trecords (\d+)\ttagged (\d+)\tclassified (\d+)\tfragments (\d+)\tfrom a tie (\d+)", lines[0])
    assert m and m.group(1) == os.path.join(od, OUT)
    rec, tagged, classified, frags, ties = (int(x) for x in m.groups()[1:])
    assert rec == len(src) and tagged == frags == len(kept) and tagged - classified == want[-1]
    cl = [ln for ln in errs.split("\n") if ln.startswith("classify_reads:")]
    assert len(cl) == 1 and cl[0].endswith("from a tie %d" % ties)


def test_other_files_are_unchanged_and_flag_off_runs_nothing(runs):
    e0, t0, errs0, d0, calls0 = runs["off"]
    e1, t1, _, d1, _ = runs["on"]
    assert _ok(e0) and _ok(e1) and type(e0) is type(e1)
    assert calls0 == 0 and "tag_bam" not in errs0
    a, b = _files(d0), _files(d1)
    assert OUT not in a and sorted(list(a) + [OUT]) == sorted(b)
    assert TSV in a and all(a[k] == b[k] for k in a)
    assert _result_lines(t0) and _result_lines(t0) == _result_lines(t1)


def test_names_under_a_clade_are_those_extract_class_writes(L, runs, mid_dbs, single, tm, tmp_path, monkeypatch):      # noqa: F811
    """the same reads as FASTQ with --extract_class C<id>: single-end with unique names, so names carry the comparison"""
    from strainscan_amd import StrainScan
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    od = runs["on"][3]
    direct = _direct(od)
    leaf = max(tm["leaves"], key=lambda nid: direct.get(nid, 0))
    root = next(nid for nid in tm["node_ids"] if tm["parent_of"][nid] is None and nid not in tm["leaves"])
    assert direct[leaf] > 0
    fo = str(tmp_path / "fq")
    err, _, _, errs = _run(StrainScan.main, ["-i", single["fq"], "-d", mid_dbs["DB_M"]["db_dir"], "-o", fo, "--classify_reads", "1",
                                             "--extract_class", "C%d,%d,unclassified" % (leaf, root)])
    assert _ok(err), err
    assert _direct(fo) == direct                                          # the BAM holds the reads of the FASTQ
    tags = bam_tag_model.read_tags(gzip.decompress(open(os.path.join(od, OUT), "rb").read())[len(HDR):])
    for item, clade in (("C%d" % leaf, tm["num"][leaf]), (str(root), tm["num"][root]), ("unclassified", 0)):
        fq = open(os.path.join(fo, DIR, "class_%s_1.fastq" % item), "rb").read().split(b"\n")
        want = sorted(ln[1:].split()[0] for ln in fq[0:-1:4])
        got = sorted(name for _, name, sn, _ in tags if sn is not None and scm.in_clade(tm["parent"], 0 if sn == -1 else tm["num"][sn], clade))
        assert got == want and len(got) > 0, item


def test_pairs_tag_both_mates_with_the_fragments_class(L, mid_dbs, sample, tmp_path, monkeypatch):      # noqa: F811
    from strainscan_amd import StrainScan
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    od = str(tmp_path / "out")
    c0 = L.bam_tag_calls()
    err, _, _, errs = _run(StrainScan.main, ["-i", sample["bam"], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od, "--classify_reads", "1", "--tag_bam",
                                             "--pairs"])
    assert _ok(err), err
    assert L.bam_tag_calls() == c0 + 1
    stream = gzip.decompress(open(os.path.join(od, OUT), "rb").read())
    tags = bam_tag_model.read_tags(stream[len(HDR):])
    src = bam_pairs_model.walk(sample["stream"])
    assert len(tags) == len(src)
    by_name = {}
    for (flag, name, sn, sc), r in zip(tags, src):
        assert (sn is not None) == bam_pairs_model.kept(r)
        if sn is not None:
            by_name.setdefault(name, []).append((sn, sc))
    assert len(by_name) == sample["n"] and all(len(set(v)) == 1 for v in by_name.values())      # mates share their tags
    assert sum(1 for v in by_name.values() if len(v) == 2) > sample["n"] // 2
    want = _direct(od)
    hist = _histogram(v[0][0] for v in by_name.values())                    # once per fragment
    assert hist == {k: v for k, v in want.items() if v} and len(hist) > 2
    m = re.search(r"tag_bam: \S+\tM=1\trecords (\d+)\ttagged (\d+)\tclassified (\d+)\tfragments (\d+)\t", errs)
    assert m and int(m.group(1)) == len(src) and int(m.group(4)) == sample["n"] == sum(want.values())


def test_a_record_that_bears_sn_says_one_line_and_leaves_no_file(L, mid_dbs, single, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    recs = [single["stream"][r["at"]:r["at"] + r["size"]] for r in bam_pairs_model.walk(single["stream"])]
    recs.insert(40, bamio.record("bears", "ACGT" * 30, flag=4, aux=b"NMC\1" + b"sni\5\0\0\0"))
    bam = tmp_path / "T.bam"
    bam.write_bytes(bamio.bgzf(HDR, recs, level=1))
    outs = {}
    for name, extra in (("off", []), ("on", ["--tag_bam"])):
        od = str(tmp_path / name)
        err, _, text, errs = _run(StrainScan.main, ["-i", str(bam), "-d", mid_dbs["DB_M"]["db_dir"], "-o", od, "--classify_reads", "1"] + extra)
        assert _ok(err), err
        outs[name] = (type(err), _result_lines(text), errs, _files(od))
    lines = _tag_lines(outs["on"][2])
    assert len(lines) == 1 and lines[0].startswith("tag_bam: 1 records of %s already bear an sn or sc tag" % bam) and "samtools view -x sn -x sc" in lines[0]
    assert lines[0].endswith(" and no tagged BAM was written") and not _tag_lines(outs["off"][2])
    assert outs["on"][0] is outs["off"][0] and outs["on"][1] == outs["off"][1] and outs["on"][3] == outs["off"][3] and TSV in outs["on"][3]


def test_multi_db_writes_one_file_per_label(L, runs, mid_dbs, single, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbm, dbmem = mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]
    c0 = L.bam_tag_calls()
    err, rc, _, errs = _run(multi_db.main, ["-i", single["bam"], "-d", dbm, "-d", "mem=" + dbmem, "-o", str(tmp_path / "out"),
                                            "--classify_reads", "1", "--tag_bam"])
    assert err is None and rc == 0 and L.bam_tag_calls() == c0 + 2
    want = gzip.decompress(open(os.path.join(runs["on"][3], OUT), "rb").read())
    for label in (os.path.basename(os.path.normpath(dbm)), "mem"):          # the two databases hold the same tree
        assert gzip.decompress(open(os.path.join(str(tmp_path / "out"), label, OUT), "rb").read()) == want, label
    assert not os.path.exists(os.path.join(str(tmp_path / "out"), OUT)) and len(_tag_lines(errs)) == 2
