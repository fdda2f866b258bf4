"""`strainscan -x N` on a BAM sample: extracted/<table>_1.bam is a BGZF BAM with the input's header and, byte for byte and in file
order, the records the model of tests/test_bam_select_gpu.py writes for the table -- for the tree's table, every cluster table
scanned at layer 2 and, with --by_strain, every called strain; the read names are those `-x N` extracts from the same reads as
FASTQ; stdout and every report are those of a run without the flag; without the flag nothing new runs; a mix of BAM and FASTQ
inputs is refused with one line."""
import gzip
import os
import pickle

import numpy as np
import pytest

from tests import bamio, label_model, rs_model
from tests.test_bam_select_gpu import HDR, model, walk
from tests.test_extract_cli_gpu import DIR, _files, _ok, _reports, _result_lines, _run, _with_cache, pair      # noqa: F401

pytestmark = pytest.mark.gpu

N = 16


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _keys_of(fasta_path, k=31):
    with open(fasta_path, "rb") as f:
        kmers = list(dict.fromkeys(km.upper() for km in rs_model.kmers_of_fasta(f.read())))
    return rs_model.encode_kmers(kmers, k)


def _table_fasta(db_dir, t):
    return (os.path.join(db_dir, "Tree_database", "kmer.fa") if t == "tree"
            else os.path.join(db_dir, "Kmer_Sets_L2", "Kmer_Sets", t, "all_kmer.fasta"))


def _names(stream_or_records):
    return [r[4] for r in walk(stream_or_records)]


@pytest.fixture(scope="module")
def sample(mid_dbs, tmp_path_factory):
    """M_mix as a BAM of 1 MB and more (half the records 0x10, decoys under the reads' names, aux data, records without bases)
    and as the FASTQ of the same reads -> dict(bam=, fq=, stream=)"""
    root = tmp_path_factory.mktemp("xb_sample")
    names, seqs = bamio.fastq_reads(mid_dbs["reads"]["M_mix"][1])
    recs = bamio.sample_records(21, list(zip(names, seqs)), aligned=True, decoys=0.1, extras=True)
    data = bamio.bgzf(HDR, recs, level=6)
    assert len(data) >= 1 << 20
    bam, fq = root / "S.bam", root / "S.fq"
    bam.write_bytes(data)
    fq.write_bytes(bamio.fastq(seqs, names))
    return dict(bam=str(bam), fq=str(fq), stream=HDR + b"".join(recs), root=root)


@pytest.fixture(scope="module")
def runs(L, mid_dbs, sample, tmp_path_factory):
    """`strainscan -i S.bam` without and with -x 16, and `-i S.fq -x 16` -> name: (err, stdout, stderr, out dir, bam extract
    calls made, bam counters before and after)"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("xb_cli")

    def go():
        out = {}
        for name, inp, extra in (("plain", sample["bam"], []), ("flag", sample["bam"], ["-x", str(N)]), ("fq", sample["fq"], ["-x", str(N)])):
            before, c0 = L.bam_extract_calls(), L.bam_counters()
            od = str(root / name)
            err, _, text, errs = _run(StrainScan.main, ["-i", inp, "-d", mid_dbs["DB_M"]["db_dir"], "-o", od] + extra)
            out[name] = (err, text, errs, od, L.bam_extract_calls() - before, c0, L.bam_counters())
        return out
    return _with_cache(root, go)


def _tables(out_dir):
    clusters = sorted(d for d in os.listdir(out_dir) if d.startswith("C") and os.path.isdir(os.path.join(out_dir, d)))
    assert len(clusters) >= 2
    return ["tree"] + clusters


def _check_bam(path, stream, keys, n):
    """the file against the model -> the model's counters"""
    data = open(path, "rb").read()
    assert data.endswith(bamio.EOF)
    got = gzip.decompress(data)
    want, wc = model(stream, keys, 31, n)
    assert got[:len(HDR)] == HDR
    assert got[len(HDR):] == want, (path, len(got), len(want))
    return wc


def test_extracted_bams_are_the_models(runs, mid_dbs, sample):
    err, _, errs, od, calls, c0, c1 = runs["flag"]
    assert _ok(err), err
    ex = os.path.join(od, DIR)
    tables = _tables(od)
    assert sorted(os.listdir(ex)) == sorted("%s_1.bam" % t for t in tables)
    lines = {ln.split("\t")[0].split(" ")[1]: ln for ln in errs.split("\n") if ln.startswith("extract_reads:")}
    assert sorted(lines) == sorted(tables)
    sizes = {}
    for t in tables:
        wc = _check_bam(os.path.join(ex, "%s_1.bam" % t), sample["stream"], _keys_of(_table_fasta(mid_dbs["DB_M"]["db_dir"], t)), N)
        print(t, wc)
        sizes[t] = wc
        # one line per table and file: table, N, file, records kept, selected, written
        assert lines[t] == "extract_reads: %s\tN=%d\tfile 1\tkept %d\tselected on the device %d\twritten %d" % (t, N, wc[1], wc[2], wc[3])
    assert calls == len(tables)
    assert any(0 < wc[3] < wc[1] for t, wc in sizes.items() if t != "tree"), sizes      # neither empty nor everything
    assert all(wc[0] > wc[1] for wc in sizes.values())                                # decoys and empty records were there to skip
    # a file of 1 MB and more: inflated on the device, once per table and once for the load
    assert c1["device"] - c0["device"] >= len(tables) + 1 and c1["host"] == c0["host"]


def test_read_names_are_those_of_the_fastq_run(runs):
    _, _, _, od_b, _, _, _ = runs["flag"]
    err, _, _, od_f, _, _, _ = runs["fq"]
    assert _ok(err), err
    seen = 0
    for t in _tables(od_b):
        got = _names(gzip.decompress(open(os.path.join(od_b, DIR, "%s_1.bam" % t), "rb").read()))
        fq = open(os.path.join(od_f, DIR, "%s_1.fastq" % t), "rb").read().split(b"\n")
        want = [ln[1:].split()[0] for ln in fq[0:-1:4]]
        assert len(got) == len(set(got)) and sorted(got) == sorted(want), t
        seen += len(got)
    assert seen


def test_flag_off_runs_nothing_and_reports_are_unchanged(runs):
    e0, t0, errs0, d0, calls0, _, _ = runs["plain"]
    e1, t1, _, d1, calls1, _, _ = runs["flag"]
    assert _ok(e0) and _ok(e1) and type(e0) is type(e1)
    assert calls0 == 0 and calls1 > 0 and "extract_reads" not in errs0
    assert not os.path.exists(os.path.join(d0, DIR)) and os.path.isdir(os.path.join(d1, DIR))
    a, b = _files(d0), _reports(d1)
    assert a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    assert t0 == t1 or _result_lines(t0) == _result_lines(t1)
    assert _result_lines(t0)


def test_collated_pairs_are_the_fastq_pairs(L, mid_dbs, pair, tmp_path, monkeypatch):
    """0x40 / 0x80 mates under one name: the 0x40 names of <table>_1.bam are those of -i R1.fq -j R2.fq's _1.fastq, the 0x80
    names those of _2.fastq"""
    from strainscan_amd import StrainScan
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    rs = np.random.RandomState(5)
    recs = []
    for i, (m1, m2) in enumerate(zip(*pair["recs"])):
        for m, (_, s) in enumerate((m1, m2)):
            s = s.decode().upper()
            rev = rs.random_sample() < 0.5
            recs.append(bamio.record("pair%d" % i, bamio.revcomp(s) if rev else s, flag=0x1 | (0x40, 0x80)[m] | (0x10 if rev else 0),
                                     qual=rs.randint(2, 41, size=len(s)).astype(np.uint8).tobytes()))
    bam = tmp_path / "P.bam"
    bam.write_bytes(bamio.bgzf(HDR, recs, level=6))
    db_dir = mid_dbs["DB_M"]["db_dir"]
    e1, _, _, _ = _run(StrainScan.main, ["-i", str(bam), "-d", db_dir, "-o", str(tmp_path / "b"), "-x", str(N)])
    e2, _, _, _ = _run(StrainScan.main, ["-i", pair["paths"][0], "-j", pair["paths"][1], "-d", db_dir, "-o", str(tmp_path / "f"), "-x", str(N)])
    assert _ok(e1) and _ok(e2)
    tables = _tables(str(tmp_path / "b"))
    seen = 0
    for t in tables:
        out = walk(gzip.decompress(open(os.path.join(str(tmp_path / "b"), DIR, "%s_1.bam" % t), "rb").read()))
        for m, bit in ((1, 0x40), (2, 0x80)):
            fq = open(os.path.join(str(tmp_path / "f"), DIR, "%s_%d.fastq" % (t, m)), "rb").read().split(b"\n")
            want = [ln[1:].rsplit(b"/", 1)[0] for ln in fq[0:-1:4]]
            got = [r[4] for r in out if r[2] & bit]
            assert got == want, (t, m, len(got), len(want))                     # the same pairs, in the same order
            seen += len(got)
    assert seen


def test_host_inflate_routes_give_the_models_file(L, mid_dbs, sample, tmp_path, monkeypatch):
    """SS_GZ_GPU=0, and a copy of the sample cut to below 1 MB: inflated on the host, uploaded, the same path from there on"""
    fa = _table_fasta(mid_dbs["DB_M"]["db_dir"], "tree")
    keys = _keys_of(fa)
    db = L.KmerDB.from_text(open(fa, "rb").read(), 31, True)
    try:
        # the device route first, for the counters
        c0 = L.bam_counters()
        c = L.bam_extract(sample["bam"], db, N, str(tmp_path / "dev.bam"))
        c1 = L.bam_counters()
        assert c1["device"] == c0["device"] + 1 and c1["host"] == c0["host"]
        wc = _check_bam(str(tmp_path / "dev.bam"), sample["stream"], keys, N)
        assert [c[x] for x in L.BAM_SELECT_COUNTERS] == wc and wc[3] > 0
        monkeypatch.setenv("SS_GZ_GPU", "0")
        L.bam_extract(sample["bam"], db, N, str(tmp_path / "host.bam"))
        monkeypatch.delenv("SS_GZ_GPU")
        c2 = L.bam_counters()
        assert c2["host"] == c1["host"] + 1 and c2["device"] == c1["device"]
        assert open(str(tmp_path / "host.bam"), "rb").read() == open(str(tmp_path / "dev.bam"), "rb").read()
        # below 1 MB, and the same stream uncompressed
        recs = [sample["stream"][r[0]:r[0] + r[1]] for r in walk(sample["stream"])][:4000]
        small = HDR + b"".join(recs)
        (tmp_path / "small.bam").write_bytes(bamio.bgzf(HDR, recs, level=6))
        (tmp_path / "raw.bam").write_bytes(small)
        assert os.path.getsize(str(tmp_path / "small.bam")) < 1 << 20
        for name in ("small", "raw"):
            L.bam_extract(str(tmp_path / (name + ".bam")), db, N, str(tmp_path / (name + "_out.bam")))
            assert _check_bam(str(tmp_path / (name + "_out.bam")), small, keys, N)[3] > 0
        c3 = L.bam_counters()
        assert c3["host"] == c2["host"] + 2 and c3["device"] == c2["device"]
        assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
        # a FASTQ is no BAM; an unwritable output leaves nothing
        with pytest.raises(L.SSError) as e:
            L.bam_extract(sample["fq"], db, N, str(tmp_path / "no.bam"))
        assert e.value.code == L.SS_EINVAL and not os.path.exists(str(tmp_path / "no.bam"))
        with pytest.raises(L.SSError) as e:
            L.bam_extract(sample["bam"], db, N, str(tmp_path / "no_dir" / "no.bam"))
        assert e.value.code == L.SS_EIO and not os.path.exists(str(tmp_path / "no_dir"))
    finally:
        db.close()


def test_a_mix_of_bam_and_fastq_is_refused(L, runs, mid_dbs, sample, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    od = str(tmp_path / "out")
    before = L.bam_extract_calls()
    err, _, _, errs = _run(StrainScan.main, ["-i", sample["bam"], "-j", sample["fq"], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od, "-x", str(N)])
    err0, _, _, _ = _run(StrainScan.main, ["-i", sample["bam"], "-j", sample["fq"], "-d", mid_dbs["DB_M"]["db_dir"], "-o", str(tmp_path / "plain")])
    lines = [ln for ln in errs.split("\n") if ln.startswith("extract_reads:")]
    assert len(lines) == 1 and "not both" in lines[0] and "nothing was extracted" in lines[0], lines
    assert type(err) is type(err0) and L.bam_extract_calls() == before
    assert not os.path.exists(os.path.join(od, DIR))
    a, b = _files(str(tmp_path / "plain")), _files(od)
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)


def test_by_strain_writes_the_labelled_models(L, mid_dbs, sample, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    import scipy.sparse as sp
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    od = str(tmp_path / "out")
    n = 4
    err, _, _, errs = _run(StrainScan.main, ["-i", sample["bam"], "-d", mid_dbs["DB_M"]["db_dir"], "-o", od, "-x", str(n), "--by_strain"])
    assert _ok(err), err
    ex = os.path.join(od, DIR)
    strain_files = sorted(f for f in os.listdir(ex) if "." in f.split("_")[0])
    want_files = []
    written = {}
    for cls in _tables(od)[1:]:
        report = os.path.join(od, cls, "StrainVote.report")
        if not os.path.exists(report):
            continue
        called = [(int(r[0]), r[1]) for r in (ln.split("\t") for ln in open(report).read().split("\n")[1:] if ln.strip())]
        cdir = os.path.join(mid_dbs["DB_M"]["db_dir"], "Kmer_Sets_L2", "Kmer_Sets", cls)
        with open(os.path.join(cdir, "id2strain_re.pkl"), "rb") as f:
            sid = pickle.load(f)
        col_of = {name: c for c, name in (sid.items() if isinstance(sid, dict) else enumerate(sid))}
        dense = np.asarray(sp.load_npz(os.path.join(cdir, "all_strains_re.npz")).todense())
        lab = label_model.row_labels(dense, [col_of[name] for _, name in called])
        with open(os.path.join(cdir, "all_kmer.fasta"), "rb") as f:
            keys = rs_model.encode_kmers([km.upper() for km in rs_model.kmers_of_fasta(f.read())], 31)
        for j, (num, _) in enumerate(called, 1):
            t = "%s.%d" % (cls, num)
            want_files.append("%s_1.bam" % t)
            written[t] = _check_bam(os.path.join(ex, "%s_1.bam" % t), sample["stream"], label_model.label_keys(keys, lab, j), n)[3]
    print(written)
    assert strain_files == sorted(want_files) and len(want_files) >= 3
    assert any(v > 0 for v in written.values())
    lines = [ln for ln in errs.split("\n") if ln.startswith("extract_reads:") and "." in ln.split("\t")[0]]
    assert sorted(ln.split("\t")[0].split(" ")[1] for ln in lines) == sorted(written)
