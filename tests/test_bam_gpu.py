"""BAM input on the MI355X: the read set and the counts of a BAM equal those of the same reads as FASTQ, on the device path
(ss_bam_dev.hip: files of 1 MB and more) and on the host path (small files, SS_GZ_GPU=0), for the writer options of
tests/bamio.py; `strainscan -i S.bam` writes what `-i S.fq` writes; damaged streams raise and leave the process able to load
the next file."""
import ast
import contextlib
import io
import json
import os
import struct

import numpy as np
import pytest

from tests import bamio
from tests import scenarios as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _genome_reads(seed, n_reads, L_=150, G=60000):
    rs = np.random.RandomState(seed)
    lut = np.frombuffer(b"ACGT", np.uint8)
    g = lut[rs.randint(0, 4, size=G)].tobytes().decode()
    reads = []
    for i in range(n_reads):
        s = int(rs.randint(0, G - L_))
        r = g[s:s + L_]
        if rs.random_sample() < 0.05:
            j = int(rs.randint(0, L_))
            r = r[:j] + "N" + r[j + 1:]
        if rs.random_sample() < 0.01:
            j = int(rs.randint(0, L_))
            r = r[:j] + "MRW="[int(rs.randint(0, 4))] + r[j + 1:]
        reads.append(("q%d" % i, bamio.revcomp(r) if rs.random_sample() < 0.5 else r))
    kms = [g[i:i + 31] for i in range(0, G - 31, 3)]
    kfa = "".join(">1\n%s\n" % km for km in kms).encode()
    return reads, kfa


OPTIONS = {
    "plain_l6": dict(level=6, cuts="htslib", aligned=False, decoys=0.0, extras=False, eof=True),
    "stored_random_cuts": dict(level=0, cuts="random", aligned=True, decoys=0.2, extras=True, eof=True),
    "aligned_no_eof": dict(level=6, cuts="htslib", aligned=True, decoys=0.2, extras=True, eof=False),
    "random_cuts_l6": dict(level=6, cuts="random", aligned=False, decoys=0.1, extras=True, eof=True),
    "long_reads": dict(level=6, cuts="htslib", aligned=True, decoys=0.0, extras=False, eof=True, long=True),
}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (bam path, bgzip fastq path, plain fastq path, kept reads); every BAM >= 1 MB."""
    root = tmp_path_factory.mktemp("ss_bam")
    reads, kfa = _genome_reads(5, 30000)
    out = {"kfa": kfa}
    for i, (name, opt) in enumerate(OPTIONS.items()):
        rd = list(reads)
        if opt.get("long"):
            rs = np.random.RandomState(77)
            rd = rd[:2000] + [("long%d" % j, "".join("ACGT"[c] for c in rs.randint(0, 4, size=int(rs.randint(70000, 150000)))))
                              for j in range(40)] + rd[2000:]
        recs = bamio.sample_records(11 + i, rd, aligned=opt["aligned"], decoys=opt["decoys"], extras=opt["extras"])
        data = bamio.bgzf(bamio.header(), recs, level=opt["level"], cuts=opt["cuts"], eof=opt["eof"], seed=i)
        assert len(data) >= 1 << 20
        kept = bamio.decode(data)
        assert kept == [s for _, s in rd]
        p = root / ("%s.bam" % name)
        p.write_bytes(data)
        fq = bamio.fastq(kept)
        q = root / ("%s.fq.gz" % name)
        q.write_bytes(bamio.bgzip_text(fq))
        t = root / ("%s.fq" % name)
        t.write_bytes(fq)
        out[name] = (str(p), str(q), str(t), kept)
    small = root / "small.bam"
    sr = reads[:500]
    small.write_bytes(bamio.bgzf(bamio.header(), bamio.sample_records(3, sr, aligned=True, decoys=0.2), level=6))
    out["small"] = (str(small), None, None, [s for _, s in sr])
    return out


def _load(L, paths, monkeypatch, order=None, gz_gpu=None):
    if order:
        monkeypatch.setenv("SS_READS_ORDER", order)
    else:
        monkeypatch.delenv("SS_READS_ORDER", raising=False)
    if gz_gpu is not None:
        monkeypatch.setenv("SS_GZ_GPU", gz_gpu)
    else:
        monkeypatch.delenv("SS_GZ_GPU", raising=False)
    rs = L.ReadSet(paths)
    try:
        return rs.read_back(), rs.info()
    finally:
        rs.close()


def records(block):
    return sorted(r for r in block.split(b"\n") if r)


def _padded(flat):
    return flat + b"\n" * (((len(flat) + 1 + 15) & ~15) - len(flat))


@pytest.mark.parametrize("name", list(OPTIONS))
def test_read_set_equals_fastq(L, files, name, monkeypatch):
    bam, fqgz, _, kept = files[name]
    want, n_want = bamio.flat(kept)
    c0 = L.bam_counters()
    got, info = _load(L, [bam], monkeypatch, order="file")
    c1 = L.bam_counters()
    assert c1["device"] == c0["device"] + 1 and c1["host"] == c0["host"], (c0, c1)
    assert got == _padded(want)
    assert info["n_records"] == n_want and info["n_bases"] == len(want)
    # the same reads as a .fq.gz, in file order and binned: byte for byte where that file takes the device path too (one
    # block, like the BAM's); a .fq.gz of 150-kb records goes to the host parser, whose parse chunks land in the slab in
    # the order the threads finish them, and a ragged slab's order inside a bin is whatever its atomics decide: the same
    # records then
    fq_got, _ = _load(L, [fqgz], monkeypatch, order="file")
    got_b, _ = _load(L, [bam], monkeypatch)
    fq_b, _ = _load(L, [fqgz], monkeypatch)
    if name == "long_reads":
        assert records(fq_got) == records(got) and records(got_b) == records(fq_b) == records(got)
    else:
        assert fq_got == got and got_b == fq_b
    # the host path (SS_GZ_GPU=0) gives the same block
    h0 = L.bam_counters()["host"]
    got_h, _ = _load(L, [bam], monkeypatch, order="file", gz_gpu="0")
    assert L.bam_counters()["host"] == h0 + 1
    assert got_h == got


def test_small_file_takes_the_host_path(L, files, monkeypatch):
    bam, _, _, kept = files["small"]
    c0 = L.bam_counters()
    got, info = _load(L, [bam], monkeypatch, order="file")
    c1 = L.bam_counters()
    assert c1["host"] == c0["host"] + 1 and c1["device"] == c0["device"]
    want, n = bamio.flat(kept)
    assert got == _padded(want) and info["n_records"] == n


@pytest.mark.parametrize("name", ["plain_l6", "stored_random_cuts", "long_reads"])
def test_counts_equal_fastq(L, files, name, monkeypatch):
    monkeypatch.delenv("SS_GZ_GPU", raising=False)
    bam, fqgz, fq, _ = files[name]
    db = L.KmerDB.from_text(files["kfa"], 31, True)
    try:
        res = {}
        for key, paths in (("bam", [bam]), ("fq", [fq]), ("fqgz", [fqgz])):
            db.reset()
            db.scan_files(paths)
            res[key + "_stream"] = db.counts_rows()
            db.reset()
            rs = L.ReadSet(paths)
            rs.scan_into(db)
            L.lib().ss_device_sync()
            rs.close()
            res[key + "_resident"] = db.counts_rows()
        for k, v in res.items():
            assert np.array_equal(v, res["fq_stream"]), k
        assert int(res["fq_stream"].sum()) > 0
        # sharded: the ranks' shares add up to the whole
        tot = np.zeros_like(res["fq_stream"])
        for rank in range(3):
            db.reset()
            db.scan_files([bam], rank, 3)
            tot += db.counts_rows()
        assert np.array_equal(tot, res["fq_stream"])
    finally:
        db.close()


def test_damaged_bam_raises_then_a_good_file_loads(L, files, tmp_path, monkeypatch):
    monkeypatch.delenv("SS_GZ_GPU", raising=False)
    monkeypatch.setenv("SS_READS_ORDER", "file")
    _, _, _, kept = files["plain_l6"]
    rs = np.random.RandomState(9)
    recs = [bamio.record("r%d" % i, s, qual=rs.randint(2, 41, size=len(s)).astype(np.uint8).tobytes()) for i, s in enumerate(kept)]
    bad = list(recs)
    bad[len(bad) // 2] = struct.pack("<i", 20) + bad[len(bad) // 2][4:]           # block_size below 32
    for level in (0, 6):
        p = tmp_path / ("bad%d.bam" % level)
        p.write_bytes(bamio.bgzf(bamio.header(), bad, level=level))
        assert os.path.getsize(p) >= 1 << 20
        d0 = L.bam_counters()["device"]
        with pytest.raises(L.SSError) as e:
            L.ReadSet([str(p)])
        assert e.value.code == L.SS_EIO
        assert L.bam_counters()["device"] == d0
    truncated = tmp_path / "cut.bam"
    data = bamio.bgzf(bamio.header(), recs, level=0, eof=False)
    truncated.write_bytes(data[:len(data) - 70000])
    with pytest.raises(L.SSError):
        L.ReadSet([str(truncated)])
    bam = files["plain_l6"][0]
    got, _ = _load(L, [bam], monkeypatch, order="file")
    assert got == _padded(bamio.flat(kept)[0])


def _member_spans(data):
    """(offset, size) of every BGZF member of a file."""
    out, o = [], 0
    while o < len(data):
        size = struct.unpack_from("<H", data, o + 16)[0] + 1
        out.append((o, size))
        o += size
    return out


@pytest.mark.parametrize("field", ["crc", "isize"])
@pytest.mark.parametrize("n_reads", [12000, 300])
def test_bad_member_crc_or_length_raises(L, files, field, n_reads, tmp_path, monkeypatch):
    """A member whose CRC-32 or ISIZE does not match its data: SS_EIO from a load and from a scan, nothing loaded -- for a file of
    1 MB and more (the device inflater declines it, the host inflaters find it) and for a small one (host path only)."""
    monkeypatch.delenv("SS_GZ_GPU", raising=False)
    _, _, _, kept = files["plain_l6"]
    rs = np.random.RandomState(13)
    recs = [bamio.record("r%d" % i, s, qual=rs.randint(2, 41, size=len(s)).astype(np.uint8).tobytes())
            for i, s in enumerate(kept[:n_reads])]
    data = bytearray(bamio.bgzf(bamio.header(), recs, level=0))
    assert (len(data) >= 1 << 20) == (n_reads > 1000)
    spans = _member_spans(bytes(data))
    o, size = spans[len(spans) // 2]
    data[o + size - (8 if field == "crc" else 4)] ^= 0x01
    p = tmp_path / "bad.bam"
    p.write_bytes(bytes(data))
    with pytest.raises(L.SSError) as e:
        L.ReadSet([str(p)])
    assert e.value.code == L.SS_EIO
    db = L.KmerDB.from_text(files["kfa"], 31, True)
    try:
        with pytest.raises(L.SSError) as e:
            db.scan_files([str(p)])
        assert e.value.code == L.SS_EIO
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------
# the whole command
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid(mid_dbs, tmp_path_factory):
    """The mid database and its M_mix sample as a BAM (aligned: half the records reverse-complemented, decoys) and as the
    FASTQ made from that BAM."""
    root = tmp_path_factory.mktemp("ss_bam_mid")
    names, seqs = bamio.fastq_reads(mid_dbs["reads"]["M_mix"][1])
    recs = bamio.sample_records(21, list(zip(names, seqs)), aligned=True, decoys=0.1, extras=True)
    bam = root / "M_mix.bam"
    bam.write_bytes(bamio.bgzf(bamio.header(), recs, level=6))
    fqp = root / "M_mix.fq"
    fqp.write_bytes(bamio.fastq(seqs, names))
    return mid_dbs["DB_M"], str(bam), str(fqp)


def _files(d):
    out = {}
    for root, _, fs in os.walk(d):
        for f in fs:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def _run(argv):
    from strainscan_amd import StrainScan
    from strainscan_amd import db as ssdb
    ssdb.clear_cache()
    np.random.seed(sc.POISSON_SEED)
    buf = io.StringIO()
    err = None
    with contextlib.redirect_stdout(buf):
        try:
            StrainScan.main(argv)
        except BaseException as e:      # noqa: B902 -- how the run ended is part of what is compared
            err = e
    return err, buf.getvalue()


@pytest.mark.parametrize("argv,golden", [([], "mix_default"), (["-b", "1"], "mix_b1"), (["-l", "1"], "mix_l1"),
                                         (["-e", "1"], "mix_e1"), (["-k", "25"], None)])
def test_command_bam_equals_fastq(L, mid, argv, golden, golden_dir, tmp_path, monkeypatch):
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    info, bam, fq = mid
    e1, t1 = _run(["-i", bam, "-d", info["db_dir"], "-o", str(tmp_path / "bam")] + argv)
    e2, t2 = _run(["-i", fq, "-d", info["db_dir"], "-o", str(tmp_path / "fq")] + argv)
    assert type(e1) is type(e2), (argv, e1, e2)
    a, b = _files(str(tmp_path / "bam")), _files(str(tmp_path / "fq"))
    assert a or e1 is not None, argv
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in b), argv
    if golden:
        # the reference's own run on the same reads (tests/test_mid_gpu.py::test_mid_flow_cli compares the same way)
        from tests.test_mid_gpu import _cmp_report
        g = json.load(open(os.path.join(golden_dir, "mid_flow.json")))[golden]
        assert (type(e1).__name__ if e1 is not None and not isinstance(e1, SystemExit) else None) == (g["error"] or None), golden
        got = {k: v.decode() for k, v in a.items()}
        assert sorted(got) == sorted(g["files"]), golden
        for rel, want_text in g["files"].items():
            if rel == "strain_prob.txt":
                gl, wl = got[rel].strip().split("\n"), want_text.strip().split("\n")
                assert gl[0] == wl[0] and len(gl) == len(wl)
                for x, y in zip(gl[1:], wl[1:]):
                    fx, fy = x.split("\t"), y.split("\t")
                    assert fx[0] == fy[0] and fx[2:] == fy[2:] and abs(float(fx[1]) - float(fy[1])) <= 1e-12 * max(1.0, float(fy[1]))
            elif rel == "final_report.txt" and len(ast.literal_eval(g["cls_dict"])) > 1:
                _cmp_report(got[rel], want_text, float_cols=(3, 4, 5, 6))
            else:
                _cmp_report(got[rel], want_text, float_cols=(3, 4, 5, 6, 8, 9))


def test_command_streaming_and_multi(L, mid, tmp_path, monkeypatch):
    """Streaming (no resident read set: every scan decodes the BAM again) and strainscan-multi give what the resident run
    gives."""
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    info, bam, fq = mid
    _run(["-i", bam, "-d", info["db_dir"], "-o", str(tmp_path / "res")])
    from strainscan_amd import db as ssdb
    with monkeypatch.context() as m:
        m.setattr(ssdb, "RESIDENT_LIMIT_BYTES", 0)
        _run(["-i", bam, "-d", info["db_dir"], "-o", str(tmp_path / "stream")])
    a, b = _files(str(tmp_path / "res")), _files(str(tmp_path / "stream"))
    assert a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    from strainscan_amd import multi_db
    ssdb.clear_cache()
    with contextlib.redirect_stdout(io.StringIO()):
        rows_b = multi_db.identify_databases((bam, ""), [info["db_dir"]], str(tmp_path / "mb"),
                                             before_each=lambda i: np.random.seed(sc.POISSON_SEED))
        ssdb.clear_cache()
        rows_f = multi_db.identify_databases((fq, ""), [info["db_dir"]], str(tmp_path / "mf"),
                                             before_each=lambda i: np.random.seed(sc.POISSON_SEED))
    assert [r[2] for r in rows_b] == [r[2] for r in rows_f] == ["reports"]
    a, b = _files(str(tmp_path / "mb")), _files(str(tmp_path / "mf"))
    a.pop(multi_db.TSV, None)
    b.pop(multi_db.TSV, None)
    assert a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)


def test_cram_is_refused_by_the_command(L, mid, tmp_path):
    info, _, _ = mid
    cram = tmp_path / "s.cram"
    cram.write_bytes(b"CRAM\3\0" + b"\0" * 64)
    err, _ = _run(["-i", str(cram), "-d", info["db_dir"], "-o", str(tmp_path / "o")])
    assert err is not None and err.code == 2
