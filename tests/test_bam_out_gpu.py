"""The file step that ss_bam_extract and ss_bam_tag_file share (ss_bam_out.hip): header and body to the host, the BGZF file written
to <out_path>.tmp and renamed, nothing left on any error, the file counted and the call's eight timing slots published.  Every case
runs through both callers, on hand-built streams of four records (files of about a kilobyte: the host-inflate route).  The table,
the forest and the record helpers are those of tests/test_bam_tag_gpu.py."""
import gzip
import os

import pytest

from tests import bamio
from tests.test_bam_tag_gpu import HDR, L, R, T, cold, genome, of_node, tags_of      # noqa: F401 (L, T, genome: fixtures)
from tests.test_bgzf_write_host import _members

pytestmark = pytest.mark.gpu

CALLS = ("extract", "tag")
MIN_HITS = 5


def call(L, T, which, in_path, out_path, min_hits=MIN_HITS):
    """-> the call's counters (extract: BAM_SELECT_COUNTERS, tag: BAM_TAG_COUNTERS)"""
    if which == "extract":
        return L.bam_extract(str(in_path), T.db, min_hits, str(out_path))
    return L.bam_tag_file(str(in_path), T.db, T.row_node, T.parent, min_hits, T.value, str(out_path))


def timing(L, which):
    return L.bam_extract_timing() if which == "extract" else L.bam_tag_timing()


def all_timings(L):
    return {"extract": L.bam_extract_timing(), "tag": L.bam_tag_timing(), "pairs": L.bam_pairs_timing()}


@pytest.fixture(scope="module")
def records(genome):
    import numpy as np
    rs = np.random.RandomState(31)
    return [R("hot4", of_node(genome, 4, 100, 150)), R("cold", cold(rs)), R("decoy", of_node(genome, 5, 0, 100), flag=0x100, aux=b"snA!"),
            R("hot9", bamio.revcomp(of_node(genome, 9, 200, 120)), flag=0x10, aux=b"XAAx")]


@pytest.fixture(scope="module")
def unkept(genome):
    return [R("u%d" % i, of_node(genome, 1 + i, 2 * i, 80 + i), flag=0x100, aux=b"XAAx" if i % 2 else b"") for i in range(3)]


def write_input(tmp_path, recs):
    p = tmp_path / "in.bam"
    p.write_bytes(bamio.bgzf(HDR, recs, level=1))
    assert p.stat().st_size < 4096
    return p


def refused_with_eio(L, T, which, in_path, out_path):
    """the call fails with SS_EIO (the tag call: as BamTagError), publishes no timing and counts no file"""
    before, files = all_timings(L), L.bam_counters()
    with pytest.raises(L.BamTagError if which == "tag" else L.SSError) as e:
        call(L, T, which, in_path, out_path)
    assert e.value.code == L.SS_EIO
    assert all_timings(L) == before and L.bam_counters()["host"] == files["host"] and L.bam_counters()["device"] == files["device"]


@pytest.mark.parametrize("which", CALLS)
def test_out_path_in_a_directory_that_does_not_exist(L, T, records, tmp_path, which):
    p = write_input(tmp_path, records)
    refused_with_eio(L, T, which, p, tmp_path / "nowhere" / "out.bam")
    assert sorted(os.listdir(tmp_path)) == ["in.bam"]                  # nothing is created


@pytest.mark.parametrize("which", CALLS)
def test_out_path_names_a_directory(L, T, records, tmp_path, which):
    p = write_input(tmp_path, records)
    d = tmp_path / "out.bam"
    d.mkdir()
    refused_with_eio(L, T, which, p, d)                                # (the rename fails)
    assert sorted(os.listdir(tmp_path)) == ["in.bam", "out.bam"]       # no out.bam.tmp beside it
    assert d.is_dir() and os.listdir(d) == []


@pytest.mark.parametrize("which", CALLS)
def test_header_and_no_kept_record(L, T, unkept, tmp_path, which):
    p, out = write_input(tmp_path, unkept), tmp_path / "out.bam"
    c = call(L, T, which, p, out)
    data = out.read_bytes()
    assert data.endswith(bamio.EOF) and sorted(os.listdir(tmp_path)) == ["in.bam", "out.bam"]
    if which == "extract":
        assert c == dict(records=3, kept=0, selected=0, written=0)
        assert gzip.decompress(data) == HDR
        assert _members(data) == [HDR, b""]                            # the header's member and the EOF block
    else:
        assert c["records"] == 3 and c["tagged"] == 0 and c["classified"] == 0
        assert gzip.decompress(data) == HDR + b"".join(unkept)         # the records that are not kept, unchanged


def test_extract_min_hits_that_no_record_reaches(L, T, records, tmp_path):
    p, out = write_input(tmp_path, records), tmp_path / "out.bam"
    c = call(L, T, "extract", p, out, min_hits=1000)
    assert c == dict(records=4, kept=3, selected=0, written=0)
    assert _members(out.read_bytes()) == [HDR, b""]
    assert sorted(os.listdir(tmp_path)) == ["in.bam", "out.bam"]


def test_same_input_through_both_calls(L, T, records, tmp_path):
    """... and what each call leaves behind: its own timing, the file counted once, the other features' timings untouched"""
    p = write_input(tmp_path, records)
    outs = {}
    for which in CALLS:
        before, files = all_timings(L), L.bam_counters()
        out = tmp_path / (which + ".bam")
        c = call(L, T, which, p, out)
        after, tm = all_timings(L), timing(L, which)
        print(which, c, tm)
        assert tm["total"] > 0 and tm["download"] >= 0 and tm["stream"] > 0 and tm["compress_write"] > 0
        assert tm != before[which] and tm["total"] >= tm["stream"] + tm["download"] + tm["compress_write"]
        assert all(after[k] == before[k] for k in after if k != which)      # three timings, kept apart
        assert L.bam_counters()["host"] == files["host"] + 1 and L.bam_counters()["device"] == files["device"]
        data = out.read_bytes()
        assert data.endswith(bamio.EOF)
        outs[which] = gzip.decompress(data)
        assert outs[which][:len(HDR)] == HDR                            # the input's header, byte for byte
    assert sorted(os.listdir(tmp_path)) == ["extract.bam", "in.bam", "tag.bam"]
    assert outs["extract"] == HDR + records[0] + records[3]            # 60 and 45 hits; the cold record and the decoy are not written
    assert [(name, sn, sc) for _, name, sn, sc in tags_of(outs["tag"][len(HDR):])] == \
        [(b"hot4", 104, 60), (b"cold", -1, 0), (b"decoy", None, None), (b"hot9", 109, 45)]
    assert len(outs["tag"]) == len(HDR) + sum(len(r) for r in records) + 3 * L.BAM_TAG_BYTES
