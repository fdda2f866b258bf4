"""The BAM mate link without a device: the model's own invariants on the streams of tests/bam_pairs_cases.py, the parser rule of
--pairs (a BAM under -i needs no -j), and the new symbols of the C ABI."""
import argparse
import collections
import os
import re

import numpy as np
import pytest

from tests import bam_pairs_cases as cases, bam_pairs_model as bpm, bamio


@pytest.mark.parametrize("n", cases.SIZES)
def test_model_invariants(n):
    s = cases.stream(n)
    recs = bpm.walk(s)
    frags, mate, c, who = bpm.fragments(s)
    assert len(recs) == n == c[0] and c[5] == 0
    kept = [i for i, r in enumerate(recs) if bpm.kept(r)]
    assert c[1] == len(kept) == 2 * c[2] + c[3] + c[4]
    assert len(frags) == c[1] - c[2] == c[2] + c[3] + c[4]
    # the link is an involution on kept records, never reaches a record that is not kept, and joins equal names of roles {1, 2}
    for i in range(n):
        m = int(mate[i])
        assert (m == bpm.NOT_KEPT) == (i not in kept)
        if m < bpm.NO_MATE:
            assert int(mate[m]) == i and recs[m]["name"] == recs[i]["name"] and {bpm.role(recs[i]), bpm.role(recs[m])} == {1, 2}
            assert recs[i]["flag"] & recs[m]["flag"] & 0x1
    # bytes: the bases of the kept records, an N and a line end per fragment; every fragment holds exactly one more N than its mates
    flat, _ = bamio.flat(bamio.decode(s))
    assert sum(len(f) + 1 for f in frags) == (len(flat) - c[1]) + 2 * len(frags)
    forms = bpm.flat_forms(s, recs)
    assert collections.Counter(b"".join(frags).replace(b"N", b"")) == collections.Counter(flat.replace(b"\n", b"").replace(b"N", b""))
    for f, (i, m) in zip(frags, who):
        assert len(f) == len(forms[i]) + (len(forms[m]) if m is not None else 0) + 1
    assert [i for i, _ in who] == sorted(i for i, _ in who)           # in the stream order of the earlier record
    if n == 2:
        assert mate.tolist() == [1, 0] and frags == [forms[1] + b"N" + forms[0]]      # mate 2 stands first; mate 1 leads the fragment
    if n == 1:
        assert c == [1, 1, 0, 1, 0, 0] and frags == [forms[0] + b"N"]
    if n >= 255:
        by_name = collections.defaultdict(list)
        for i, r in enumerate(recs):
            by_name[r["name"]].append(i)
        assert int(mate[0]) == n - 1 and bpm.role(recs[0]) == 2                        # first and last record, mate 2 first
        assert sum(1 for i in by_name[b"d"] if i in kept) == 2 and len(by_name[b"d"]) == 5
        assert sum(1 for i in by_name[b"o"] if i in kept) == 1 and c[3] >= 6 and c[4] >= 5
        assert sum(1 for i in by_name[b"r1"] if int(mate[i]) < bpm.NO_MATE) == 2 and len(by_name[b"r1"]) == 3
        assert any(f.startswith(b"N") for f in frags) and any(f.endswith(b"N") for f in frags)
        assert {len(f) % 16 for f in frags} >= {2, 3, 0, 1}
    if n == 4097:
        assert max(len(f) for f in frags) == 40001


def test_mask_follows_the_stored_order():
    rec = [bamio.record("q", "ACGTACGT", flag=0x41 | 0x10, qual=bytes([30, 30, 5, 30, 30, 30, 30, 5])),
           bamio.record("q", "AAAA", flag=0x81, qual=b"\xff" * 4)]
    frags, _, c, _ = bpm.fragments(cases.HDR + b"".join(rec), min_qual=20)
    assert c[2] == 1 and frags == [bamio.revcomp("ACNTACGN").encode() + b"N" + b"AAAA"]


@pytest.mark.parametrize("shape,bad", [("three_of_one_name", 3), ("two_of_role_1", 2), ("role_0_shares_a_name", 2), ("one_name_257", 257)])
def test_violations(shape, bad):
    s = cases.violating()[shape]
    frags, mate, c, _ = bpm.fragments(s)
    assert frags is None and c[5] == bad and c[0] == len(bpm.walk(s))
    if shape != "one_name_257":                                         # the ordinary pairs beside the violation are still linked
        assert c[2] == 2 and c[4] == 1 and sum(1 for m in mate if m < bpm.NO_MATE) == 4


def test_parser_accepts_a_bam_without_j(tmp_path):
    from strainscan_amd import StrainScan
    bam, fq = tmp_path / "s.bam", tmp_path / "s.fq"
    bam.write_bytes(bamio.bgzf(cases.HDR, cases.records(2)))
    fq.write_bytes(bamio.fastq(["ACGT"]))
    ap = argparse.ArgumentParser()
    StrainScan.add_arguments(ap)
    ok = ap.parse_args(["-i", str(bam), "-d", "db", "--pairs", "--read_support"])
    StrainScan.refuse_pairs_alone(ap, ok)                               # passes
    with pytest.raises(SystemExit) as e:
        StrainScan.refuse_pairs_alone(ap, ap.parse_args(["-i", str(fq), "-d", "db", "--pairs", "--read_support"]))
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:                                # a BAM does not lift the other rule
        StrainScan.refuse_pairs_alone(ap, ap.parse_args(["-i", str(bam), "-d", "db", "--pairs"]))
    assert e.value.code == 2


def test_new_symbols_exist():
    from strainscan_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "strainscan_hip.h")).read()
    for name in ("ss_bam_mates", "ss_reads_join_pairs_bam", "ss_reads_load_pairs_bam", "ss_bam_select_pairs", "ss_bam_extract_pairs",
                 "ss_bam_pairs_timing"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert re.search(r"\bint %s\(" % name, header), name
    for name in ("bam_mates", "bam_pairs_timing"):
        assert callable(getattr(_lib, name))
    assert callable(_lib.ReadSet.join_pairs_bam) and callable(_lib.ReadSet.load_pairs_bam)
    import inspect
    assert "pairs" in inspect.signature(_lib.bam_extract).parameters and "pairs" in inspect.signature(_lib.bam_select).parameters
