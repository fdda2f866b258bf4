"""`--divergence` without a device: the model (tests/gap_model.py) on hand-built records whose answers are known from the rule
alone, the conditions that keep tests/test_gaps_gpu.py from passing vacuously, the flag's parser and state, and the file's text."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gap_cases as gc, gap_model as gm, rs_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO = ("hits_called", "hits_cluster", "misses", "gap_lt", "gap_km1", "gap_k", "gap_k_2k", "gap_ge2k", "gaps_in_cluster", "sites", "reads_with_sites",
        "detectable")


@pytest.fixture(scope="module")
def g():
    return gc.genome()


@pytest.fixture(scope="module")
def k31(g):
    return gc.table("k31", g)


def _one(record, keys, row_called=None, m=1):
    return gm.gaps_model(record + b"\n", keys, row_called, gc.K, m)


@pytest.mark.parametrize("name", ["clean", "sub_75", "sub_10", "deletion", "insertion_3", "two_subs", "n_at_75", "short", "exactly_k"])
def test_hand_built_records(g, k31, name):
    _, kmers, keys, _ = k31
    record, want = gc.hand_records(g)[name]
    tot, rec = _one(record, keys)
    print(name, tot)
    # no planted k-mer is in the table by accident: the windows over a changed base are all misses
    have = set(kmers)
    windows = [record[p:p + 31] for p in range(len(record) - 30)]
    assert sum(w in have for w in windows) == want.get("hits_called", 0)
    assert tot["records"] == 1 and tot["assessed"] == (1 if want.get("hits_called", 0) else 0)
    for f in ZERO:
        assert tot[f] == want.get(f, 0), (f, tot[f])
    assert tot["windows"] == tot["hits_called"] + tot["misses"] == sum(all(c in b"ACGT" for c in w) for w in windows)
    assert tot["kmers"] == tot["kmers_called"] == len(kmers) and tot["long_records"] == 0
    gaps = sum(tot[f] for f in ("gap_lt", "gap_km1", "gap_k", "gap_k_2k", "gap_ge2k"))
    assert rec.tolist() == [[tot["hits_called"], gaps, tot["sites"], tot["detectable"]]]
    if name == "clean":
        assert tot["detectable"] == 88 and gaps == 0
    if name == "insertion_3":
        assert windows.index(next(w for w in windows if w not in have)) == 45 and tot["misses"] == gc.K + 2


def test_a_run_of_uncalled_kmers_is_in_cluster(g, k31):
    _, kmers, keys, starts = k31
    record, uncalled = gc.in_cluster_case(g)
    called = np.array([s not in uncalled for s in starts], np.uint8)
    tot, rec = _one(record, keys, called)
    assert tot["hits_called"] == 120 - 41 and tot["hits_cluster"] == 41 and tot["misses"] == 0
    assert tot["gaps_in_cluster"] == 1 and tot["gap_k_2k"] == 1 and tot["sites"] == 0 and tot["reads_with_sites"] == 0
    assert tot["kmers"] == len(kmers) and tot["kmers_called"] == len(kmers) - 2 * 41
    assert rec.tolist() == [[79, 1, 0, 88]]
    # one miss inside the run and it is a site
    tot, _ = _one(gc.sub(record, 60), keys, called)
    assert tot["gaps_in_cluster"] == 0 and tot["sites"] == 1 and tot["gap_k_2k"] == 1 and tot["misses"] == 31 and tot["hits_cluster"] == 20


def test_min_hits_decides_who_is_assessed(g, k31):
    _, _, keys, _ = k31
    record = gc.hand_records(g)["sub_75"][0]
    at, rec_at = _one(record, keys, m=89)
    above, rec_above = _one(record, keys, m=90)
    assert at["assessed"] == 1 and at["sites"] == 1 and at["windows"] == 120
    assert above["records"] == 1 and all(above[f] == 0 for f in ZERO + ("assessed", "windows"))
    assert rec_at.tolist() == rec_above.tolist() == [[89, 1, 1, 88]]      # the records' own numbers do not depend on it


def test_the_union_rule(g):
    k, kmers, keys, starts = gc.table("k21", g)
    full, called = gc.called_rows("k21", kmers, starts, "half")
    assert len(full) == len(kmers) == len(keys) + 1
    uk, uc = gm.kmer_called(keys, called)
    assert uk.size == len(keys) - 2
    first = {int(kk): int(c) for kk, c in zip(keys[:-2].tolist(), called[:-2].tolist())}
    again_called, again_not = int(keys[-1]), int(keys[-2])
    assert first[again_called] == 0 and first[again_not] == 1            # the rows disagree, both ways round ...
    at = {int(kk): bool(c) for kk, c in zip(uk.tolist(), uc.tolist())}
    assert at[again_called] and at[again_not]                            # ... and any called row calls the k-mer
    assert int(uc.sum()) == int(called[:-2].sum()) + 1


def test_the_device_cases_are_not_vacuous(g):
    """every count the device tests compare is non-zero somewhere, the long records take the general pass, the tile-edge block
    has its gaps where it says"""
    seen = {f: 0 for f in gm.FIELDS}
    for name in ("k31", "k21"):
        k, kmers, keys, starts = gc.table(name, g)
        for how in ("all", "half"):
            _, called = gc.called_rows(name, kmers, starts, how)
            for reads in (gc.mixed_reads(g), gc.one_length_reads(g)):
                tot, rec = gm.gaps_model(gc.block(reads), keys, called, k, 2)
                for f in gm.FIELDS:
                    seen[f] += tot[f]
                assert 0 < tot["assessed"] < tot["records"] == len(reads)
    assert all(seen[f] > 0 for f in gm.FIELDS if f != "long_records"), seen
    _, _, keys, _ = gc.table("k31", g)
    tot, rec = gm.gaps_model(gc.block(gc.long_records(g)), keys, None, 31, 1)
    assert tot["long_records"] == 2 and tot["gap_km1"] >= 10 and tot["gap_k"] > 50 and tot["gap_k_2k"] > 20 and rec[1, 0] > 65535
    blk = gc.tile_edge_block(g)
    state = gm.window_states(blk, keys, None, 31)
    assert (state[1009:1040] == gm.X).all() and state[1008] == gm.C and state[1040] == gm.C
    assert state[2047] == gm.C and (state[2048:2079] == gm.X).all() and state[2079] == gm.C
    assert blk[3072:] == b"\n" and blk[3071:3072] != b"\n"            # record 4 ends at the tile edge
    tot, _ = gm.gaps_model(blk, keys, None, 31, 1)
    assert tot["gap_k"] == 3 and tot["sites"] == 3 and tot["records"] == 4


def test_shards_add_up_on_the_model(g):
    k, kmers, keys, starts = gc.table("k31", g)
    _, called = gc.called_rows("k31", kmers, starts, "half")
    reads = gc.mixed_reads(g)
    whole, _ = gm.gaps_model(gc.block(reads), keys, called, k, 3)
    a, _ = gm.gaps_model(gc.block(reads[:140]), keys, called, k, 3)
    b, _ = gm.gaps_model(gc.block(reads[140:]), keys, called, k, 3)
    assert gm.add(a, b) == whole


def test_hits_are_those_of_read_support(g):
    k, kmers, keys, _ = gc.table("k21", g)
    text = gc.block(gc.mixed_reads(g))
    _, rec = gm.gaps_model(text, keys, None, k, 1)
    assert rec[:, 0].tolist() == rs_model.hits_per_record(text, keys, k).tolist()


# ---------------------------------------------------------------------------------------------- the flag and the file


def test_flag_parsing_and_state():
    import strainscan_amd
    from strainscan_amd import StrainScan, read_reports as rr
    for multi in (False, True):
        ap = argparse.ArgumentParser(prog="x")
        StrainScan.add_arguments(ap, multi=multi)
        base = ["-i", "r.fq", "-d", "DB"]
        assert ap.parse_args(base).divergence == 0
        assert ap.parse_args(base + ["--divergence", "3"]).divergence == 3
        for bad in ("0", "-1", "two", "1.5", "", str(1 << 32)):
            with pytest.raises(SystemExit) as e:
                ap.parse_args(base + ["--divergence", bad])
            assert e.value.code == 2, bad
        args = ap.parse_args(["-i", "a.fq", "-j", "b.fq", "-d", "DB", "--pairs", "--divergence", "2"])
        StrainScan.refuse_pairs_alone(ap, args)                         # --pairs accepts it as its report
    assert rr.DIVERGENCE["m"] == 0
    try:
        strainscan_amd.set_divergence(4)
        assert rr.DIVERGENCE == dict(m=4, rows={}, order={}, skipped=None)
        for bad in (-1, 1.5, "2", True):
            with pytest.raises(ValueError):
                strainscan_amd.set_divergence(bad)
        strainscan_amd.set_divergence(None)
        assert rr.DIVERGENCE["m"] == 0
        strainscan_amd.set_divergence(4)
    finally:
        rr.reset_all()
    assert rr.DIVERGENCE == dict(m=0, rows={}, order={}, skipped=None)
    assert rr.write_divergence(".") is None
    rr.collect_divergence("C1", "no_such_dir", "no_such_report", 31, ["no_such.fq"])      # off: nothing is looked at


def test_commands_refuse_a_bad_value_before_any_input_is_opened(tmp_path):
    for mod in ("strainscan_amd.StrainScan", "strainscan_amd.multi_db"):
        cmd = [sys.executable, "-m", mod, "-i", str(tmp_path / "no_such.fq"), "-d", str(tmp_path / "no_db"), "-o", str(tmp_path / "out"),
               "--divergence", "0"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 2 and "--divergence" in r.stderr, (mod, r.stderr[-500:])
        assert not (tmp_path / "out").exists()


def test_file_text_and_called_rows():
    from strainscan_amd import read_reports as rr
    r = {f: i + 1 for i, f in enumerate(gm.FIELDS)}
    clusters = [("C7", [1, 3], r), ("C2", [2], dict(r, detectable=0))]
    text = rr.divergence_text(clusters)
    assert text == gm.report_text(clusters)
    lines = text.split("\n")
    assert lines[0].split("\t") == list(gm.COLUMNS) and len(gm.COLUMNS) == 19
    row = lines[1].split("\t")
    assert row[:5] == ["C7", "1,3", str(r["kmers"]), str(r["kmers_called"]), str(r["assessed"])]
    assert row[-1] == "%.3f" % (1000.0 * r["sites"] / r["detectable"]) and lines[2].split("\t")[-1] == "-"
    # the union of the called strains' columns, any number of them; explicit zeros do not count
    indptr = np.array([0, 2, 2, 3, 5])
    indices = np.array([0, 2, 1, 2, 3])
    data = np.array([1, 1, 1, 0, 1])
    assert rr.called_rows(indptr, indices, data, 5, [2]).tolist() == [1, 0, 0, 0, 0]
    assert rr.called_rows(indptr, indices, data, 5, [1, 3]).tolist() == [0, 0, 1, 1, 0]
    assert rr.called_rows(indptr, indices, None, 3, [0, 1, 2, 3]).tolist() == [1, 0, 1]
    assert rr.called_rows(indptr, indices, data, 4, list(range(4)) + [40]).tolist() == [1, 0, 1, 1]


def test_abi_names_are_declared_and_built():
    hdr = open(os.path.join(ROOT, "include", "strainscan_hip.h")).read()
    mk = open(os.path.join(ROOT, "strainscan_amd", "csrc", "Makefile")).read()
    from strainscan_amd import _lib
    for name in ("ss_reads_gaps", "ss_reads_gaps_calls"):
        assert name + "(" in hdr and name in _lib.SIGNATURES
    assert "ss_gaps.hip" in mk and "#define SS_GAPS_OUT 18" in hdr
    assert _lib.GAPS_FIELDS == gm.FIELDS and len(_lib.GAPS_FIELDS) == _lib.GAPS_OUT == 18
