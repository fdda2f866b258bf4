"""`--by_strain` on the host: the row labels of tests/label_model.py on hand-written matrices, read_reports.strain_row_labels (the CSR form the
command uses) against them, the slot rule for a k-mer listed twice, the labelled model against rs_model on each label's sub-table,
the text of strain_support.tsv, and the flag parser."""
import numpy as np
import pytest

from tests import label_model, rs_model


def _csr_labels(dense, called, n_rows=None):
    import scipy.sparse as sp
    from strainscan_amd import read_reports
    m = sp.csr_matrix(np.asarray(dense, np.int8))
    return read_reports.strain_row_labels(m.indptr, m.indices, m.data, m.shape[0] if n_rows is None else n_rows, called)


#            s0 s1 s2 s3
MATRIX = [[1, 0, 0, 0],      # 0: only s0
          [0, 1, 0, 0],      # 1: only s1
          [1, 1, 0, 0],      # 2: s0 and s1
          [1, 0, 1, 0],      # 3: s0 and s2
          [0, 0, 1, 1],      # 4: s2 and s3
          [0, 0, 0, 1],      # 5: only s3
          [1, 1, 1, 1],      # 6: all
          [0, 0, 0, 0]]      # 7: none


@pytest.mark.parametrize("called,want", [
    ([0], [1, 0, 1, 1, 0, 0, 1, 0]),                 # one called strain: every row it has, shared with uncalled strains or not
    ([0, 1], [1, 2, 0, 1, 0, 0, 0, 0]),              # two with shared rows: rows 2 and 6 are nobody's; row 3 counts for s0 (s2 is not called)
    ([1, 0], [2, 1, 0, 2, 0, 0, 0, 0]),              # labels follow the order of the report
    ([2, 3], [0, 0, 0, 1, 0, 2, 0, 0]),              # rows 4 and 6 shared; rows 0..2 only in uncalled strains: label 0
    ([3, 0, 2], [2, 0, 2, 0, 0, 1, 0, 0]),           # s2 has no row of its own among the called: a label without rows
])
def test_row_labels(called, want):
    got = label_model.row_labels(MATRIX, called)
    assert got.dtype == np.uint8 and got.tolist() == want
    assert _csr_labels(MATRIX, called).tolist() == want


def test_row_labels_random_matrix_csr_equals_dense():
    rs = np.random.RandomState(3)
    dense = (rs.random_sample((500, 12)) < 0.3).astype(np.int8)
    for called in ([4], [0, 11], [7, 2, 9, 5], list(range(12))):
        want = label_model.row_labels(dense, called)
        assert _csr_labels(dense, called).tolist() == want.tolist()
        assert set(want.tolist()) <= set(range(len(called) + 1))
    # a table with more (or fewer) rows than the matrix: the rows beyond it have no label
    assert _csr_labels(dense, [0, 11], n_rows=510).tolist() == label_model.row_labels(dense, [0, 11]).tolist() + [0] * 10
    assert _csr_labels(dense, [0, 11], n_rows=490).tolist() == label_model.row_labels(dense, [0, 11]).tolist()[:490]


def test_cluster_csr_arrays_stored_and_deflated(tmp_path):
    """a .npz whose members are stored is mapped, one that is deflated is read the solver's way: the same arrays, the same labels"""
    import scipy.sparse as sp
    from strainscan_amd import read_reports
    rs = np.random.RandomState(9)
    dense = (rs.random_sample((300, 7)) < 0.4).astype(np.int8)
    dense[5] = 0                                         # an empty row
    m = sp.csr_matrix(dense)
    stored, deflated = str(tmp_path / "stored.npz"), str(tmp_path / "deflated.npz")
    np.savez(stored, indices=m.indices, indptr=m.indptr, format=np.array(b"csr"), shape=np.array(m.shape), data=m.data)
    sp.save_npz(deflated, m, compressed=True)
    want = label_model.row_labels(dense, [6, 1, 3])
    for path, mapped in ((stored, True), (deflated, False)):
        indptr, indices, data = read_reports.cluster_csr_arrays(path)
        assert isinstance(indices, np.memmap) == mapped
        assert (np.asarray(indptr) == m.indptr).all() and (np.asarray(indices) == m.indices).all() and (np.asarray(data) == m.data).all()
        assert read_reports.strain_row_labels(indptr, indices, data, 300, [6, 1, 3]).tolist() == want.tolist()


def test_slot_rule_for_a_kmer_listed_twice():
    keys = np.array([5, 9, 5, 7, 9, 7, 3], np.uint64)
    labels = np.array([1, 2, 1, 0, 1, 3, 2], np.uint8)
    uk, ul = label_model.kmer_labels(keys, labels)
    got = dict(zip(uk.tolist(), ul.tolist()))
    assert got == {5: 1, 9: 0, 7: 0, 3: 2}             # 5: common label; 9: 2 and 1 disagree; 7: 0 and 3 disagree
    assert label_model.label_keys(keys, labels, 1).tolist() == [5]
    assert label_model.label_keys(keys, labels, 3).tolist() == []


def test_labeled_model_is_rs_model_on_each_sub_table():
    rs = np.random.RandomState(5)
    lut = np.frombuffer(b"ACGT", np.uint8)
    g = lut[rs.randint(0, 4, size=4000)].tobytes()
    kmers = [g[i:i + 21] for i in range(0, 3000, 2)]
    kmers += kmers[:50]                                # listed twice
    keys = rs_model.encode_kmers(kmers, 21)
    labels = rs.randint(0, 4, size=len(kmers)).astype(np.uint8)
    recs = [g[s:s + ln] for s, ln in zip(rs.randint(0, 3800, size=300), rs.randint(1, 200, size=300))]
    recs[7] = recs[7][:10] + b"N" + recs[7][11:]
    recs[9] = recs[9].lower()
    text = b"\n".join(recs) + b"\n\n" + g[100:300] + b"\n"
    per = label_model.labeled_hits_per_record(text, keys, labels, 3, 21)
    hist, hits, nk = label_model.labeled_support_model(text, keys, labels, 3, 21)
    for j in (1, 2, 3):
        sub = label_model.label_keys(keys, labels, j)
        assert (per[j] == rs_model.hits_per_record(text, sub, 21)).all()
        h, t = rs_model.support_model(text, sub, 21)
        assert (hist[j - 1] == h).all() and hits[j - 1] == t and nk[j - 1] == sub.size
    assert per.sum() == rs_model.hits_per_record(text, np.unique(keys), 21).sum()
    assert per[0].sum() > 0 and min(hits) > 0


def test_strain_support_text():
    from strainscan_amd import read_reports
    hist = [0] * 65
    hist[0], hist[1], hist[3], hist[20], hist[64] = 90, 4, 3, 2, 1
    text = read_reports.strain_support_text([("C12.1", "GCF_000123", 4321, 100, 999, hist), ("C12.2", "GCF_000456", 0, 100, 0, [100] + [0] * 64)])
    assert text == ("table\tstrain\tkmers\treads\thits\tge1\tge2\tge4\tge8\tge16\tge32\tge64\n"
                    "C12.1\tGCF_000123\t4321\t100\t999\t10\t6\t3\t3\t3\t1\t1\n"
                    "C12.2\tGCF_000456\t0\t100\t0\t0\t0\t0\t0\t0\t0\t0\n")


def test_called_strains_of_a_report(tmp_path):
    from strainscan_amd import read_reports
    from strainscan_amd.Vote_Strain_L2_Lasso_new_sp import STRAINVOTE_HEADER
    p = tmp_path / "StrainVote.report"
    p.write_text(STRAINVOTE_HEADER + "1\tGCF_A\tC7\t0.7\t8.0\t9.3\t0.99\t1/2\t1\t0.9\t*\n"
                 "2\tGCF_B (With_ExtraRegion_covered)\tC7\t0.3\t3.1\t3.6\t0.9\t1/2\t1\t0.7\t\n")
    assert read_reports.called_strains(str(p)) == [(1, "GCF_A"), (2, "GCF_B")]


@pytest.mark.parametrize("mod", ["StrainScan", "multi_db"])
def test_by_strain_alone_is_refused_before_any_input_is_opened(mod, capsys, tmp_path):
    import importlib
    m = importlib.import_module("strainscan_amd." + mod)
    argv = ["-i", str(tmp_path / "no_such.fq"), "-d", str(tmp_path / "no_such_db"), "-o", str(tmp_path / "out"), "--by_strain"]
    with pytest.raises(SystemExit) as e:
        m.main(argv)
    assert e.value.code == 2
    assert "--by_strain needs --read_support and/or -x" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_by_strain_parses_with_either_companion():
    import argparse
    from strainscan_amd import StrainScan
    ap = argparse.ArgumentParser()
    StrainScan.add_arguments(ap)
    for extra in (["--read_support"], ["-x", "4"], ["--read_support", "-x", "4"]):
        args = ap.parse_args(["-i", "a", "-d", "b", "--by_strain"] + extra)
        StrainScan.refuse_by_strain_alone(ap, args)
        assert args.by_strain is True
    assert ap.parse_args(["-i", "a", "-d", "b"]).by_strain is False
