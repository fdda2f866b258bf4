"""The model of `--by_strain` that the labelled read-support tests hold the device and the command to.

Row labels.  A cluster's matrix has a row per k-mer of all_kmer.fasta and a column per strain.  Given the called columns c_1 ...
c_L (in the order of StrainVote.report), row r has label j when it is 1 in column c_j and 0 in every other called column; every
other row -- shared between called strains, or in none of them -- has label 0.  Uncalled columns are not looked at: a k-mer that
a called strain shares only with strains that were not called counts for it.

Slots.  all_kmer.fasta may list a k-mer twice; the rows then share one slot of the table.  The slot's label is the rows' common
label, 0 where they disagree.

Everything label j reports equals what rs_model gives for the sub-table "k-mers with label j": labeled_support_model is
rs_model.support_model on each label's sub-table.
"""
import numpy as np

from tests import rs_model


def row_labels(matrix, called):
    """matrix: dense 0/1 array [n_rows, n_strains]; called: the called columns in report order -> np.uint8[n_rows]."""
    m = np.asarray(matrix)
    sub = (m[:, list(called)] != 0).astype(np.int64).reshape(m.shape[0], len(called))
    out = np.zeros(m.shape[0], np.uint8)
    for r in range(m.shape[0]):
        ones = [j for j in range(len(called)) if sub[r, j]]
        if len(ones) == 1:
            out[r] = ones[0] + 1
    return out


def kmer_labels(keys, labels):
    """The slot rule: (distinct keys, their labels) for rows with `keys` (np.uint64) and `labels`; a key listed under different
    labels gets 0."""
    keys = np.asarray(keys, np.uint64)
    labels = np.asarray(labels, np.uint8)
    if not keys.size:
        return keys, labels
    order = np.argsort(keys, kind="stable")
    sk, sl = keys[order], labels[order]
    first = np.nonzero(np.concatenate(([True], sk[1:] != sk[:-1])))[0]
    lo, hi = np.minimum.reduceat(sl, first), np.maximum.reduceat(sl, first)
    return sk[first], np.where(lo == hi, lo, 0).astype(np.uint8)


def label_keys(keys, labels, j):
    """the sub-table of label j: its distinct keys"""
    uk, ul = kmer_labels(keys, labels)
    return uk[ul == j]


def labeled_hits_per_record(text, keys, labels, n_labels, k):
    """-> np.int64[n_labels + 1, n_records]: row j = rs_model.hits_per_record(text, label_keys(keys, labels, j), k), row 0 the
    hits of label 0's k-mers.  One pass over the windows for all labels: a window's label is looked up once (what rs_model does
    per sub-table with np.isin; tests/test_label_host.py holds the two to each other)."""
    uk, ul = kmer_labels(keys, labels)
    order = np.argsort(uk)
    uk, ul = uk[order], ul[order]
    ids, n_rec = rs_model.record_ids(text)
    key, live = rs_model.window_keys(text, k)
    out = np.zeros((n_labels + 1, n_rec), np.int64)
    if not uk.size or not key.size:
        return out
    at = np.minimum(np.searchsorted(uk, key), uk.size - 1)
    hit = live & (uk[at] == key)
    rec, lab = ids[:hit.size][hit], ul[at][hit].astype(np.int64)
    np.add.at(out, (lab, rec), 1)
    return out


def labeled_support_model(text, keys, labels, n_labels, k, n_bins=65):
    """-> (hist u64[n_labels, n_bins], hits [n_labels], kmers [n_labels]): rs_model.support_model on each label's sub-table."""
    per = labeled_hits_per_record(text, keys, labels, n_labels, k)
    _, ul = kmer_labels(keys, labels)
    hist = np.stack([rs_model.histogram(per[j], n_bins) for j in range(1, n_labels + 1)])
    return hist, [int(per[j].sum()) for j in range(1, n_labels + 1)], [int((ul == j).sum()) for j in range(1, n_labels + 1)]
