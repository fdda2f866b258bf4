"""The model of `--classify_strains` that the strain-set tests hold the device and the command to.

The called strains of a cluster are numbered 1..n (n <= 16) in the order of its report.  row_sets[i] is the MASK of row i of the
table: bit j - 1 is set when strain j has the row's k-mer.

Slots.  label_model's rule with masks: rows that list the same k-mer keep their common mask, 0 where they disagree.

Per record (rs_model's record and hit).  h[j] = the record's hits whose k-mer's mask has bit j - 1; h0 = its hits whose k-mer has
mask 0.  score = the largest h[j].  The record's set is { j : h[j] == score } when score >= m and score > 0, else empty.  A set of
one strain is a unique assignment, a set of several a tie, the empty set unassigned.  The score is kept also where it is below m.

Everything is plain Python over the hits of a record: it is the statement, not a fast one.
"""
import numpy as np

from tests import class_model


def kmer_sets(keys, row_sets):
    """The slot rule: (distinct keys sorted, their masks i64); a key listed under different masks gets 0."""
    return class_model.kmer_nodes(keys, row_sets)


def record_votes(text, keys, row_sets, k):
    """-> ([{mask: hits}] per record of `text`, mask 0 = the hits of k-mers without a strain, n_records)"""
    return class_model.record_hits(text, keys, row_sets, k)


def strain_hits_of(hm, n):
    """{mask: hits} of one record -> [h0, h[1], ..., h[n]]"""
    h = [0] * (n + 1)
    for mask, c in hm.items():
        if mask == 0:
            h[0] += c
        for j in range(1, n + 1):
            if (mask >> (j - 1)) & 1:
                h[j] += c
    return h


def set_of(h, m):
    """[h0, h[1..n]] of one record -> (the set as a mask, the score)"""
    score = max(h[1:]) if len(h) > 1 else 0
    if score < m or score <= 0:
        return 0, score
    return sum(1 << (j - 1) for j in range(1, len(h)) if h[j] == score), score


def popcount(x):
    return bin(int(x)).count("1")


def classify_strains_model(text, keys, row_sets, n, k, m, per=None):
    """-> dict(unique, tied, strain_hits, kmers: u64[n + 1]; set_reads: u64[1 << n]; sets: u16 and scores: u32 per record in
    rs_model.record_ids' numbering; ties).  per: record_votes(...)[0] where the caller has it already."""
    if per is None:
        per, _ = record_votes(text, keys, row_sets, k)
    uniq, tied, hits = (np.zeros(n + 1, np.uint64) for _ in range(3))
    set_reads = np.zeros(1 << n, np.uint64)
    sets, scores = np.zeros(len(per), np.uint16), np.zeros(len(per), np.uint32)
    one = np.uint64(1)
    for i, hm in enumerate(per):
        h = strain_hits_of(hm, n)
        st, sc = set_of(h, m)
        sets[i], scores[i] = st, sc
        hits += np.array(h, np.uint64)
        set_reads[st] += one
        if popcount(st) <= 1:
            uniq[st.bit_length()] += one
        else:
            tied[0] += one
            for j in range(1, n + 1):
                if (st >> (j - 1)) & 1:
                    tied[j] += one
    _, um = kmer_sets(keys, row_sets)
    kmers = np.zeros(n + 1, np.uint64)
    for j in range(1, n + 1):
        kmers[j] = int(((um >> (j - 1)) & 1).sum()) if um.size else 0
    return dict(unique=uniq, tied=tied, strain_hits=hits, kmers=kmers, set_reads=set_reads, sets=sets, scores=scores, ties=int(tied[0]))


def selected(sets, want, how):
    """the records (indices) that ss_reads_select_strains puts in the entry (want, how)"""
    sets = np.asarray(sets, np.int64)
    return np.nonzero((sets & want) != 0 if how else sets == want)[0]


def reads_share(set_reads, n):
    """-> [share of strain j, j = 0..n]: the sum over the sets that hold j, in ascending mask order, of set_reads / |set|; entry
    0: the unassigned records"""
    share = [float(int(set_reads[0]))] + [0.0] * n
    for mask in range(1, len(set_reads)):
        if set_reads[mask]:
            part = int(set_reads[mask]) / popcount(mask)
            for j in range(1, n + 1):
                if (mask >> (j - 1)) & 1:
                    share[j] += part
    return share


def classes_text(clusters):
    """strain_classes.tsv.  clusters: [(table name, [strain names in report order], result dict)] in the order scanned."""
    rows = ["table\tstrain\tkmers\thits\treads_unique\treads_tied\treads_share"]
    for table, names, r in clusters:
        n = len(names)
        share = reads_share(r["set_reads"], n)
        rows.append("%s\tunassigned\t0\t%d\t%d\t0\t%.3f" % (table, int(r["strain_hits"][0]), int(r["unique"][0]), share[0]))
        for j, name in enumerate(names, 1):
            rows.append("%s.%d\t%s\t%d\t%d\t%d\t%d\t%.3f" % (table, j, name, int(r["kmers"][j]), int(r["strain_hits"][j]), int(r["unique"][j]),
                                                           int(r["tied"][j]), share[j]))
    return "\n".join(rows) + "\n"


def sets_text(clusters):
    """strain_sets.tsv: one row per non-empty set with reads, per cluster: reads descending, then mask ascending."""
    rows = ["table\tset\tstrains\treads"]
    for table, names, r in clusters:
        sr = r["set_reads"]
        for mask in sorted((m for m in range(1, len(sr)) if sr[m]), key=lambda m: (-int(sr[m]), m)):
            members = [str(j) for j in range(1, len(names) + 1) if (mask >> (j - 1)) & 1]
            rows.append("%s\t%s\t%d\t%d" % (table, ",".join(members), len(members), int(sr[mask])))
    return "\n".join(rows) + "\n"
