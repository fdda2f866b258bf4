"""The model of `--divergence` (ss_reads_gaps) that the gap tests hold the device and the command to.

Slots.  A k-mer of the table is CALLED when any of the rows that list it is called (row_called None: every row is): the union of
its rows, not label_model's agree-or-zero rule.

Per record (rs_model's record).  Window p is valid when its k bytes are all in ACGTacgt; a valid window is C (its k-mer is a called
k-mer), T (a k-mer of the table that is not called) or X (neither), an invalid one is I.  A gap is a maximal run of T / X windows
with a C window directly before it and directly behind it; it is in-cluster when all of it is T; it is a site when its length g is
in k - 1 .. 2 k - 1 and it is not in-cluster.  A stretch is a maximal run of valid windows; detectable = the sum over the stretches
that hold a C of max(0, last C - first C - k).  A record is assessed when it has at least min_hits C windows, and only assessed
records add to the totals.

The windows of the whole text are classified at once and run-length encoded: a window that holds a '\\n' is I, so no run crosses
records.
"""
import numpy as np

from tests import rs_model

FIELDS = ("records", "assessed", "windows", "hits_called", "hits_cluster", "misses", "gap_lt", "gap_km1", "gap_k", "gap_k_2k", "gap_ge2k",
          "gaps_in_cluster", "sites", "reads_with_sites", "detectable", "kmers", "kmers_called", "long_records")
LONG = 4095          # records of more bytes take the device's general pass (long_records)
I, X, T, C = 0, 1, 2, 3


def kmer_called(keys, row_called=None):
    """The slot rule: (distinct keys sorted, bool: any of the key's rows is called)."""
    keys = np.asarray(keys, np.uint64)
    called = np.ones(keys.size, bool) if row_called is None else np.asarray(row_called) != 0
    assert called.shape == keys.shape
    if not keys.size:
        return keys, called
    order = np.argsort(keys, kind="stable")
    sk, sc = keys[order], called[order]
    first = np.nonzero(np.concatenate(([True], sk[1:] != sk[:-1])))[0]
    return sk[first], np.maximum.reduceat(sc.astype(np.uint8), first).astype(bool)


def window_states(text, keys, row_called, k):
    """-> u8[len(text)]: I, X, T or C per byte of `text`, the state of the window that starts there"""
    state = np.zeros(len(text), np.uint8)
    uk, uc = kmer_called(keys, row_called)
    key, live = rs_model.window_keys(text, k)
    if not key.size:
        return state
    st = np.where(live, X, I).astype(np.uint8)
    if uk.size:
        at = np.minimum(np.searchsorted(uk, key), uk.size - 1)
        hit = live & (uk[at] == key)
        st[hit] = np.where(uc[at][hit], C, T)
    state[:st.size] = st
    return state


def gap_class(g, k):
    return 0 if g < k - 1 else 1 if g == k - 1 else 2 if g == k else 3 if g < 2 * k else 4


def gaps_model(text, keys, row_called, k, min_hits):
    """-> (dict of FIELDS, i64[n_records, 4]: hits_called, gaps, sites, detectable per record in rs_model.record_ids' numbering)"""
    ids, n_rec = rs_model.record_ids(text)
    state = window_states(text, keys, row_called, k)
    per = np.zeros((n_rec, 11), np.int64)          # C, T, X, the five classes, in-cluster, sites, detectable
    lens = np.bincount(ids[ids >= 0], minlength=n_rec) if n_rec else np.zeros(0, np.int64)
    if state.size and n_rec:
        live = state != I
        for col, s in ((0, C), (1, T), (2, X)):
            per[:, col] = np.bincount(ids[state == s], minlength=n_rec)
        # runs of equal kind: C, gap material (T or X), I
        kind = np.where(state == C, 2, np.where(live, 1, 0))
        start = np.nonzero(np.concatenate(([True], kind[1:] != kind[:-1])))[0]
        end = np.concatenate((start[1:], [kind.size]))
        rk = kind[start]
        nx = np.concatenate(([0], np.cumsum(state == X)))
        for r in np.nonzero(rk == 1)[0]:
            if r == 0 or r == rk.size - 1 or rk[r - 1] != 2 or rk[r + 1] != 2:
                continue
            g, rec = int(end[r] - start[r]), ids[start[r]]
            assert rec >= 0 and ids[end[r]] == rec and ids[start[r] - 1] == rec
            per[rec, 3 + gap_class(g, k)] += 1
            if nx[end[r]] == nx[start[r]]:
                per[rec, 8] += 1
            elif k - 1 <= g < 2 * k:
                per[rec, 9] += 1
        # stretches: runs of valid windows
        sstart = np.nonzero(live & np.concatenate(([True], ~live[:-1])))[0]
        send = np.nonzero(live & np.concatenate((~live[1:], [True])))[0]
        cpos = np.nonzero(state == C)[0]
        for a, b in zip(sstart.tolist(), send.tolist()):
            lo, hi = np.searchsorted(cpos, a), np.searchsorted(cpos, b, side="right")
            if hi > lo:
                per[ids[a], 10] += max(0, int(cpos[hi - 1] - cpos[lo]) - k)
    assessed = per[:, 0] >= min_hits
    tot = per[assessed].sum(axis=0) if n_rec else np.zeros(11, np.int64)
    uk, uc = kmer_called(keys, row_called)
    out = dict(records=n_rec, assessed=int(assessed.sum()), windows=int(tot[0] + tot[1] + tot[2]), hits_called=int(tot[0]), hits_cluster=int(tot[1]),
               misses=int(tot[2]), gap_lt=int(tot[3]), gap_km1=int(tot[4]), gap_k=int(tot[5]), gap_k_2k=int(tot[6]), gap_ge2k=int(tot[7]),
               gaps_in_cluster=int(tot[8]), sites=int(tot[9]), reads_with_sites=int((assessed & (per[:, 9] > 0)).sum()), detectable=int(tot[10]),
               kmers=int(uk.size), kmers_called=int(uc.sum()), long_records=int((lens > LONG).sum()))
    rec = np.stack([per[:, 0], per[:, 3:8].sum(axis=1), per[:, 9], per[:, 10]], axis=1) if n_rec else np.zeros((0, 4), np.int64)
    return out, rec


def per_kb(sites, detectable):
    return "%.3f" % (1000.0 * sites / detectable) if detectable else "-"


COLUMNS = ("table", "strains", "kmers", "kmers_called", "reads", "windows", "hits_called", "hits_cluster", "misses", "gap_lt", "gap_km1", "gap_k",
           "gap_k_2k", "gap_ge2k", "gaps_in_cluster", "sites", "reads_with_sites", "detectable", "per_kb")


def report_text(clusters):
    """strain_divergence.tsv.  clusters: [(table name, [report numbers of the called strains], totals dict)] in the order scanned."""
    rows = ["\t".join(COLUMNS)]
    for table, numbers, r in clusters:
        vals = [table, ",".join(str(x) for x in numbers), r["kmers"], r["kmers_called"], r["assessed"]]
        vals += [r[c] for c in COLUMNS[5:18]] + [per_kb(r["sites"], r["detectable"])]
        rows.append("\t".join(str(v) for v in vals))
    return "\n".join(rows) + "\n"


def add(a, b):
    """the totals of two sets against one table, added up as those of their union"""
    out = {f: a[f] + b[f] for f in FIELDS}
    out["kmers"], out["kmers_called"] = a["kmers"], a["kmers_called"]
    return out
