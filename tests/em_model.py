"""The model of `--em_strains` that the EM tests hold the device and the command to: plain float64 numpy.

The called strains of a cluster are numbered 1..L (L <= 16); a SET is a non-zero mask, bit j - 1 for strain j; n[s] is the reads
whose set is masks[s] (the unassigned reads, mask 0, take no part) and N their sum, taken in integers.

  active     strain j is active when some set with n[s] > 0 holds j; an inactive strain has rho_j = 0 throughout
  start      rho_j = 1 / (the number of active strains)
  iteration  for every set with n[s] > 0: d[s] = the sum of rho_i over its strains, i ascending; a set with d[s] == 0 contributes
             nothing; rho'_j = rho_j * (the sum over the sets that hold j of n[s] / d[s]) / N -- (1/N) * sum of n[s] * rho_j / d[s]
             with the common factor taken out of the sum, which is how the header states it and the device computes it
  stopping   after iteration t: t == max_iter, or the largest |rho'_j - rho_j| < tol (tol == 0: exactly max_iter iterations)
  N == 0     rho = 0, iters = 0
  theta_j    (rho_j / kmers[j]) / the sum of that over the strains with kmers > 0; 0 where the sum is 0

The sum over the sets is taken one set after the other (np.cumsum adds strictly in sequence), ascending by default and descending
on request: the difference between the two is what a third order -- the device's tree -- may differ by, and the tests' tolerance
is taken from it.
"""
import numpy as np

from tests import boot_model

QUANTILES = (0.025, 0.975)


def em(counts, masks, n_strains, max_iter, tol, descending=False):
    """counts: [n_sets] integers, masks: [n_sets] -> (rho f64[n_strains], iters)"""
    counts = [int(c) for c in counts]
    masks = [int(m) for m in masks]
    L = int(n_strains)
    if descending:
        counts, masks = counts[::-1], masks[::-1]
    total = sum(counts)
    rho = np.zeros(L, np.float64)
    if total == 0:
        return rho, 0
    member = ((np.array(masks, np.int64)[:, None] >> np.arange(L)[None, :]) & 1).astype(bool)
    n = np.array(counts, np.float64)
    has = n > 0
    active = member[has].any(axis=0)
    rho[active] = 1.0 / int(active.sum())
    N = np.float64(total)
    it = 0
    while True:
        d = np.zeros(len(masks), np.float64)
        for j in range(L):                                            # i ascending
            d = d + np.where(member[:, j], rho[j], 0.0)
        use = has & (d > 0)
        q = np.divide(n, d, out=np.zeros_like(n), where=use)
        terms = np.where(member & use[:, None], q[:, None], 0.0)
        sums = np.cumsum(terms, axis=0)[-1]                           # one set after the other
        new = rho * sums / N
        delta = float(np.abs(new - rho).max())
        rho = new
        it += 1
        if it >= max_iter or delta < tol:
            return rho, it


def em_batch(counts, masks, n_strains, max_iter, tol, descending=False):
    """counts: [n_vec][n_sets] -> (rho [n_vec, n_strains], iters u32[n_vec]); vectors that are equal are solved once"""
    counts = np.asarray(counts)
    rho = np.zeros((counts.shape[0], n_strains), np.float64)
    iters = np.zeros(counts.shape[0], np.uint32)
    done = {}
    for v in range(counts.shape[0]):
        key = counts[v].tobytes()
        if key not in done:
            done[key] = em(counts[v], masks, n_strains, max_iter, tol, descending)
        rho[v], iters[v] = done[key]
    return rho, iters


def abundance(rho, kmers):
    """theta of one rho vector"""
    per = [float(r) / int(k) if int(k) > 0 else 0.0 for r, k in zip(rho, kmers)]
    tot = 0.0
    for p in per:
        tot += p
    return [p / tot if tot != 0 else 0.0 for p in per]


def quantile_index(q, b):
    return int(np.floor(q * (b - 1) + 0.5))


def replicate_set_counts(L, text, sets, n_strains, seed, first, n_rep):
    """u64[n_rep, 1 << n_strains]: row j = the sum, over the records of `text` whose set (`sets`, per record in the model's
    numbering: strain_set_model.classify_strains_model(...)["sets"]) is m, of boot_model's weight for replicate first + j.
    `L` is strainscan_amd._lib (the digest of a record runs on the host)."""
    out = np.zeros((n_rep, 1 << n_strains), np.uint64)
    recs = boot_model.records_of(text)
    assert len(recs) == len(sets)
    if not recs:
        return out
    keys = L.flat_record_keys(b"\n".join(recs) + b"\n")
    for j in range(n_rep):
        w = boot_model.weights_of_keys(keys[:, 1], seed, first + j)
        out[j] = np.bincount(np.asarray(sets, np.int64), weights=w, minlength=1 << n_strains).astype(np.uint64)
    return out


def replicate_weights(L, text, seed, first, n_rep):
    """i64[n_rep, records]: boot_model's weights of every record of `text`"""
    recs = boot_model.records_of(text)
    if not recs:
        return np.zeros((n_rep, 0), np.int64)
    keys = L.flat_record_keys(b"\n".join(recs) + b"\n")
    return np.stack([boot_model.weights_of_keys(keys[:, 1], seed, first + j) for j in range(n_rep)])


def compact(vectors):
    """[V, 1 << n] set counts -> (counts [V, S], masks [S]): the non-zero masks with reads in any vector, ascending"""
    vectors = np.asarray(vectors, np.uint64).copy()
    vectors[:, 0] = 0
    masks = np.flatnonzero(vectors.any(axis=0))
    return vectors[:, masks], masks.astype(np.uint16)


def em_table(clusters, b, max_iter=1000, tol=1e-9):
    """The rows of strain_em.tsv as lists, numbers unformatted.  clusters: [(table, [(n, name)], kmers[L], enet texts[L], vectors
    [B + 1, 1 << L] set counts)] -> [[table.n, name, kmers, N, rho_j * N, rho_j, theta_j, lo or None, hi or None, present or None,
    enet, iters]]"""
    rows = []
    for table, called, kmers, enet, vectors in clusters:
        n = len(called)
        counts, masks = compact(vectors)
        if masks.size:
            rho, iters = em_batch(counts, masks, n, max_iter, tol)
        else:
            rho, iters = np.zeros((b + 1, n)), np.zeros(b + 1, np.uint32)
        theta = np.array([abundance(r, kmers) for r in rho])
        N = int(counts[0].sum())
        for j, (num, name) in enumerate(called):
            lo = hi = present = None
            if b:
                ts = np.sort(theta[1:, j])
                lo, hi = (float(ts[quantile_index(q, b)]) for q in QUANTILES)
                present = int((rho[1:, j] > 0).sum())
            rows.append(["%s.%d" % (table, num), name, int(kmers[j]), N, float(rho[0, j]) * N, float(rho[0, j]), float(theta[0, j]), lo, hi, present,
                         enet[j], int(iters[0])])
    return rows
