"""The model of `--classify_reads` that the read-class tests hold the device and the command to.

Nodes are numbered 1..n; row_node[i] in 0..n says whose k-mer row i of the table is (0: nobody's), parent[v] (v in 1..n; entry 0
is not read) is v's parent or 0.  The parents must describe a forest; parent[v] < v is not required.

Slots.  label_model's rule with integer nodes: rows that list the same k-mer keep their common node, 0 where they disagree.

Per record (rs_model's record and hit).  h[v] = the record's hits whose k-mer has node v.  For every v with h[v] > 0, score(v) =
the sum of h[u] over the path from v's root to v, v included.  The class is the node with the largest score; several nodes with
that score (they are never on one path) give their lowest common ancestor, 0 when they stand in different trees.  A largest score
below m, or no hit with a node, gives 0.

Everything is plain Python over the hits of a record: it is the statement, not a fast one.
"""
import numpy as np

from tests import rs_model


def kmer_nodes(keys, row_node):
    """The slot rule: (distinct keys sorted, their nodes i64); a key listed under different nodes gets 0."""
    keys = np.asarray(keys, np.uint64)
    nodes = np.asarray(row_node, np.int64)
    if not keys.size:
        return keys, nodes
    order = np.argsort(keys, kind="stable")
    sk, sn = keys[order], nodes[order]
    first = np.nonzero(np.concatenate(([True], sk[1:] != sk[:-1])))[0]
    lo, hi = np.minimum.reduceat(sn, first), np.maximum.reduceat(sn, first)
    return sk[first], np.where(lo == hi, lo, 0).astype(np.int64)


def check_forest(parent, n_nodes):
    """False for a parent above n_nodes or a cycle."""
    parent = [int(p) for p in parent]
    if any(parent[v] > n_nodes or parent[v] < 0 for v in range(1, n_nodes + 1)):
        return False
    state = [0] * (n_nodes + 1)            # 0 unseen, 1 on the current walk, 2 known to reach a root
    for v in range(1, n_nodes + 1):
        walk, u = [], v
        while u and state[u] == 0:
            state[u] = 1
            walk.append(u)
            u = parent[u]
        if u and state[u] == 1:
            return False
        for w in walk:
            state[w] = 2
    return True


def root_path(parent, v):
    """[v, parent[v], ..., root]"""
    out = []
    while v:
        out.append(v)
        v = int(parent[v])
    return out


def lca(parent, a, b):
    """the lowest common ancestor of a and b, 0 when they share none"""
    on_a = set(root_path(parent, a))
    for u in root_path(parent, b):
        if u in on_a:
            return u
    return 0


def classify_hits(h, parent, m):
    """h: {node: hits} of one record, nodes >= 1 -> (class, the best score, whether the class came from a tie)"""
    best, tied = 0, []
    for v in sorted(h):
        sc = sum(h.get(u, 0) for u in root_path(parent, v))
        if sc > best:
            best, tied = sc, [v]
        elif sc == best:
            tied.append(v)
    if not tied or best < m:
        return 0, best, False
    cls = tied[0]
    for v in tied[1:]:
        cls = lca(parent, cls, v) if cls else 0
    return cls, best, len(tied) > 1


def record_hits(text, keys, row_node, k):
    """-> ([{node: hits}] per record of `text`, node 0 = hits of k-mers without a node, n_records)"""
    uk, un = kmer_nodes(keys, row_node)
    ids, n_rec = rs_model.record_ids(text)
    key, live = rs_model.window_keys(text, k)
    per = [dict() for _ in range(n_rec)]
    if not uk.size or not key.size:
        return per, n_rec
    at = np.minimum(np.searchsorted(uk, key), uk.size - 1)
    hit = live & (uk[at] == key)
    n1 = int(un.max()) + 1
    pair, cnt = np.unique(ids[:hit.size][hit] * n1 + un[at][hit], return_counts=True)      # (record, node) pairs and their hits
    for q, c in zip(pair.tolist(), cnt.tolist()):
        per[q // n1][q % n1] = c
    return per, n_rec


def classes_detail(text, keys, row_node, parent, k, m, per=None):
    """-> [(class, best score, tie, h)] per record; per: record_hits(...)[0] where the caller has it already"""
    if per is None:
        per, _ = record_hits(text, keys, row_node, k)
    out = []
    for h in per:
        hv = {v: c for v, c in h.items() if v}
        out.append(classify_hits(hv, parent, m) + (h,))
    return out


def classes_per_record(text, keys, row_node, parent, k, m, per=None):
    """-> np.uint32[n_records]: the class of every record of `text`, in rs_model.record_ids' numbering"""
    return np.array([d[0] for d in classes_detail(text, keys, row_node, parent, k, m, per)], np.uint32)


def classify_model(text, keys, row_node, parent, n_nodes, k, m, per=None):
    """-> (direct u64[n_nodes + 1], node_hits u64[n_nodes + 1], kmers u64[n_nodes + 1])"""
    direct = np.zeros(n_nodes + 1, np.uint64)
    node_hits = np.zeros(n_nodes + 1, np.uint64)
    for cls, _, _, h in classes_detail(text, keys, row_node, parent, k, m, per):
        direct[cls] += np.uint64(1)
        for v, c in h.items():
            node_hits[v] += np.uint64(c)
    _, un = kmer_nodes(keys, row_node)
    kmers = np.bincount(un, minlength=n_nodes + 1).astype(np.uint64)[:n_nodes + 1]
    kmers[0] = 0
    return direct, node_hits, kmers


def clade_sums(direct, parent, n_nodes):
    """reads_clade: direct summed over every node and all below it -> list[n_nodes + 1] (entry 0: direct[0])"""
    clade = [int(x) for x in direct]
    for v in range(1, n_nodes + 1):
        for u in root_path(parent, v)[1:]:
            clade[u] += int(direct[v])
    return clade


def report_text(node_ids, parent_ids, leaves, direct, node_hits, kmers):
    """read_classes.tsv.  node_ids: ascending ids, node v (1-based) = node_ids[v - 1]; parent_ids: {id: parent id or None};
    leaves: the ids that are clusters."""
    n = len(node_ids)
    num = {nid: i + 1 for i, nid in enumerate(node_ids)}
    parent = [0] * (n + 1)
    for nid in node_ids:
        p = parent_ids.get(nid)
        parent[num[nid]] = num[p] if p is not None else 0
    clade = clade_sums(direct, parent, n)
    rows = ["node\tparent\tcluster\tkmers\thits\treads_direct\treads_clade",
            "unclassified\t-\t-\t0\t%d\t%d\t%d" % (int(node_hits[0]), int(direct[0]), int(direct[0]))]
    for v, nid in enumerate(node_ids, 1):
        p = parent_ids.get(nid)
        rows.append("%s\t%s\t%s\t%d\t%d\t%d\t%d" % (nid, "-" if p is None else p, "C%s" % nid if nid in leaves else "-", int(kmers[v]),
                                                   int(node_hits[v]), int(direct[v]), clade[v]))
    return "\n".join(rows) + "\n"
