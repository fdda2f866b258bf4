"""The touched-node exchange on the device (ss_nodes.hip: pack_offsets_kernel, pack_copy_kernel, harvest_kernel, the DENSE
node_reduce_kernel, the flag copies, ss_nodes_clear_dev) and the row vector's round trip (gather_rows_kernel /
scatter_rows_kernel of ss_scan.hip), driven in one process on injected counts and compared with tests/nodemodel.py -- the
model dist.exchange_touched's protocol test runs over -- and with the oracle's match_node.  Bit-exact: integer work."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.nodemodel import NumpyNodes

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_BASE = 200_000
DUP_BLOCK = (100_000, 100_500)      # rows whose keys are repeated later: an all-invalid stretch
N_DUP_RANDOM = 300                  # ... and single ones scattered over the first 60 000 rows
SENTINEL = 0x5EA15EA1
STAT_FIELDS = ("length", "n_pos", "n_kept", "sum_kept", "median2")


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _make_keys(n_base, dup_block, n_dup_random, seed):
    """Random 62-bit keys; the keys of some rows come again at the end, so the earlier copies are invalid rows."""
    rs = np.random.RandomState(seed)
    keys = np.unique(rs.randint(0, 1 << 62, size=n_base + 1000, dtype=np.uint64))
    rs.shuffle(keys)
    keys = keys[:n_base]
    assert keys.size == n_base
    dup = np.concatenate([np.arange(*dup_block), np.sort(rs.choice(min(60_000, dup_block[0]), n_dup_random, replace=False))])
    return np.concatenate([keys, keys[dup]]), dup


@pytest.fixture(scope="module")
def table(L):
    """-> (db, valid): one table for the module; every test loads the counts it needs."""
    keys, dup = _make_keys(N_BASE, DUP_BLOCK, N_DUP_RANDOM, 2024)
    db = L.KmerDB(keys, np.ones(keys.size, np.uint8), 31, True)
    valid = db.row_valid.copy()
    assert keys.size % 256 != 0
    want_valid = np.ones(keys.size, np.uint8)
    want_valid[dup] = 0                                    # the LAST row of a k-mer owns it
    assert np.array_equal(valid, want_valid) and int((valid == 0).sum()) == dup.size > 0
    yield db, valid
    db.close()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    """uint32 / int32 numpy array -> int32 tensor on the device."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _load(db, counts):
    import torch
    t = _dev(counts)
    db.load_counts_rows_dev(t.data_ptr(), _stream())
    torch.cuda.synchronize()


def _stats(st):
    return [tuple(int(s[f]) for f in STAT_FIELDS) for s in st]


def _oracle_stats(counts, valid, lists):
    from oracle import oracle as orc
    out = []
    for rows in lists:
        o = orc.match_node(counts, valid, np.asarray(rows, np.int64))
        out.append((o["length"], o["n_pos"], o["n_kept"], o["sum_kept"], int(round(2 * o["median"])) if o["n_pos"] else 0))
    return out


class _Dev:
    """The ss_nodes_* exchange calls of one bound NodeSet on numpy arrays (what dist._NodeExchange does on tensors)."""

    def __init__(self, L, ns):
        self.L, self.ns, self.n_nodes, self.n_positions = L, ns, ns.n_nodes, int(ns.n_rows_total)

    def _check(self, rc, where):
        import torch
        self.L.check(rc, where)
        torch.cuda.synchronize()

    def flags_set(self, flags):
        t = _dev(np.asarray(flags, np.int32)) if self.n_nodes else _dev(np.zeros(1, np.int32))
        self._check(self.L.lib().ss_nodes_touched_set_dev(self.ns._h, t.data_ptr(), _stream()), "ss_nodes_touched_set_dev")

    def flags_get(self):
        t = _dev(np.full(max(1, self.n_nodes), 7, np.int32))
        self._check(self.L.lib().ss_nodes_touched_get_dev(self.ns._h, t.data_ptr(), _stream()), "ss_nodes_touched_get_dev")
        return t.cpu().numpy()[:self.n_nodes]

    def pack_rc(self, buf_t, cap):
        """ss_nodes_pack_dev -> (return code, *n_packed); buf_t None: the size query."""
        import torch
        n = C.c_uint64(12345)
        rc = self.L.lib().ss_nodes_pack_dev(self.ns._h, buf_t.data_ptr() if buf_t is not None else None, int(cap), C.byref(n),
                                            _stream())
        torch.cuda.synchronize()
        return rc, int(n.value)

    def total(self):
        rc, n = self.pack_rc(None, 0)
        assert rc == self.L.SS_OK
        return n

    def pack(self, n):
        """The uncapped pack into a buffer 64 elements longer than n, pre-filled with the sentinel."""
        buf = _dev(np.full(n + 64, SENTINEL, np.uint32))
        rc, got = self.pack_rc(buf, n)
        assert rc == self.L.SS_OK and got == n
        return _host(buf)

    def pack_capped(self, cap):
        import torch
        buf = _dev(np.full(cap + 64, SENTINEL, np.uint32))
        tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        self._check(self.L.lib().ss_nodes_pack_capped_dev(self.ns._h, buf.data_ptr(), int(cap), tot.data_ptr(), _stream()),
                    "ss_nodes_pack_capped_dev")
        return _host(buf), int(tot.item())

    def unpack(self, packed):
        t = _dev(packed)
        self._check(self.L.lib().ss_nodes_unpack_dev(self.ns._h, t.data_ptr(), _stream()), "ss_nodes_unpack_dev")

    def unpack_capped(self, packed, cap):
        t = _dev(packed)
        self._check(self.L.lib().ss_nodes_unpack_capped_dev(self.ns._h, t.data_ptr(), int(cap), _stream()), "ss_nodes_unpack_capped_dev")

    def clear(self):
        self._check(self.L.lib().ss_nodes_clear_dev(self.ns._h, _stream()), "ss_nodes_clear_dev")

    def read_val(self):
        """The dense buffer: every flag set, then the uncapped pack.  Leaves every flag set."""
        self.flags_set(np.ones(self.n_nodes, np.int32))
        n = self.total()
        assert n == self.n_positions
        out = self.pack(n)
        assert (out[n:] == SENTINEL).all()
        return out[:n]

    def write_val(self, val):
        """Leaves every flag set."""
        self.flags_set(np.ones(self.n_nodes, np.int32))
        assert self.total() == self.n_positions            # (the unpack goes by the offsets of the last pack)
        self.unpack(np.concatenate([val, np.zeros(64, np.uint32)]))


# ---- (a) ---------------------------------------------------------------------------------------------------------------
def test_row_vector_round_trip(L, table):
    """ss_counts_load_rows_dev / ss_counts_rows_dev: what is loaded comes back on the valid rows, 0 on the others; a second
    load replaces the first in full; ss_scan_reset gives zeros.  The row count is no multiple of the block."""
    db, valid = table
    n = db.n_rows
    assert n == valid.size and n % 256 != 0 and (valid == 0).any()
    rs = np.random.RandomState(1)
    a = rs.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    a[[0, n - 1, n // 2]] = [0xFFFFFFFF, 0x80000000, 0x90000000]
    assert valid[n - 1] == 1 and int((a >= 1 << 31).sum()) > n // 4
    db.reset()
    _load(db, a)
    assert np.array_equal(db.counts_rows(), np.where(valid == 1, a, 0).astype(np.uint32))
    b = rs.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    b[::3] = 0                                             # zeros must overwrite too
    _load(db, b)
    assert np.array_equal(db.counts_rows(), np.where(valid == 1, b, 0).astype(np.uint32))
    # the device entry point gives the same vector
    import torch
    t = _dev(np.full(n, SENTINEL, np.uint32))
    db.counts_rows_dev(t.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert np.array_equal(_host(t), np.where(valid == 1, b, 0).astype(np.uint32))
    db.reset()
    L.check(L.lib().ss_device_sync(), "sync")
    assert not db.counts_rows().any()


# ---- (b) ---------------------------------------------------------------------------------------------------------------
def _node_lengths(n_nodes, rs):
    lens = rs.randint(0, 401, size=n_nodes)
    if n_nodes >= 40:
        lens[rs.choice(n_nodes, n_nodes // 10, replace=False)] = 0
        lens[[0, n_nodes - 1]] = 0
        lens[[1, n_nodes - 2]] = [137, 259]                # the first and the last node that hold anything
    return lens


def _pack_case(L, db, lens, seed):
    import torch
    rs = np.random.RandomState(seed)
    n_nodes = lens.size
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n_pos = int(offsets[-1])
    starts = rs.randint(0, db.n_rows - 401, size=n_nodes)
    rows = np.concatenate([s + np.arange(ln) for s, ln in zip(starts, lens)] + [np.zeros(0, np.int64)]).astype(np.uint32)
    ns = L.NodeSet.from_sorted(rows, offsets).bind(db)
    dev = _Dev(L, ns)

    def rand_vec(n):
        v = rs.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        v[v == SENTINEL] ^= 1
        return v

    val0 = rand_vec(n_pos)
    dev.write_val(val0)
    assert np.array_equal(dev.read_val(), val0)
    model = NumpyNodes(offsets.astype(np.int64), val0.copy())

    def only(idx):
        f = np.zeros(n_nodes, np.int32)
        f[idx] = 1
        return f

    nonempty = np.nonzero(lens > 0)[0]
    patterns = {"none": np.zeros(n_nodes, np.int32), "all": np.ones(n_nodes, np.int32),
                "half": (rs.random_sample(n_nodes) < 0.5).astype(np.int32), "first": only(0), "last": only(n_nodes - 1),
                "zero-length": (lens == 0).astype(np.int32)}
    if nonempty.size:
        patterns["first non-empty"] = only(nonempty[0])
        patterns["last non-empty"] = only(nonempty[-1])
    for name, flags in patterns.items():
        where = (n_nodes, name)
        model.flags_set(torch.from_numpy(flags), None)
        dev.flags_set(flags)
        assert np.array_equal(dev.flags_get(), flags), where
        T = model.pack(None, None)
        if name == "all":
            assert T == n_pos
        if name == "half" and n_nodes >= 40:
            assert 0 < T < n_pos, where
        if name == "zero-length":
            assert T == 0 and (n_nodes < 40 or flags.sum() > 2), where
        assert dev.total() == T, where

        def model_pack():
            t = torch.zeros(T + 1, dtype=torch.int32)
            assert model.pack(t, None) == T
            return t.numpy().view(np.uint32)[:T]

        want = model_pack()
        if T > 0:
            for cap in sorted({0, T // 2, T - 1}):
                buf = _dev(np.full(T + 64, SENTINEL, np.uint32))
                rc, n = dev.pack_rc(buf, cap)
                assert rc == L.SS_ERANGE and n == T and (_host(buf) == SENTINEL).all(), (where, cap)
        got = dev.pack(T)
        assert np.array_equal(got[:T], want) and (got[T:] == SENTINEL).all(), where
        # the capped forms: around 0, around T, all positions, around the boundary between two packed segments
        seg_ends = np.cumsum(lens[flags == 1])
        inner = seg_ends[(seg_ends > 0) & (seg_ends < T)]
        caps = {0, 1, T - 1, T, T + 1, n_pos}
        if inner.size:
            b = int(inner[inner.size // 2])
            caps |= {b - 1, b, b + 1}
        elif name in ("all", "half") and n_nodes >= 40:
            raise AssertionError("no boundary between two packed segments: %r" % (where,))
        for cap in sorted(c for c in caps if c >= 0):
            m = min(cap, T)
            want = model_pack()                            # (the buffer changes with every unpack below)
            got, total = dev.pack_capped(cap)
            want_c = torch.from_numpy(np.full(cap + 64, SENTINEL, np.uint32).view(np.int32))
            tot_c = torch.zeros(1, dtype=torch.int64)
            model.pack_capped(want_c, cap, tot_c, None)
            assert total == T == int(tot_c[0]), (where, cap, total)
            assert np.array_equal(got[:m], want[:m]), (where, cap)
            assert (got[m:] == SENTINEL).all(), (where, cap)
            assert np.array_equal(got, want_c.numpy().view(np.uint32)), (where, cap)
            # the other way: a different buffer comes in through the same offsets
            other = rand_vec(cap + 64)
            dev.unpack_capped(other, cap)
            model.unpack_capped(torch.from_numpy(other.view(np.int32)), cap, None)
            have = dev.read_val()                          # (sets every flag; the pattern is set again below)
            assert np.array_equal(have, model.val), (where, cap, int((have != model.val).sum()))
            dev.flags_set(flags)
        # the uncapped unpack
        assert dev.total() == T
        other = rand_vec(T + 64)
        dev.unpack(other)
        model.unpack(torch.from_numpy(other.view(np.int32)), None)
        assert np.array_equal(dev.read_val(), model.val), where
    assert n_pos == 0 or not np.array_equal(model.val, val0)
    dev.flags_set(patterns["half"])
    dev.clear()
    assert not dev.flags_get().any()
    assert not dev.read_val().any()
    dev.clear()
    ns.close()


@pytest.mark.parametrize("n_nodes", [1, 40, 1023, 1024, 1025, 2049, 3001])
def test_pack_and_unpack_against_the_model(L, table, n_nodes):
    """ss_nodes_touched_set/get_dev, ss_nodes_pack_dev, ss_nodes_pack_capped_dev, ss_nodes_unpack(_capped)_dev and
    ss_nodes_clear_dev against tests/nodemodel.py: 1, 2 and 3 nodes per thread of pack_offsets_kernel and node counts
    that do not fill its block; empty nodes, the first and the last among them; a buffer that ends before, at and after a
    segment's end (the `po >= cap` return and the cut inside a segment of pack_copy_kernel), with a sentinel behind it.
    A single node is run empty (as the first and the last node are) and with rows."""
    db, _ = table
    rs = np.random.RandomState(500 + n_nodes)
    if n_nodes == 1:
        _pack_case(L, db, np.array([0]), 1)
        _pack_case(L, db, np.array([333]), 2)
        return
    lens = _node_lengths(n_nodes, rs)
    assert lens[0] == 0 and lens[-1] == 0 and (lens[1:-1] == 0).any() and lens.sum() > 0
    _pack_case(L, db, lens, 3000 + n_nodes)


# ---- (c) ---------------------------------------------------------------------------------------------------------------
def _check_clean(dev):
    assert not dev.flags_get().any()
    assert not dev.read_val().any()
    dev.clear()                                            # (read_val has set the flags)


def test_dense_reduction_on_injected_counts(L, table):
    """NodeSet.harvest (harvest_kernel + node_reduce_kernel<DENSE>) on the counts of test_node_reduce_synthetic_counts,
    loaded into the table: a node with more positive counts than the kernel keeps in LDS and counts >= 65535 (both take
    the passes over the dense buffer), ties at the median, an x.5 median, the outlier cut, an all-invalid and an empty
    node; against the oracle's match_node and the row-gather path, twice (the buffer and the flags come back clean)."""
    db, valid = table
    rs = np.random.RandomState(99)
    n = db.n_rows
    counts = np.zeros(n, np.uint32)
    counts[:60_000] = rs.poisson(20, 60_000)                      # one big covered region
    counts[60_000:70_000] = rs.randint(0, 3, 10_000)              # many ties, zeros
    counts[70_000:70_100] = rs.randint(250, 70_000, 100)          # wide range: two radix bytes and >= 65535
    counts[70_050] = 65_535
    counts[70_051] = 3_000_000
    counts[80_000:80_009] = [5, 5, 5, 5, 5, 5, 5, 5, 700]         # outlier cut
    counts[90_000:90_004] = [1, 2, 3, 4]                          # even length, x.5 median
    counts[100_000:100_500] = 9                                   # rows that are not valid: never seen
    counts[110_000:110_006] = [65_535, 7, 65_535, 9, 65_534, 65_535]      # the largest count is exactly 65 535 ...
    counts[110_010:110_015] = [65_536, 65_535, 65_536, 3, 65_536]         # ... and exactly 65 536
    assert valid[80_000:80_009].all() and valid[90_000:90_004].all() and valid[110_000:110_015].all()
    assert not valid[100_000:100_500].any() and (valid[:60_000] == 0).any()
    lists = [np.arange(0, 60_000),                                # 58 k positives: beyond the LDS cap
             np.arange(0, 30_000), np.arange(60_000, 70_000), np.arange(70_000, 70_100),
             np.arange(80_000, 80_009), np.arange(90_000, 90_004), np.arange(90_000, 90_003),
             np.arange(100_000, 100_500), np.arange(150_000, 151_000), np.arange(0),
             rs.choice(n, 25_000, replace=False), np.arange(70_040, 90_004),
             np.arange(110_000, 110_006), np.arange(110_010, 110_015)]
    want = _oracle_stats(counts, valid, lists)
    db.reset()
    _load(db, counts)
    ns = L.NodeSet(lists)
    dev = _Dev(L, ns.bind(db))
    for _ in range(2):
        got = ns.harvest(db)
        assert _stats(got) == want
        assert got.tobytes() == ns.reduce(db).tobytes()
        _check_clean(dev)
    assert got[0]["n_pos"] > 32768 and got[3]["n_pos"] > 0 and got[7]["length"] == 0 and len(lists[7]) > 0
    assert got[9]["length"] == 0 and got[5]["median2"] == 5 and got[4]["n_kept"] == 8 and got[12]["median2"] == 65_534 + 65_535
    lengths = got["length"].copy()
    db.reset()
    L.check(L.lib().ss_device_sync(), "sync")
    got = ns.harvest(db)
    assert not got["n_pos"].any() and np.array_equal(got["length"], lengths) and lengths.sum() > 0
    assert got.tobytes() == ns.reduce(db).tobytes()
    ns.close()
    # few valid list positions: the `n_used & 3` tail of harvest_kernel, alone (no full group of four) and behind one group
    inv = 100_007
    small = {1: [[5]], 2: [[5], [9]], 3: [[5, inv], [7, 9], []], 7: [[1, 2, 3], [], [4, inv, 5, 6, 100_400, 70_051]]}
    counts[[1, 2, 3, 4, 5, 6, 7, 9]] = [11, 12, 13, 14, 15, 16, 17, 19]
    _load(db, counts)
    for n_used, ls in small.items():
        ls = [np.asarray(r, np.int64) for r in ls]
        assert sum(int(valid[r].sum()) for r in ls) == n_used
        ns = L.NodeSet(ls)
        want = _oracle_stats(counts, valid, ls)
        assert sum(w[1] for w in want) == n_used                  # every one of them holds a count
        dev = _Dev(L, ns.bind(db))
        for _ in range(2):
            got = ns.harvest(db)
            assert _stats(got) == want, n_used
            assert got.tobytes() == ns.reduce(db).tobytes()
            _check_clean(dev)
        ns.close()
    db.reset()


# ---- (d) ---------------------------------------------------------------------------------------------------------------
def _lockstep_nodes(n_rows, valid):
    """~60 node lists over disjoint stretches of the table (so that a hit touches one node), one of them above 40 000
    rows, empty ones, and two nodes that share rows with others."""
    rs = np.random.RandomState(31)
    sizes = rs.randint(0, 2500, size=58)
    sizes[[0, 20, 57]] = 0
    sizes[7] = 40_500
    assert sizes.sum() < n_rows
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    lists = [np.arange(s, s + z) for s, z in zip(starts, sizes)]
    lists.append(np.concatenate([lists[3][::2], lists[30][1::3]]))            # shares rows with nodes 3 and 30
    lists.append(np.sort(rs.choice(np.arange(150_000, n_rows), 1500, replace=False)))
    return lists


@pytest.mark.parametrize("world", [2, 3, 5])
def test_ranks_in_lockstep_on_one_device(L, table, world):
    """What dist.exchange_touched does between harvest and reduce, for `world` node sets on one device with torch
    standing in for the collectives: a first round whose buffer (64 elements) is too small -- every rank learns the same
    total, nothing is left behind --, then a round that fits: every rank ends with the statistics of the uint32-wrapped
    sum of all ranks' counts (a count whose sum wraps to a large value, one whose sum wraps to 0 in a node without other
    hits)."""
    import torch
    db, valid = table
    n = db.n_rows
    lists = _lockstep_nodes(n, valid)
    n_nodes = len(lists)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    all_rows = np.concatenate(lists)
    n_pos = int(offsets[-1])
    sets = [L.NodeSet(lists).bind(db) for _ in range(world)]
    devs = [_Dev(L, ns) for ns in sets]
    assert all(d.n_positions == n_pos for d in devs)
    # per-rank counts
    wrap_big = int(lists[5][len(lists[5]) // 2])           # 0x90000000 on two ranks, in a node with other hits
    wrap_zero = int(lists[40][3])                          # 0x80000000 on two ranks: node 40's only hit
    assert valid[wrap_big] and valid[wrap_zero]
    per_rank = []
    for r in range(world):
        rr = np.random.RandomState(700 + r)
        c = np.zeros(n, np.uint32)
        for j in [5, 7, 10 + r, 45 + 2 * r]:               # 5 and the large node 7 on every rank, two of the rank's own
            rows = lists[j]
            assert rows.size > 3
            idx = rr.choice(rows, size=max(1, rows.size // 3), replace=False)
            c[idx] = rr.randint(1, 50, size=idx.size)
        if r < 2:
            c[wrap_big] = 0x90000000
            c[wrap_zero] = 0x80000000
        per_rank.append(c)
    total_counts = np.zeros(n, np.uint32)
    for c in per_rank:
        total_counts = total_counts + c                    # uint32 arithmetic wraps
    assert total_counts[wrap_big] == 0x20000000 and total_counts[wrap_zero] == 0
    # the model: what each rank's harvest leaves, the union of the flags, the packed size
    models = [NumpyNodes(offsets, np.where(valid[all_rows] == 1, c[all_rows], 0).astype(np.uint32)) for c in per_rank]
    touched = np.stack([m.touched for m in models])
    union = touched.max(axis=0)
    assert ((touched.sum(axis=0) == 1) & (union == 1)).any()                  # a node only one rank has hits in
    assert union[40] == 1 and not any(total_counts[lists[40]])                # touched, yet no positive count in the sum
    for m in models:
        m.flags_set(torch.from_numpy(union), None)
    T = models[0].pack(None, None)
    assert 64 < T < n_pos and 0 < union.sum() < n_nodes
    want_val = np.zeros(n_pos, np.uint32)
    for m in models:
        want_val = want_val + m.val
    want_stats = _oracle_stats(total_counts, valid, lists)
    assert want_stats[40][1] == 0 and want_stats[40][0] > 0 and want_stats[5][4] > 0
    nbytes = n_nodes * L.NODE_STAT_DTYPE.itemsize

    def one_round(cap):
        for r in range(world):
            _load(db, per_rank[r])
            sets[r].harvest_dev(db, _stream())
            torch.cuda.synchronize()
        for r in range(world):
            assert np.array_equal(devs[r].flags_get(), touched[r]), r
        flags = np.stack([d.flags_get() for d in devs]).max(axis=0)
        assert np.array_equal(flags, union)
        for d in devs:
            d.flags_set(flags)
        packed, totals = zip(*[d.pack_capped(cap) for d in devs])
        assert list(totals) == [T] * world
        summed = _host(sum(_dev(p) for p in packed))        # the int32 sum on the device, as the all-reduce does it
        out = []
        for r, d in enumerate(devs):
            d.unpack_capped(summed, cap)
            st = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            sets[r].reduce_touched_dev(st.data_ptr(), _stream())
            torch.cuda.synchronize()
            out.append(st.cpu().numpy().view(L.NODE_STAT_DTYPE))
        return out

    db.reset()
    one_round(64)                                          # T > cap: the statistics are of no use
    for d in devs:
        _check_clean(d)
    stats = one_round(2 * T)
    for d in devs:
        _check_clean(d)
    for r in range(world):
        assert stats[r].tobytes() == stats[0].tobytes(), r
    assert _stats(stats[0]) == want_stats
    _load(db, total_counts)
    assert stats[0].tobytes() == sets[0].reduce(db).tobytes()
    # and the dense buffer itself, after harvest + exchange, is the model's sum on the union's nodes
    for r in range(world):
        _load(db, per_rank[r])
        sets[r].harvest_dev(db, _stream())
    torch.cuda.synchronize()
    for d in devs:
        d.flags_set(union)
    packed = [d.pack_capped(2 * T)[0] for d in devs]
    summed = _host(sum(_dev(p) for p in packed))
    mask = np.repeat(union, np.diff(offsets)).astype(bool)
    for r, d in enumerate(devs):
        d.unpack_capped(summed, 2 * T)
        have = d.read_val()
        assert np.array_equal(have[mask], want_val[mask]) and np.array_equal(have[~mask], models[r].val[~mask]), r
        assert not have[~mask].any()
        d.clear()
    for ns in sets:
        ns.close()
    db.reset()


# ---- (e) ---------------------------------------------------------------------------------------------------------------
CHILD = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, %(repo)r)
import torch
import torch.distributed as dist
torch.cuda.set_device(0)
dist.init_process_group("gloo", init_method="file://" + %(store)r, rank=0, world_size=1)
from strainscan_amd import _lib as L, dist as sdist
from tests.test_nodes_exchange_gpu import _make_keys, _load, _stats, _oracle_stats
keys, dup = _make_keys(50_000, (20_000, 20_100), 50, 77)
db = L.KmerDB(keys, np.ones(keys.size, np.uint8), 31, True)
valid = db.row_valid.copy()
assert (valid == 0).sum() == dup.size
rs = np.random.RandomState(5)
sizes = rs.randint(0, 1200, size=30)
sizes[[0, 29]] = 0
starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
lists = [np.arange(s, s + z) for s, z in zip(starts, sizes)]
n_pos = int(sizes.sum())

def counts_in(nodes, seed):
    rr = np.random.RandomState(seed)
    c = np.zeros(keys.size, np.uint32)
    for j in nodes:
        idx = rr.choice(lists[j], size=lists[j].size // 2, replace=False)
        c[idx] = rr.randint(1, 90, size=idx.size)
    return c

def total_of(c):
    return int(sum(len(r) for r in lists if (c[r] * valid[r]).any()))

res = {}
c1 = counts_in([3, 4, 11], 1)
T = total_of(c1)
assert 64 < T and 2 * T < n_pos, (T, n_pos)
_load(db, c1)
ns = L.NodeSet(lists)
sdist.PACK_MIN = 64
rounds = []

def between(n):
    rounds.append(1)
    return sdist.exchange_touched(n)

got = ns.harvest(db, between=between)
res["first_equal"] = got.tobytes() == ns.reduce(db).tobytes() and _stats(got) == _oracle_stats(c1, valid, lists)
res["first_rounds"] = len(rounds)
res["n_pos_sum"] = int(got["n_pos"].sum())
res["pack_cap"] = int(ns.__dict__["_pack_cap"])
res["pack_cap_want"] = min(max(64, 2 * T), n_pos)
del rounds[:]
got = ns.harvest(db, between=between)
res["second_equal"] = got.tobytes() == ns.reduce(db).tobytes()
res["second_rounds"] = len(rounds)

class Boom(Exception):
    pass

def bad(n):
    sdist.exchange_touched(n)
    raise Boom("after the harvest")

def raises():
    try:
        ns.harvest(db, between=bad)
    except Boom:
        return True
    return False

res["raised"] = raises()
got = ns.harvest(db)
res["after_raise_equal"] = got.tobytes() == ns.reduce(db).tobytes() and _stats(got) == _oracle_stats(c1, valid, lists)
# the same with other nodes hit afterwards: counts left in the buffer would show in nodes 3, 4 and 11
res["raised_again"] = raises()
c2 = counts_in([7, 20], 2)
db.reset()
_load(db, c2)
got = ns.harvest(db)
res["after_raise_other_equal"] = got.tobytes() == ns.reduce(db).tobytes() and _stats(got) == _oracle_stats(c2, valid, lists)
res["other_n_pos"] = [int(got[j]["n_pos"]) for j in (3, 4, 11, 7, 20)]
json.dump(res, open(%(out)r, "w"))
dist.destroy_process_group()
'''


def test_harvest_retries_through_exchange_touched(tmp_path):
    """NodeSet.harvest with dist.exchange_touched between harvest and reduce, in a process of its own (a gloo group of
    one rank): the first buffer (PACK_MIN = 64) is too small, so the harvest runs a second round with the buffer the
    first one sized, which the node set keeps; the next call needs one round; an exception out of `between` leaves no
    counts behind in the dense buffer."""
    out = tmp_path / "res.json"
    code = CHILD % dict(repo=REPO, store=str(tmp_path / "store"), out=str(out))
    p = subprocess.run([sys.executable, "-c", code], stderr=subprocess.PIPE, timeout=240)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    res = json.loads(out.read_text())
    assert res["first_equal"] and res["first_rounds"] == 2 and res["n_pos_sum"] > 64
    assert res["pack_cap"] == res["pack_cap_want"]
    assert res["second_equal"] and res["second_rounds"] == 1
    assert res["raised"] and res["after_raise_equal"]
    assert res["raised_again"] and res["after_raise_other_equal"]
    assert res["other_n_pos"][:3] == [0, 0, 0] and min(res["other_n_pos"][3:]) > 0
