"""The route table of the page-index scans, walked once: which kernel instantiation a scan takes follows from the table's k (31,
or k at run time, or the per-position kernel), its filter kind (a Bloom filter, the ss_db_expect_hits flag, neither), the layout
of the block (ASCII aligned / unaligned, a binned ASCII or packed slab, a set in file order) and whether one table or several
share the pass.  Every route counts exactly what the oracle counts; a fused ss_scan_reads_multi equals the single scans and
makes the launches its grouping promises (one per group of two to four tables of one k and one kind per slab).

The set is small (about 3 000 tiles): below the probe of unflagged tables under binned reads, which test_scan_gpu.py
(test_combining_kernel_chosen_from_the_data) and test_packed_reads_gpu.py (test_packed_set_past_the_probe) hold.

Absent from the table, because the library has no such route: the Bloom kind at k other than 31 in a several-tables pass (there is
no such instantiation: those tables go one by one through the single-table scan, asserted here by their launch counts), and -- for
every kind -- k = 19, below the smallest k that shares a pass.  A fused call reads a resident set, whose slabs are 16-byte
aligned: the unaligned block is a single-table route only."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G, STEP, N_READS, READ_LEN = 60000, 7, 20000, 150
KINDS = ("bloom", "expect_hits", "plain")
SHARE_K_MIN = 20                 # several tables share a pass at k >= 20 (the Bloom kind: at k = 31 only)


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def sample(L):
    """The genome, the reads as a flat block and as FASTQ, and the five inputs of a route (made once, never changed)."""
    import torch
    rs = np.random.RandomState(1207)
    lut = np.frombuffer(b"ACGT", np.uint8)
    g = lut[rs.randint(0, 4, size=G)]
    starts = rs.randint(0, G - READ_LEN, size=N_READS)
    arr = g[starts[:, None] + np.arange(READ_LEN)[None, :]].copy()
    arr[5::97, rs.randint(0, READ_LEN)] = ord("N")               # a few reads with an N
    arr[11::301, 3] = ord("N")                                   # ... some in the first k-mer (the bin of their own)
    recs = [a.tobytes() for a in arr]
    flat = b"\n".join(recs) + b"\n"
    fq = b"".join(b"@r\n" + r + b"\n+\n" + b"I" * READ_LEN + b"\n" for r in recs)
    d = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    buf = torch.zeros(d.numel() + 32, dtype=torch.uint8, device="cuda")
    a0 = (-buf.data_ptr()) % 16                                  # a 16-byte aligned address inside buf
    buf[a0 + 3:a0 + 3 + d.numel()] = d
    assert (d.data_ptr() % 16, (buf.data_ptr() + a0 + 3) % 16) == (0, 3)
    sets = {}
    for name in ("binned_ascii", "binned_packed", "file_order"):
        L.check(L.lib().ss_test_hook(5, 1 if name == "binned_ascii" else 0), "ss_test_hook")
        try:
            sets[name] = L.ReadSet.from_flat_dev(d.data_ptr(), d.numel(), order=name != "file_order")
        finally:
            L.lib().ss_test_hook(5, 0)
        assert (sets[name].packed_slabs() > 0) == (name == "binned_packed"), name
    L.check(L.lib().ss_device_sync(), "sync")
    yield dict(g=g.tobytes(), fq=fq, n=d.numel(), aligned=d, unaligned=(buf, buf.data_ptr() + a0 + 3), sets=sets)
    for s in sets.values():
        s.close()


def _kfa(g, k, j):
    """Table j of a k: the k-mers of the genome taken every 7 bases from base j on (_kdb of test_binning_gather_gpu.py)."""
    return b"".join(b">1\n" + g[i:i + k] + b"\n" for i in range(j, len(g) - k, STEP))


_oracle = {}


def _want(sample, k, j):
    """The oracle's row counts of table j at this k (computed once, shared by the three kinds)."""
    from oracle import oracle as orc
    if (k, j) not in _oracle:
        _oracle[(k, j)] = orc.jellyfish_count(_kfa(sample["g"], k, j), [sample["fq"]], k=k, upper=True)[0]
        assert _oracle[(k, j)].sum() > 100_000
    return _oracle[(k, j)]


def _tables(L, sample, k, kind, n=5):
    """n tables of one k and one kind: a forced Bloom filter, the flag, or neither (SS_BLOOM_BITS is read when a table is built)."""
    old = os.environ.get("SS_BLOOM_BITS")
    os.environ["SS_BLOOM_BITS"] = "0" if kind == "plain" else "16"
    try:
        dbs = [L.KmerDB.from_text(_kfa(sample["g"], k, j), k, True) for j in range(n)]
    finally:
        if old is None:
            del os.environ["SS_BLOOM_BITS"]
        else:
            os.environ["SS_BLOOM_BITS"] = old
    for db in dbs:
        info = db.info()
        assert info["layout"] == 1
        assert (info["filter_bits"] > 0) == (kind != "plain"), (kind, info)
        if kind == "expect_hits":
            db.expect_hits()
    return dbs


def _launches(L, db):
    return int(L.lib().ss_scan_kernel_launches(db.handle))


def _single(L, sample, db, inp):
    """One single-table scan of the input into the (reset) table -> (row counts, launches it made)."""
    db.reset()
    l0 = _launches(L, db)
    if inp == "aligned":
        db.scan_flat_dev(sample["aligned"].data_ptr(), sample["n"], None)
    elif inp == "unaligned":
        db.scan_flat_dev(sample["unaligned"][1], sample["n"], None)
    else:
        sample["sets"][inp].scan_into(db)
    L.check(L.lib().ss_device_sync(), "sync")
    return db.counts_rows(), _launches(L, db) - l0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [31, 25, 19])
def test_every_route_counts_what_the_oracle_counts(L, sample, k, kind):
    """k x filter kind, and inside: the five inputs, each under ss_test_hook(4) = 0 (the product's choice: at k = 19 the
    per-position kernel for a flagged table, the run-queue kernel otherwise), 2 (the per-position kernel) and 3 (the run-queue
    kernel: at k = 19 with the flag the one the product does not pick, the combining variant under binned reads); then
    ss_scan_reads_multi of two and of five tables (a group of four and a single) over the three resident sets."""
    dbs = _tables(L, sample, k, kind)
    wants = [_want(sample, k, j) for j in range(len(dbs))]
    inputs = ("aligned", "unaligned", "binned_ascii", "binned_packed", "file_order")
    try:
        for hook in (0, 2, 3):
            L.check(L.lib().ss_test_hook(4, hook), "ss_test_hook")
            for inp in inputs:
                got, launched = _single(L, sample, dbs[0], inp)
                assert np.array_equal(got, wants[0]), (k, kind, hook, inp)
                assert launched == 1, (k, kind, hook, inp)                       # one slab, one launch
        L.check(L.lib().ss_test_hook(4, 0), "ss_test_hook")
        shares = k >= SHARE_K_MIN and (k == 31 or kind != "bloom")
        for inp in inputs[2:]:
            for n_tab in (2, 5):
                tabs = dbs[:n_tab]
                for db, want in zip(tabs, wants):
                    got, _ = _single(L, sample, db, inp)                         # every table's own single scan ...
                    assert np.array_equal(got, want), (k, kind, inp, "single", n_tab)
                    db.reset()
                m0, l0 = L.scan_multi_launches(), [_launches(L, db) for db in tabs]
                sample["sets"][inp].scan_into_many(tabs)
                L.check(L.lib().ss_device_sync(), "sync")
                m1, l1 = L.scan_multi_launches(), [_launches(L, db) for db in tabs]
                for db, want in zip(tabs, wants):                                # ... is what the fused call leaves in it
                    assert np.array_equal(db.counts_rows(), want), (k, kind, inp, "fused", n_tab)
                # one fused launch per group of two to four tables (five = four + a single: one), a launch of its own for
                # a table alone in its group or of a kind / k that shares no pass; each table is launched once either way
                delta = {kd: m1[kd] - m0[kd] for kd in KINDS}
                assert delta == {kd: (1 if shares and kd == kind else 0) for kd in KINDS}, (k, kind, inp, n_tab, delta)
                assert [b - a for a, b in zip(l0, l1)] == [1] * n_tab, (k, kind, inp, n_tab)
    finally:
        L.check(L.lib().ss_test_hook(4, 0), "ss_test_hook")
        for db in dbs:
            db.close()
