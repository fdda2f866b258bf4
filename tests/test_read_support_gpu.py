"""ss_reads_support (ss_support.hip, scan_minik_kernel's SupportSink): hits per record, reduced to a histogram and a total, held
bit for bit to the model of tests/rs_model.py for every (table, read set) below; the total equals what ss_scan_reads counts over
the same pair, and the table's counters are the same before and after."""
import gzip
import os

import numpy as np
import pytest

from tests import rs_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


def _rand(rs, n):
    return np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, size=n)].tobytes()


def _distinct(kmers):
    return list(dict.fromkeys(kmers))


def _kfa(kmers):
    return b"".join(b">1\n" + km + b"\n" for km in kmers)


def _all_kmers(g, k, step=1):
    return [g[i:i + k] for i in range(0, len(g) - k + 1, step)]


@pytest.fixture(scope="module")
def material():
    """The genome g, the repeat genome, the random k-mers, and `src`: what the reads are cut from (all three, so that every table
    is hit)."""
    rs = np.random.RandomState(2024)
    g = _rand(rs, 70000)
    stretch = _rand(rs, 60)
    rep = b"".join(_rand(rs, 1128) + stretch for _ in range(5))
    rep += _rand(rs, 6000 - len(rep))
    rnd = _distinct([_rand(rs, 31) for _ in range(100000)])
    src = g + rep + b"".join(rnd[::333])
    return dict(g=g, rep=rep, rnd=rnd, src=src)


TABLES = ["k31_sampled", "k31_dense", "k31_repeat", "k31_random", "k25", "k17"]


@pytest.fixture(scope="module")
def tables(L, material):
    """name -> (KmerDB, k, model keys)"""
    g = material["g"]
    spec = {
        "k31_sampled": (31, _all_kmers(g, 31, 7), False),                 # inline slots, a Bloom filter
        "k31_dense": (31, _all_kmers(g[:20000], 31), True),               # solid buckets; expects hits
        "k31_repeat": (31, _all_kmers(material["rep"], 31), False),       # several k-mers per minimizer offset
        "k31_random": (31, material["rnd"], False),                       # more minimizers than the smallest index has slots
        "k25": (25, _all_kmers(g, 25, 3), False),
        "k17": (17, _all_kmers(g[:30000], 17), False),                    # three m-mers per k-mer
    }
    out = {}
    for name, (k, kmers, expect) in spec.items():
        kmers = _distinct(kmers)
        db = L.KmerDB.from_text(_kfa(kmers), k, True)
        if expect:
            db.expect_hits(True)
        out[name] = (db, k, rs_model.encode_kmers(kmers, k))
    yield out
    for db, _, _ in out.values():
        db.close()


def _one_length_block(material):
    rs = np.random.RandomState(7)
    src = np.frombuffer(material["src"], np.uint8)
    starts = rs.randint(0, src.size - 150, size=3000)
    arr = src[starts[:, None] + np.arange(150)[None, :]].copy()
    arr[::53, :][np.arange(len(arr[::53])), rs.randint(0, 150, size=len(arr[::53]))] = ord("N")
    arr[5::211, 0] = ord("N")
    arr[9::223, 149] = ord("N")
    return b"".join(a.tobytes() + b"\n" for a in arr)


def _ragged_block(material, tail_mod):
    """Lengths 1, 30, 31, 32 and 150, two long records, lower case, N inside and at the ends, an empty record; the block's length
    is tail_mod modulo 1024 (its last record is sized for that)."""
    rs = np.random.RandomState(11)
    g, src = material["g"], material["src"]
    recs = []
    for i in range(2400):
        ln = (1, 30, 31, 32, 150, 150, 150, 150)[i % 8]
        s = rs.randint(0, len(src) - ln)
        r = bytearray(src[s:s + ln])
        if i % 17 == 0 and ln > 40:
            a = rs.randint(0, ln - 35)
            r[a:a + 35] = bytes(r[a:a + 35]).lower()
        if i % 19 == 0:
            r[rs.randint(0, ln)] = ord("N")
        if i % 41 == 0:
            r[0] = ord("N")
        if i % 43 == 0:
            r[-1] = ord("n")
        recs.append(bytes(r))
    recs.insert(700, g[1000:3500])             # spans three tiles
    recs.insert(1500, g[5000:10000].lower()[:2500] + g[7500:10000])
    block = b"\n".join(recs[:1000]) + b"\n\n" + b"\n".join(recs[1000:]) + b"\n"      # (two '\n' in a row: an empty record)
    last = (tail_mod - len(block) - 1) % 1024
    if last < 40:
        last += 1024
    block += src[300:300 + last] + b"\n"
    assert len(block) % 1024 == tail_mod
    return block


def _fastq_gz(path, block, seed):
    rs = np.random.RandomState(seed)
    qa = np.frombuffer(b"0123456789BCDEFGHIJ", np.uint8)
    out = []
    for i, r in enumerate(block.split(b"\n")):
        if r:
            out.append(b"@r%d\n%s\n+\n%s\n" % (i, r, qa[rs.randint(0, qa.size, size=len(r))].tobytes()))
    with open(path, "wb") as f:
        f.write(gzip.compress(b"".join(out), 1))
    assert os.path.getsize(path) >= 1 << 20
    return path


SETS = ["packed", "ascii_binned", "file_order", "ragged_binned", "ragged_1024", "ragged_1025", "gz_pair"]


@pytest.fixture(scope="module")
def read_sets(L, material, tmp_path_factory):
    """name -> (ReadSet, its bytes read back)"""
    import torch
    keep, out = [], {}

    def flat(block, order, ascii_slabs=False):
        d = torch.frombuffer(bytearray(block), dtype=torch.uint8).cuda()
        keep.append(d)
        L.check(L.lib().ss_test_hook(5, 1 if ascii_slabs else 0), "ss_test_hook")
        try:
            rset = L.ReadSet.from_flat_dev(d.data_ptr(), d.numel(), order=order)
        finally:
            L.lib().ss_test_hook(5, 0)
        L.check(L.lib().ss_device_sync(), "sync")
        return rset

    one = _one_length_block(material)
    out["packed"] = flat(one, True)
    assert out["packed"].packed_slabs() >= 1
    out["ascii_binned"] = flat(one, True, ascii_slabs=True)
    assert out["ascii_binned"].packed_slabs() == 0
    out["file_order"] = flat(one, False)
    out["ragged_binned"] = flat(_ragged_block(material, 0), True)
    out["ragged_1024"] = flat(_ragged_block(material, 0), False)
    out["ragged_1025"] = flat(_ragged_block(material, 1), False)
    # two .fastq.gz files of 1 MB and more: the device path gives each a slab of its own -- record indices run on across slabs
    rs = np.random.RandomState(13)
    src = np.frombuffer(material["src"], np.uint8)
    root = str(tmp_path_factory.mktemp("rs_gz"))
    paths = []
    for m in range(2):
        starts = rs.randint(0, src.size - 150, size=11000)
        arr = src[starts[:, None] + np.arange(150)[None, :]]
        paths.append(_fastq_gz(os.path.join(root, "r%d.fastq.gz" % (m + 1)), b"".join(a.tobytes() + b"\n" for a in arr), 100 + m))
    out["gz_pair"] = L.ReadSet(paths)
    sets = {name: (r, r.read_back()) for name, r in out.items()}
    yield sets
    for r in out.values():
        r.close()


_MODEL = {}


def _model(tables, read_sets, tname, sname):
    """per-record hits of the model, computed once per (table, set)"""
    if (tname, sname) not in _MODEL:
        _, k, keys = tables[tname]
        _MODEL[tname, sname] = rs_model.hits_per_record(read_sets[sname][1], keys, k)
    return _MODEL[tname, sname]


@pytest.mark.parametrize("sname", SETS)
@pytest.mark.parametrize("tname", TABLES)
def test_support_equals_model(L, tables, read_sets, tname, sname):
    db, k, _ = tables[tname]
    rset, text = read_sets[sname]
    per = _model(tables, read_sets, tname, sname)
    n_rec = sum(1 for p in text.split(b"\n") if p)
    assert per.size == n_rec
    # the scan of the same pair: its counters are what support() must leave alone, their sum what its total must equal
    db.reset()
    rset.scan_into(db)
    L.check(L.lib().ss_device_sync(), "sync")
    before = db.counts_rows().copy()
    hist, hits = rset.support(db)
    after = db.counts_rows()
    want = rs_model.histogram(per, 65)
    print(tname, sname, "records", n_rec, "hits", hits, "model", int(per.sum()), "scan", int(before.sum()), "ge1", n_rec - int(hist[0]))
    assert hist.dtype == np.uint64 and hist.shape == (65,)
    assert hits == int(per.sum())
    assert (hist == want).all(), (hist.tolist(), want.tolist())
    assert hits == int(before.astype(np.uint64).sum())
    assert (before == after).all()
    for nb in (2, 300):
        h2, hits2 = rset.support(db, n_bins=nb)
        assert hits2 == hits
        assert int(h2.sum()) == n_rec
        assert (h2 == rs_model.histogram(per, nb)).all()


def test_long_records_reach_the_last_bin(L, tables, read_sets):
    """the 2 500- and 5 000-base records against the dense table: more than 64 hits each, in the open-ended bin"""
    per = _model(tables, read_sets, "k31_dense", "ragged_binned")
    assert (per >= 2000).sum() >= 1 and per.max() >= 2400
    hist, _ = read_sets["ragged_binned"][0].support(tables["k31_dense"][0])
    assert int(hist[64]) == int((per >= 64).sum()) >= 2


def test_errors(L, material, read_sets):
    rset = read_sets["packed"][0]
    k15 = L.KmerDB.from_text(_kfa(_distinct(_all_kmers(material["g"][:5000], 15, 5))), 15, True)
    try:
        with pytest.raises(L.SSError) as e:
            rset.support(k15)
        assert e.value.code == L.SS_ERANGE
    finally:
        k15.close()


def test_n_bins_below_two_is_refused(L, tables, read_sets):
    before = L.support_calls()
    with pytest.raises(L.SSError) as e:
        read_sets["packed"][0].support(tables["k25"][0], n_bins=1)
    assert e.value.code == L.SS_EINVAL
    assert L.support_calls() == before
    read_sets["packed"][0].support(tables["k25"][0])
    assert L.support_calls() == before + 1
