"""The inputs of the read-class device tests (tests/test_classify_gpu.py), made with numpy alone so that the conditions that keep
those tests from passing vacuously can be checked on the model without a device (tests/test_classify_host.py does).

The source is 70 kb of random bases cut into stretches of 235; stretch j belongs to node j + 1.  300 nodes:
  1..40     a chain written upwards: parent[v] = v + 1 (so parent[v] > v), node 40 its root and node 1 at depth 40
  41..60    children of 40
  61..280   the bushy part: eleven children under each of 41..60, neighbouring stretches being siblings
  281       a second root, 282..300 its children
Stretch 120's rows are nobody's (node 0), so node 121 has no rows; nodes 299 and 300 lie beyond the source and have none
either.  One k-mer of stretch 10 is listed a second time under node 200: its slot counts for nobody.
"""
import numpy as np

from tests import rs_model

STRETCH = 235
N_NODES = 300
SRC_LEN = 70000


def rand_bases(rs, n):
    return np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, size=n)].tobytes()


def source():
    return rand_bases(np.random.RandomState(2027), SRC_LEN)


def parents():
    par = np.zeros(N_NODES + 1, np.uint32)
    for v in range(1, 40):
        par[v] = v + 1
    par[41:61] = 40
    for v in range(61, 281):
        par[v] = 41 + (v - 61) // 11
    par[282:301] = 281
    return par


def node_of_start(i):
    j = i // STRETCH
    return 0 if j == 120 else j + 1


TABLES = {"k31_dense": (31, 1, True), "k31_sampled": (31, 7, False), "k25": (25, 2, False)}      # k, step, expects hits


def table(name, g):
    """-> (k, kmers, keys u64, row_node u32): the rows of table `name`; the last row repeats a k-mer under another node"""
    k, step, _ = TABLES[name]
    starts = list(range(0, len(g) - k + 1, step))
    kmers = [g[i:i + k] for i in starts]
    assert len(set(kmers)) == len(kmers)
    row_node = [node_of_start(i) for i in starts]
    twice = next(j for j, i in enumerate(starts) if i >= 10 * STRETCH + 70)
    assert row_node[twice] == 11
    kmers.append(kmers[twice])
    row_node.append(200)
    return k, kmers, rs_model.encode_kmers(kmers, k), np.array(row_node, np.uint32)


def kfa(kmers):
    return b"".join(b">1\n" + km + b"\n" for km in kmers)


def spliced_reads(g):
    """x bases of one stretch, then x of another, x in 31..60, filled up to 150 with N: siblings (61..280), leaves whose lowest
    common ancestor is the root 40, and leaves of the two trees"""
    rs = np.random.RandomState(5)
    out = []
    for i in range(160):
        x = 31 + i % 30
        if i % 4 < 2:
            p = 41 + rs.randint(0, 20)
            a, b = (61 + (p - 41) * 11 + c for c in rs.choice(11, 2, replace=False))
        elif i % 4 == 2:
            a, b = 61 + rs.randint(0, 110), 171 + rs.randint(0, 110)
            if (a - 61) // 11 == (b - 61) // 11:
                b += 11
        else:
            a, b = 61 + rs.randint(0, 220), 282 + rs.randint(0, 16)
        if a == 121 or b == 121:
            a, b = 61, 62
        sa, sb = ((v - 1) * STRETCH + rs.randint(0, STRETCH - 60) for v in (a, b))
        out.append(g[sa:sa + x] + g[sb:sb + x] + b"N" * (150 - 2 * x))
    return out


def one_length_block(g, lower=False):
    """3000 reads of 150 bases with N's, the spliced reads among them; lower: one lower-case base (a binned slab then stays ASCII)"""
    rs = np.random.RandomState(7)
    src = np.frombuffer(g, np.uint8)
    starts = rs.randint(0, src.size - 150, size=2840)
    arr = src[starts[:, None] + np.arange(150)[None, :]].copy()
    arr[::53, :][np.arange(len(arr[::53])), rs.randint(0, 150, size=len(arr[::53]))] = ord("N")
    arr[5::211, 0] = ord("N")
    arr[9::223, 149] = ord("N")
    recs = [a.tobytes() for a in arr]
    for i, r in enumerate(spliced_reads(g)):
        recs.insert(17 * i, r)
    assert len(recs) == 3000 and all(len(r) == 150 for r in recs)
    if lower:
        recs[1234] = recs[1234][:75] + recs[1234][75:76].lower() + recs[1234][76:]
    return b"".join(r + b"\n" for r in recs)


def long_record(g):
    """20 kb that crosses the whole source: 67 bases of every stretch"""
    n = (len(g) - 67) // STRETCH + 1
    r = b"".join(g[j * STRETCH + 90:j * STRETCH + 157] for j in range(n))
    assert 19000 <= len(r) <= 21000
    return r


def ragged_block(g, tail_mod):
    """Lengths 1, 30, 31, 32 and 150, lower case, N inside and at the ends, an empty record, a 2500-base record that spans three
    tiles, the 20 kb record; the block's length is tail_mod modulo 1024."""
    rs = np.random.RandomState(11)
    recs = []
    for i in range(1600):
        ln = (1, 30, 31, 32, 150, 150, 150, 150)[i % 8]
        s = rs.randint(0, len(g) - ln)
        r = bytearray(g[s:s + ln])
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
    recs.insert(700, g[1000:3500])
    recs.insert(900, long_record(g))
    # 45 bases of each of c stretches, c around the number of nodes a record may hold on the device's per-thread path; and a
    # record longer than that path takes, with few nodes
    for c in (7, 8, 9, 10, 16):
        recs.insert(1100 + c, b"".join(g[j * STRETCH + 20:j * STRETCH + 65] for j in rs.choice(119, c, replace=False)))
    recs.insert(1300, g[5000:5600] * 8)
    block = b"\n".join(recs[:1000]) + b"\n\n" + b"\n".join(recs[1000:]) + b"\n"      # (two '\n' in a row: an empty record)
    last = (tail_mod - len(block) - 1) % 1024
    if last < 40:
        last += 1024
    block += g[300:300 + last] + b"\n"
    assert len(block) % 1024 == tail_mod
    return block


def relabel15(row_node):
    """the nodes folded onto 15 labels (0 stays 0)"""
    rn = np.asarray(row_node, np.int64)
    return np.where(rn > 0, 1 + rn % 15, 0).astype(np.uint8)
