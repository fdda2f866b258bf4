"""The inputs of the strain-set device tests (tests/test_strain_sets_gpu.py), made with numpy alone so that the conditions that keep
those tests from passing vacuously can be checked on the model without a device (tests/test_strain_sets_host.py does).

The genome, the read blocks and the (k, step, expect_hits) of the tables are those of tests/class_cases.py; a row gets a MASK of
called strains in the place of a node.  The genome is cut into zones of ten stretches (2350 bases), four kinds in turn:
  kind 0, 1  a normal zone with strains a, b, c, d picked by its number: stretches 0-4 belong to {a, b, c} (a read inside them is a
             tie of three), 5-6 to {a, b} (a tie of two), 7 to {a}, 8 to {b, d}, 9 to {d}: overlapping stretches given to
             overlapping subsets, so a read that reaches from one into the next is a unique assignment.  The second normal zone
             gives its first five stretches to ALL strains: the mask with every bit, bit 15 among them at sixteen strains.
  kind 2     five stretches WITHOUT rows (reads inside have no hit), then five whose rows have mask 0 (hits that vote for nobody)
  kind 3     five stretches of mask 0, then five without rows but for an ISLAND of five k-mer starts of one strain in their middle:
             a read over the island has a score of at most 5 -- assigned at M = 1, unassigned with 0 < score < 8 at M = 8
Three more rows close every table: a k-mer listed again under the same mask (its slot keeps the mask), one listed again under
another mask (its slot gets 0), and one with an N (a row without a slot).
"""
import numpy as np

from tests import class_cases as cc, rs_model

ZONE = 10 * cc.STRETCH
ISLAND = 7 * cc.STRETCH + 100      # where a kind-3 zone's island begins, and its k-mer starts
ISLAND_LEN = 5

# name -> (k, step, expects hits, called strains, whole): k, step and expect as class_cases.TABLES has them;
# whole: every start has a row and strain 1 has them all (the table of the one long record)
TABLES = {
    "k31_dense_n16": (31, 1, True, 16, False),
    "k31_sampled_n2": (31, 7, False, 2, False),
    "k25_n15": (25, 2, False, 15, False),
    "k31_n1": (31, 3, True, 1, False),
    "k31_whole_n2": (31, 1, False, 2, True),
}
assert {(k, s, e) for k, s, e, _, _ in TABLES.values()} >= {v for v in cc.TABLES.values()}
MS = (1, 2, 8)


def _bits(n, *strains):
    m = 0
    for s in strains:
        m |= 1 << (s % n)
    return m


def mask_of_start(i, n):
    """the mask of the k-mer that starts at genome position i; None: no row"""
    z, off = divmod(i, ZONE)
    kind, sb = z % 4, off // cc.STRETCH
    if kind == 2:
        return None if sb < 5 else 0
    if kind == 3:
        if sb < 5:
            return 0
        return _bits(n, z) if ISLAND <= off < ISLAND + ISLAND_LEN else None
    zi = (z // 4) * 2 + kind
    a = zi * 5
    b, c, d = a + 1, a + 2, a + n // 2
    if sb < 5:
        return (1 << n) - 1 if zi == 1 else _bits(n, a, b, c)
    return (_bits(n, a, b), _bits(n, a, b), _bits(n, a), _bits(n, b, d), _bits(n, d))[sb - 5]


def whole_mask_of_start(i):
    """strain 1 everywhere, strain 2 in every other zone"""
    return 1 | (2 if (i // ZONE) % 2 == 0 else 0)


def table(name, g):
    """-> (k, n, kmers, row_sets u16 per row, keys u64 and sets u16 of the rows that have a slot): the rows of table `name`"""
    k, step, _, n, whole = TABLES[name]
    kmers, sets = [], []
    for i in range(0, len(g) - k + 1, step):
        m = whole_mask_of_start(i) if whole else mask_of_start(i, n)
        if m is not None:
            kmers.append(g[i:i + k])
            sets.append(m)
    assert len(set(kmers)) == len(kmers)
    same = next(j for j, m in enumerate(sets) if m)
    other = next(j for j, m in enumerate(sets) if m and j > same + 40)
    kmers += [kmers[same], kmers[other]]
    sets += [sets[same], sets[other] ^ 1]
    keys = rs_model.encode_kmers(kmers, k)
    valid_sets = np.array(sets, np.uint16)
    kmers.append(kmers[5][:k // 2] + b"N" + kmers[5][k // 2 + 1:])      # no k-mer: the row has no slot, its mask counts nowhere
    sets.append(1)
    return k, n, kmers, np.array(sets, np.uint16), keys, valid_sets


def one_bit_rows(row_sets):
    """-> (masks with the lowest strain of every row only, the same as labels 0..16)"""
    rs = np.asarray(row_sets, np.int64)
    low = rs & -rs
    lab = np.where(low > 0, np.log2(np.maximum(low, 1)).astype(np.int64) + 1, 0)
    return low.astype(np.uint16), lab.astype(np.uint8)


def long_record_block(g):
    """one record of about 70 000 bases: the genome but its last base"""
    return g[:len(g) - 1] + b"\n"


def two_slab_reads(g):
    """the reads of the two .fastq.gz files of the device test: 1250 reads of 1000 bases each"""
    rs = np.random.RandomState(13)
    return [[g[s:s + 1000] for s in rs.randint(0, len(g) - 1000, size=1250)] for _ in range(2)]


def host_texts(g):
    """name -> the flat text of every read set of the device test but the empty one, as the model takes it"""
    one = cc.one_length_block(g)
    lines = one.split(b"\n")[:-1]
    out = {"packed": one, "file_order": one, "binned_ascii": cc.one_length_block(g, lower=True)}
    for tail in (0, 1, 1023):
        out["ragged_%d" % tail] = cc.ragged_block(g, tail)
    out["two_slabs"] = b"".join(r + b"\n" for part in two_slab_reads(g) for r in part)
    out["half_a"] = b"".join(r + b"\n" for r in lines[:1500])
    out["half_b"] = b"".join(r + b"\n" for r in lines[1500:])
    out["long"] = long_record_block(g)
    return out
