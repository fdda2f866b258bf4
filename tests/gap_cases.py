"""The inputs of the gap tests (tests/test_gaps_host.py, tests/test_gaps_gpu.py), made with numpy alone so that what keeps the
device tests from passing vacuously can be checked on the model without a device.

The genome is 4 kb of random bases at a fixed seed.  Table "k31": every 31-mer of both strands.  Table "k21": the 21-mers of the
forward strand, with a stretch of 300 starts left out after every 700 (runs of misses of every length class between hits) and
three rows more: a k-mer listed again, a k-mer with an N (a row without a slot), and -- see called_rows -- rows that disagree.
"""
import numpy as np

from tests import rs_model

K = 31
GENOME_LEN = 4000
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rand_bases(rs, n):
    return np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, size=n)].tobytes()


def genome():
    return rand_bases(np.random.RandomState(4242), GENOME_LEN)


def other_genome():
    return rand_bases(np.random.RandomState(999), GENOME_LEN)


def revcomp(s):
    return s.translate(_COMP)[::-1]


def kfa(kmers):
    return b"".join(b">1\n" + km + b"\n" for km in kmers)


def table(name, g):
    """-> (k, kmers as rows of the table, keys u64 of the rows that have a slot, start of every such row's k-mer in g or -1)"""
    if name == "k31":
        fwd = [g[i:i + 31] for i in range(len(g) - 30)]
        rev = [revcomp(km) for km in fwd]
        kmers = fwd + rev
        assert len(set(kmers)) == len(kmers)
        starts = list(range(len(fwd))) * 2
        return 31, kmers, rs_model.encode_kmers(kmers, 31), np.array(starts, np.int64)
    assert name == "k21"
    starts = [i for i in range(len(g) - 20) if i % 1000 < 700]
    kmers = [g[i:i + 21] for i in starts]
    assert len(set(kmers)) == len(kmers)
    kmers += [kmers[50], kmers[2100]]                  # listed twice (called_rows makes the second pair disagree)
    starts += [starts[50], starts[2100]]
    keys = rs_model.encode_kmers(kmers, 21)
    kmers.append(kmers[5][:10] + b"N" + kmers[5][11:])      # no k-mer: the row has no slot
    return 21, kmers, keys, np.array(starts, np.int64)


def called_rows(name, kmers, starts, how):
    """-> (row_called for the device: u8 per row of the table or None, the same for the rows with a slot -- what the model takes)
    how: "all" (None), "half": the rows of the k-mers that start in the genome's second half are not called, nor those of an
    island of 40 starts in every 1000 of the first half (a clean read over an island has an in-cluster gap).  In "k21" the row that
    lists kmers[2100] again then disagrees with the first (called): the union rule keeps the k-mer called."""
    if how == "all":
        return None, None
    called = ((starts < GENOME_LEN // 2) & ~((starts % 1000 >= 300) & (starts % 1000 < 340))).astype(np.uint8)
    if name == "k21":
        assert starts[-1] >= GENOME_LEN // 2
        called[-1] = 1                                 # kmers[2100] again, called this time; its first row is not
        called[-2] = 0                                 # kmers[50] again, not called this time; its first row is
    full = np.concatenate([called, np.ones(len(kmers) - len(called), np.uint8)])      # (the row without a slot: its flag counts nowhere)
    return full, called


def sub(read, at):
    """`read` with the base at `at` replaced by the next letter"""
    return read[:at] + b"ACGT"[(b"ACGT".index(read[at:at + 1].upper()) + 1) % 4:][:1] + read[at + 1:]


def hand_records(g):
    """name -> (record, what the model must say at k = 31 against table "k31" with every row called: a dict of totals that are
    not zero besides records / assessed / kmers / kmers_called, detectable, windows -- see test_gaps_host)"""
    r = g[1000:1150]
    return {
        "clean": (r, dict(hits_called=120, detectable=88)),
        "sub_75": (sub(r, 75), dict(hits_called=89, misses=31, gap_k=1, sites=1, reads_with_sites=1, detectable=88)),
        "sub_10": (sub(r, 10), dict(hits_called=109, misses=11, detectable=119 - 11 - 31)),
        "deletion": (r[:75] + g[1076:1151], dict(hits_called=90, misses=30, gap_km1=1, sites=1, reads_with_sites=1, detectable=88)),
        "insertion_3": (r[:75] + b"GGG" + r[75:], dict(hits_called=90, misses=33, gap_k_2k=1, sites=1, reads_with_sites=1, detectable=122 - 31)),
        "two_subs": (sub(sub(r, 70), 80), dict(hits_called=79, misses=41, gap_k_2k=1, sites=1, reads_with_sites=1, detectable=88)),
        "n_at_75": (r[:75] + b"N" + r[76:], dict(hits_called=89, detectable=(44 - 31) + (119 - 76 - 31))),
        "short": (g[500:530], dict()),
        "exactly_k": (g[500:531], dict(hits_called=1)),
    }


def in_cluster_case(g):
    """-> (record, the rows' starts that are NOT called): a clean read whose windows 40..80 are k-mers of uncalled rows only"""
    return g[2000:2150], set(range(2040, 2081))


def one_length_reads(g, n=600, seed=3):
    """n reads of 150 bases, ACGTN only: clean ones, substitutions, N's, reads of another genome"""
    rs = np.random.RandomState(seed)
    og = other_genome()
    out = []
    for i in range(n):
        s = rs.randint(0, len(g) - 150)
        r = (og if i % 11 == 0 else g)[s:s + 150]
        for _ in range(i % 4):
            r = sub(r, rs.randint(0, 150))
        if i % 7 == 0:
            a = rs.randint(0, 150)
            r = r[:a] + b"N" + r[a + 1:]
        if i % 29 == 0:
            r = b"N" + r[1:149] + b"N"
        out.append(r)
    return out


def mixed_reads(g, n=300, seed=5):
    """n reads of 20..400 bases: substitutions, deleted and inserted bases, N's, lower case, reads of another genome, and reads that
    cross from the called half of the genome into the other"""
    rs = np.random.RandomState(seed)
    og = other_genome()
    out = []
    for i in range(n):
        ln = int(rs.randint(20, 401))
        src = og if i % 13 == 0 else g
        s = rs.randint(0, len(src) - ln) if i % 5 else min(GENOME_LEN // 2 - ln // 2, len(src) - ln)
        r = src[s:s + ln]
        for _ in range(i % 3):
            r = sub(r, rs.randint(0, len(r)))
        if i % 6 == 0 and ln > 60:
            a = rs.randint(1, ln - 1)
            r = r[:a] + r[a + 1:]
        if i % 8 == 0:
            a = rs.randint(1, len(r))
            r = r[:a] + rand_bases(rs, 1 + i % 4) + r[a:]
        if i % 9 == 0:
            a = rs.randint(0, len(r))
            r = r[:a] + b"N" + r[a + 1:]
        if i % 10 == 0:
            a = rs.randint(0, max(1, len(r) - 40))
            r = r[:a] + r[a:a + 40].lower() + r[a + 40:]
        out.append(r)
    assert min(len(r) for r in out) < 31 and max(len(r) for r in out) > 350
    return out


def block(reads):
    return b"".join(r + b"\n" for r in reads)


def tile_edge_block(g):
    """A file-order block (a position is a byte offset) at k = 31: record 2's gap of 31 windows straddles positions 1023 | 1024;
    record 3's gap begins at 2048, so its flanking C is position 2047, the last window of a tile; record 4 ends at 3072."""
    r1 = g[0:963]                                  # positions 0..962, '\n' at 963
    r2 = sub(g[1000:1400], 75)                     # from 964: the gap is windows 964 + 45 .. 964 + 75 = 1009 .. 1039
    s3 = 964 + len(r2) + 1
    b3 = 2048 + 30 - s3                            # the substituted base of record 3: its gap is windows s3 + b3 - 30 .. s3 + b3
    r3 = sub(g[1500:2300], b3)
    s4 = s3 + len(r3) + 1
    r4 = sub(g[2400:2400 + 3072 - s4], 100)
    blk = block([r1, r2, r3, r4])
    assert s3 + b3 - 30 == 2048 and 60 <= b3 < len(r3) - 60 and len(blk) == 3073 and len(r4) > 200
    return blk


def long_records(g):
    """a 5 000-base and a 70 000-base record: the genome over and over (a junction is a gap of k - 1), a substitution every 700
    bases or so, pairs of them 10 apart, and a few N's"""
    rs = np.random.RandomState(17)
    out = []
    for ln in (5000, 70000):
        r = bytearray((g * (ln // len(g) + 1))[:ln])
        for a in range(350, ln - 100, 700):
            a += int(rs.randint(0, 50))
            r[a:a + 1] = sub(bytes(r[a:a + 1]), 0)
            if (a // 700) % 3 == 0:
                r[a + 10:a + 11] = sub(bytes(r[a + 10:a + 11]), 0)
            if (a // 700) % 10 == 9:
                r[a + 300] = ord("N")
        out.append(bytes(r))
    return out
