"""The inputs of the `--em_strains` device tests (tests/test_em_sets_gpu.py), made with numpy alone so that the conditions that keep
those tests from passing vacuously can be checked on the model without a device (tests/test_em_sets_host.py does).

The tables and read sets are those of tests/strain_set_cases.py.  ss_reads_strain_sets_resampled keeps its counters in LDS while
n_replicates << n_strains <= 16384 and folds equal sets within the wave above, so the called strains are 1, 2, 12 (LDS at 1 and 4
replicates, global at 15 and 16), 13 (LDS at 1, global from 4 on) and 16: twelve and thirteen strains are the sixteen-strain table
with the masks cut to their low bits.
"""
import numpy as np

from tests import strain_set_cases as sc

# key -> (table of strain_set_cases.TABLES, called strains)
TABLES = {"n1": ("k31_n1", 1), "n2": ("k31_sampled_n2", 2), "n12": ("k31_dense_n16", 12), "n13": ("k31_dense_n16", 13),
          "n16": ("k31_dense_n16", 16), "whole": ("k31_whole_n2", 2)}
SETW_LDS = 1 << 14              # the counters a workgroup of set_weights_kernel keeps in LDS (ss_strain_sets.hip)
REPS = ((0, 1), (0, 16), (16, 4), (5, 15))      # (first_replicate, n_replicates)
SEEDS = (7, 20)
# (table key, read set, M, the (first, n) pairs, the seeds)
RESAMPLED = (
    [(t, s, 1, REPS, SEEDS) for t in ("n1", "n2", "n12", "n13", "n16") for s in ("packed", "ragged_1")]
    + [("n12", s, 1, ((0, 16), (16, 4)), (7,)) for s in ("file_order", "binned_ascii", "ragged_0", "ragged_1023", "two_slabs", "half_a", "half_b")]
    + [("n13", "two_slabs", 8, ((0, 16), (16, 4)), (7,)), ("n16", "ragged_1023", 8, ((5, 15),), (20,))]
    + [("whole", "long", 1, ((0, 16),), (7,)), ("n12", "long", 1, ((16, 4),), (7,)), ("n12", "empty", 1, ((0, 16), (16, 4)), (7,))]
)
# the sets whose records are too few for the conditions on ties and weights (one record, none)
FEW = ("long", "empty")


def cut(row_sets, vsets, n):
    """the masks of a table cut to strains 1..n"""
    keep = np.uint16((1 << n) - 1)
    return np.asarray(row_sets, np.uint16) & keep, np.asarray(vsets, np.uint16) & keep


def table(key, g):
    """-> (k, n, kmers, row_sets, keys, vsets) as strain_set_cases.table gives them, the masks cut to the key's strains"""
    tname, n = TABLES[key]
    k, _, kmers, row_sets, keys, vsets = sc.table(tname, g)
    row_sets, vsets = cut(row_sets, vsets, n)
    return k, n, kmers, row_sets, keys, vsets


def em_vectors(rng, n_vec, n_sets, n_strains):
    """(counts u64[n_vec, n_sets], masks u16[n_sets]) for ss_em_strain_sets: distinct non-zero masks in a shuffled order -- the
    first n_strains sets (where there is room) the singletons, so that every strain can be told apart -- and counts of mixed
    sizes with zeros among them"""
    space = (1 << n_strains) - 1
    assert 1 <= n_sets <= space
    single = [1 << j for j in range(n_strains)][:n_sets]
    if n_sets > space // 2:
        rest = [m for m in rng.permutation(space) + 1 if m & (m - 1)][:n_sets - len(single)]
    else:
        rest = set()
        while len(rest) < n_sets - len(single):
            m = int(rng.randint(1, space + 1))
            if m & (m - 1):
                rest.add(m)
        rest = sorted(rest)
    masks = np.array(single + [int(m) for m in rest], np.uint16)
    masks = masks[rng.permutation(masks.size)]
    assert masks.size == n_sets and np.unique(masks).size == n_sets
    counts = rng.randint(0, 2000, size=(n_vec, n_sets)).astype(np.uint64)
    counts[rng.random_sample((n_vec, n_sets)) < 0.3] = 0
    big = rng.random_sample((n_vec, n_sets)) < 0.05
    counts[big] *= np.uint64(100000)
    return counts, masks
