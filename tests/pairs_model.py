"""The model of ss_reads_join_pairs_dev and of ss_extract_write_pairs' pair names.

A flat block is its lines, each followed by one '\\n'; a line may be empty.  Pair i is line i of block 1, the byte 'N', line i of
block 2: 'N' ends a k-mer window, so the fragment's hits are its mates' hits added up.  The digest of a pair is that of the joined
record (ss_flat_record_keys, host code).
"""


def lines_of(flat):
    flat = bytes(flat)
    assert not flat or flat.endswith(b"\n")
    return flat.split(b"\n")[:-1]


def join_lines(lines1, lines2):
    assert len(lines1) == len(lines2)
    return [a + b"N" + b for a, b in zip(lines1, lines2)]


def join_flat(flat1, flat2):
    """The joined flat block, in line order and unpadded."""
    return b"".join(r + b"\n" for r in join_lines(lines_of(flat1), lines_of(flat2)))


def pair_digests(L, lines1, lines2):
    """np.uint64[n, 2]: the digest of every pair; `L` is strainscan_amd._lib."""
    return L.flat_record_keys(b"".join(r + b"\n" for r in join_lines(lines1, lines2)))
