"""The model of ss_reads_support that the read-support tests hold the device to.

Split the set's bytes on '\\n' and drop the empty pieces: those are the records.  A hit of a record is a window of k bases, all
in ACGTacgt, whose upper-cased text is one of the table's k-mers.  support_model returns the histogram of hits per record
(the last bin open-ended) and the total.  It is written with numpy so that a (table, set) pair costs milliseconds: windows are
encoded as integers (2 bits per base) and looked up with np.isin; a window that holds any other byte -- '\\n' among them, so no
window crosses records -- is never looked up.
"""
import numpy as np

_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c | 0x20] = _i


def encode_kmers(kmers, k):
    """[bytes of length k] (upper case ACGT) -> np.uint64 keys, the encoding window_keys uses."""
    a = np.frombuffer(b"".join(kmers), np.uint8).reshape(-1, k)
    c = _CODE[a].astype(np.uint64)
    assert (c < 4).all()
    key = np.zeros(len(a), np.uint64)
    for i in range(k):
        key |= c[:, i] << np.uint64(2 * i)
    return key


def kmers_of_fasta(text):
    return [ln for ln in text.split(b"\n") if ln and not ln.startswith(b">")]


def window_keys(text, k):
    """-> (keys u64[n - k + 1], live bool[n - k + 1]) for the windows of `text` (bytes); live: all k bytes are ACGTacgt."""
    c = _CODE[np.frombuffer(text, np.uint8)]
    n = c.size - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, bool)
    bad = np.concatenate(([0], np.cumsum(c == 4)))
    live = (bad[k:] - bad[:-k]) == 0
    c64 = (c & 3).astype(np.uint64)
    key = np.zeros(n, np.uint64)
    for i in range(k):
        key |= c64[i:i + n] << np.uint64(2 * i)
    return key, live


def record_ids(text):
    """-> (id i64[len(text)], n_records): the index of the record each byte belongs to (-1 for '\\n'), records being the
    non-empty pieces of text.split(b'\\n') in order."""
    ids = np.full(len(text), -1, np.int64)
    pos, n = 0, 0
    for piece in text.split(b"\n"):
        if piece:
            ids[pos:pos + len(piece)] = n
            n += 1
        pos += len(piece) + 1
    return ids, n


def hits_per_record(text, table_keys, k):
    ids, n_rec = record_ids(text)
    key, live = window_keys(text, k)
    hit = live & np.isin(key, table_keys)
    return np.bincount(ids[:hit.size][hit], minlength=n_rec).astype(np.int64)


def histogram(per_record, n_bins):
    return np.bincount(np.minimum(per_record, n_bins - 1), minlength=n_bins).astype(np.uint64)


def support_model(text, table_keys, k, n_bins=65):
    per = hits_per_record(text, table_keys, k)
    return histogram(per, n_bins), int(per.sum())
