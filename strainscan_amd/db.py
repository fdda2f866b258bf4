"""On-disk StrainScan databases -> device images.

Tree_database/ (written by the reference's library/Build_tree.py:494-526,648-698):
    kmer.fa                 `>1\\n<31-mer>\\n` per row
    kmers/<id>              space separated 0-based rows of kmer.fa, one line
    node_length.txt         `id \\t len`
    reconstructed_nodes.txt one id per line
    overlapping_info/<leaf>, <leaf>_supple
Kmer_Sets_L2/Kmer_Sets/C<id>/ is handled by strainscan_amd/Vote_Strain_L2_Lasso_new_sp.py (cluster image cache there).

A TreeImage owns the device k-mer table of kmer.fa and the node row lists; scans accumulate in
it.  Images are cached per (directory, key mode) for the life of the process so that the cutoff
ladder of StrainScan.py:196-216 (which calls identify_cluster up to twice) parses and uploads a
database once.  The sample's reads live here as well: one resident set at a time (resident_reads,
with -q's line about what the load masked), the scans of a table over them, and the image caches.
The opt-in reports about the reads (--read_support, -x, --by_strain, --bootstrap) are read_reports.py.
"""
import os
import threading

import numpy as np

from . import _lib

L1_K = 31  # the reference hard-codes `-m 31` for the tree scan (identify.py:82,86)


class CountsView:
    """`match_results` of library/identify.py:96-101 without materialising a dict: a read-only
    mapping row -> count over the per-row arrays (only valid rows are keys)."""

    def __init__(self, counts, valid):
        self.counts = counts
        self.valid = valid

    def __getitem__(self, row):
        if not self.valid[row]:
            raise KeyError(row)
        return int(self.counts[row])

    def __contains__(self, row):
        return 0 <= row < self.valid.size and bool(self.valid[row])

    def __len__(self):
        return int(self.valid.sum())

    def keys(self):
        return np.nonzero(self.valid)[0]

    def __iter__(self):
        return iter(self.keys().tolist())

    def items(self):
        k = self.keys()
        return zip(k.tolist(), self.counts[k].tolist())

    def get(self, row, default=None):
        return int(self.counts[row]) if row in self else default


_READS = {}          # one resident read set at a time: key -> _lib.ReadSet
_READS_LOCK = threading.Lock()
RESIDENT_LIMIT_BYTES = int(float(os.environ.get("SS_READS_RESIDENT_GB", "160")) * 1e9)


def _reads_key(paths, rank, world):
    # (the base-quality mask is part of what a set holds: the same files under another threshold are another set)
    return tuple((os.path.abspath(p), os.path.getmtime(p), os.path.getsize(p)) for p in paths if p) + (rank, world, _lib.get_min_base_qual())


MASK_REPORT = {"on": False, "done": False}      # the commands' -q line (StrainScan.apply_min_base_qual turns it on)


def report_mask(masked=None, no_qual=None, bases=None):
    """-q's one line on stderr: right after the load of the resident reads (its own figures), or -- reads that were streamed
    for every scan -- at the end of the command, over all passes.  Once per process."""
    q = _lib.get_min_base_qual()
    if not MASK_REPORT["on"] or MASK_REPORT["done"] or not q:
        return
    MASK_REPORT["done"] = True
    import sys
    from . import dist
    rank, world = dist.rank_world()
    if masked is None:
        c = _lib.mask_counters()
        masked, no_qual = c["masked"], c["bam_no_qual"]
    line = "min_base_qual %d: %d bases masked" % (q, masked)
    if bases:
        line += " of %d read (%.3f %%)" % (bases, 100.0 * masked / bases)
    else:
        line += " (over every pass of the streamed input)"
    if no_qual:
        line += "; %d BAM records carried no qualities and were not masked" % no_qual
    if world > 1:
        line = "rank %d of %d (its share): " % (rank, world) + line
    print(line, file=sys.stderr)
    sys.stderr.flush()


def resident_reads(paths):
    """The sample's reads as flat base blocks in HBM (parsed and copied over PCIe once), or None
    when they would not fit the budget (then every scan streams the files again).  Under
    torch.distributed each rank keeps only its shard of the blocks."""
    from . import dist
    rank, world = dist.rank_world()
    total = sum(os.path.getsize(p) for p in paths if p)
    gz = any(str(p).endswith(".gz") or _lib.input_kind(p) == "bam" for p in paths if p)      # (a BAM: budgeted like a .gz)
    if (total * (4 if gz else 1)) / world > RESIDENT_LIMIT_BYTES or RESIDENT_LIMIT_BYTES <= 0:
        return None
    key = _reads_key(paths, rank, world)
    with _READS_LOCK:                     # layer 2 asks from several threads; the set is parsed once
        rs = _READS.get(key)
        if rs is None:
            for old in _READS.values():
                old.close()
            _READS.clear()
            _close_pairs()
            _close_ordered()
            # (.gz under torch.distributed: all ranks take the same inflate path for a file, dist.load_agreed)
            before = _lib.mask_counters() if MASK_REPORT["on"] else None
            rs = dist.load_agreed([p for p in paths if p], lambda use: _lib.ReadSet(use, rank, world), discard=lambda r: r.close())
            _READS[key] = rs
            if before is not None:
                after, inf = _lib.mask_counters(), rs.info()
                report_mask(after["masked"] - before["masked"], after["bam_no_qual"] - before["bam_no_qual"],
                            inf["n_bases"] - inf["n_records"])
    return rs


_PAIRS = {}          # the joined pairs of the resident sample (--pairs): key -> _lib.ReadSet, closed with the resident set


def _close_pairs():
    for old in _PAIRS.values():
        old.close()
    _PAIRS.clear()


def resident_pairs(paths):
    """(set, None): the sample's read PAIRS as the records of a second resident set -- record i of the first file, an N, record i
    of the second (ReadSet.load_pairs); or, for one BAM, the fragments its mates make by name and flag (ReadSet.load_pairs_bam) --
    cached beside the resident reads and closed with them; or (None, why) where it is not built: one file that is no BAM, two BAMs
    or a BAM beside a FASTQ, several ranks, the plain sample not resident, no room for a second copy of the bases, unequal record
    counts, a BAM whose names are not one first and one second mate.  The scans never use it: it serves the per-read reports
    (read_reports, --pairs).  One line on stderr after the join: the pairs (a BAM: the orphans and singles too) and the bytes of
    the set."""
    import sys
    from . import dist
    rank, world = dist.rank_world()
    ps = [p for p in paths if p]
    bam = len(ps) == 1 and _lib.input_kind(ps[0]) == "bam"
    if len(ps) != 2 and not bam:
        return None, "needs the two files of a paired sample (-i and -j)"
    if not bam and any(_lib.input_kind(p) != "fastx" for p in ps):
        return None, "takes FASTA/FASTQ inputs (the mates of a pair are not adjacent in a coordinate-sorted BAM; pairs from BAM are not built)"
    if world > 1:
        return None, "runs on one rank only (this run has several)"
    rs = resident_reads(paths)
    if rs is None:
        return None, "needs the sample resident on the device (SS_READS_RESIDENT_GB)"
    key = _reads_key(paths, rank, world)
    with _READS_LOCK:
        js = _PAIRS.get(key)
        if js is not None:
            return js, None
        inf = rs.info()
        # the load's peak beside the resident reads: the two flat blocks, the joined slab and its binned copy, each at most the
        # bases and their line ends as ASCII; a BAM: its one flat block and, budgeted as resident_reads does, the inflated stream
        no_room = "has no room for the joined pairs beside the resident reads (SS_READS_RESIDENT_GB)"
        peak = 3 * (inf["n_bases"] + inf["n_records"]) + (4 * os.path.getsize(ps[0]) if bam else 0)
        if inf["device_bytes"] + peak > RESIDENT_LIMIT_BYTES:
            return None, no_room
        try:
            js = _lib.ReadSet.load_pairs_bam(ps[0]) if bam else _lib.ReadSet.load_pairs(ps[0], ps[1])
        except _lib.SSError as e:
            if e.code == _lib.SS_ENOMEM:        # (the device holds other things than this budget knows of)
                return None, no_room
            if e.code != _lib.SS_EIO:
                raise
            if bam:
                bad = getattr(e, "pair_counters", {}).get("violating", 0)
                if not bad:
                    raise
                return None, "has read names that are not one first and one second mate (%d records)" % bad
            return None, "could not pair the records of the two files (unequal record counts, or a file that cannot be read)"
        _close_pairs()
        _PAIRS[key] = js
        ji = js.info()
        if bam:
            c = js.pair_counters
            print("pairs: %d pairs joined\t%d orphans\t%d singles\t%d bytes on the device" %
                  (c["pairs"], c["orphans"], c["singles"], ji["device_bytes"]), file=sys.stderr)
        else:
            print("pairs: %d pairs joined\t%d bytes on the device" % (ji["n_records"], ji["device_bytes"]), file=sys.stderr)
        sys.stderr.flush()
    return js, None


_ORDERED = {}        # the sample once more in FILE order (--read_calls): key -> [_lib.ReadSet], closed with the resident set


def _close_ordered():
    for sets in _ORDERED.values():
        for rs in sets:
            rs.close()
    _ORDERED.clear()


def ordered_reads(paths, pairs=False):
    """(sets, None): the sample's files each as one slab in FILE ORDER (ReadSet.load_ordered), one set per file -- or, with
    `pairs`, ONE set of the two files' records joined in line order (ReadSet.load_pairs(order=False)) --, cached beside the
    resident reads and closed with them; or (None, why) where they are not built: several ranks, an input that is no
    FASTA/FASTQ, `pairs` without two files, the plain sample not resident, no room for another copy of the bases, unequal record
    counts.  The scans never use them: they serve --read_calls (read_reports), which needs record i of a set to be record i of
    its file."""
    from . import dist
    rank, world = dist.rank_world()
    ps = [p for p in paths if p]
    if world > 1:
        return None, "runs on one rank only (this run has several)"
    if any(_lib.input_kind(p) != "fastx" for p in ps):
        return None, "takes FASTA/FASTQ inputs"
    if pairs and len(ps) != 2:
        return None, "needs the two files of a paired sample (-i and -j) under --pairs"
    rs = resident_reads(paths)
    if rs is None:
        return None, "needs the sample resident on the device (SS_READS_RESIDENT_GB)"
    key = _reads_key(paths, rank, world) + (bool(pairs),)
    with _READS_LOCK:
        sets = _ORDERED.get(key)
        if sets is not None:
            return sets, None
        inf = rs.info()
        held = inf["device_bytes"] + sum(js.info()["device_bytes"] for js in _PAIRS.values())
        # the load's peak: the flat blocks of the files and the slab they are copied into, each the bases and their line ends
        no_room = "has no room for the sample in file order beside the resident reads (SS_READS_RESIDENT_GB)"
        if held + 2 * (inf["n_bases"] + inf["n_records"]) > RESIDENT_LIMIT_BYTES:
            return None, no_room
        sets = []
        try:
            if pairs:
                sets.append(_lib.ReadSet.load_pairs(ps[0], ps[1], order=False))
            else:
                for p in ps:
                    sets.append(_lib.ReadSet.load_ordered(p))
        except _lib.SSError as e:
            for s in sets:
                s.close()
            if e.code == _lib.SS_ENOMEM:
                return None, no_room
            if e.code != _lib.SS_EIO:
                raise
            return None, ("could not pair the records of the two files (unequal record counts, or a file that cannot be read)" if pairs
                          else "could not read the sample's files once more")
        _close_ordered()
        _ORDERED[key] = sets
    return sets, None


def prefetch_reads(paths):
    """Start loading the sample's reads (parse || PCIe, binning) on a worker thread WHILE the caller loads the database
    image -- both are native calls that leave the interpreter lock alone, and neither needs the other: the cached
    identify_cluster() call on 16 M reads is image 0.10 s + reads 0.07 s one after the other.  One process only (under
    torch.distributed both sides run collectives, whose order must be the same on every rank); a failure here is raised
    again by the load that follows."""
    from . import dist
    if dist.is_distributed():
        return None
    ps = [p for p in paths if p]
    if not ps or not all(os.path.exists(p) for p in ps):
        return None

    def work():
        try:
            resident_reads(paths)
        except BaseException:               # noqa: B902 -- the caller's own resident_reads() raises it again
            pass

    th = threading.Thread(target=work, name="ss-prefetch-reads")
    th.start()
    return th


def scan_into(kdb, paths, allreduce=True):
    """Count kdb's k-mers in the reads of `paths`: resident blocks when possible, streaming
    otherwise.  Under torch.distributed every rank scans its share of the reads; with `allreduce` the row counts are
    then summed over the ranks (RCCL) and loaded back, without it the table keeps this rank's counts (the tree scan:
    TreeImage exchanges the touched nodes' counts instead, dist.exchange_touched)."""
    from . import dist
    kdb.reset()
    rs = resident_reads(paths)
    if rs is not None:
        rs.scan_into(kdb)
        if allreduce and dist.is_distributed():
            dist.allreduce_table(kdb)
    elif dist.is_distributed():
        dist.scan_files_sharded(kdb, paths, allreduce=allreduce)
    else:
        kdb.scan_files([p for p in paths if p])


INDEX_EVENTS = {"built": 0, "imported": 0}       # device indexes built from keys / imported from an image, this process


def rank0_first(fn):
    """Several ranks and an image cache: rank 0 runs fn() first -- it parses / builds and EXPORTS whatever image is
    missing -- the others wait at a barrier and then run the same fn(), which now finds the image and imports it:
    one host-side index build per node instead of one per rank (an E. coli tree: ~1 s of all the box's CPUs each).
    The barrier is unconditional (every rank takes it once per call), so the ranks cannot disagree about it; a rank
    that finds no image after all (cache not writable) simply builds its own."""
    from . import dist
    if not dist.is_distributed() or not _cache_dir():
        return fn()
    import torch
    import torch.distributed as td
    rank, _ = dist.rank_world()
    dev = "cuda" if torch.cuda.is_available() and td.get_backend() == "nccl" else "cpu"

    def agree(ok):
        """MIN over the ranks of a success flag: doubles as the barrier, and a rank that failed is seen by all (the others
        would otherwise go on into the scan's collectives with one rank missing, and hang there)."""
        t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
        td.all_reduce(t, op=td.ReduceOp.MIN)
        return bool(int(t.item()))

    out, err = None, None
    if rank == 0:
        try:
            out = fn()
            wait_cache_writes()
        except Exception as e:              # raised below, after the other ranks have been told; KeyboardInterrupt /
            err = e                         # SystemExit leave at once (a rank on its way out must not enter a collective)
    if not agree(err is None):              # rank 0's turn
        raise err if err is not None else RuntimeError("rank 0 failed while building the database image")
    if rank != 0:
        try:
            out = fn()
        except Exception as e:
            err = e
    if not agree(err is None):              # everybody else's
        raise err if err is not None else RuntimeError("another rank failed while loading the database image")
    return out


def fasta_index(path, k, upper_keys):
    """Device index of a k-mer FASTA (a cluster's all_kmer.fasta): imported from the image cache when there is
    one for this file (path, size, mtime, k, key convention), else parsed, built and exported.  Only the
    minimizer-paged layout (17 <= k <= 31) has an image; a flat table (k <= 16) is built every time."""
    return rank0_first(lambda: _fasta_index(path, k, upper_keys))


def _fasta_index(path, k, upper_keys):
    cdir = _cache_dir()
    img = None
    st = os.stat(path)                                   # (a cluster without its k-mer set: FileNotFoundError, as the reference's open() raises)
    if cdir and 17 <= int(k) <= 31:
        tag = cache_tag("%s|%d|%d|%d|%d" % (os.path.realpath(path), st.st_size, st.st_mtime_ns, int(k),
                                                 int(upper_keys)))
        img = os.path.join(cdir, "index_%s.bin" % tag)
        if os.path.exists(img):
            try:
                kdb = _lib.KmerDB.from_image(img)
                INDEX_EVENTS["imported"] += 1
                return kdb
            except RuntimeError:
                pass
    kdb = _lib.KmerDB.from_fasta(path, int(k), upper_keys=upper_keys)
    INDEX_EVENTS["built"] += 1
    if img:
        try:
            _export_image(kdb, cdir, img)
        except (RuntimeError, OSError):
            pass
    return kdb


def _export_image(kdb, cdir, img):
    os.makedirs(cdir, exist_ok=True)
    tmp = _cache_tmp(img)
    try:
        kdb.export(tmp)
        os.replace(tmp, img)
    except BaseException:
        _unlink_quiet(tmp)
        raise


def _export_image_later(kdb, cdir, img):
    """The 0.9 GB image of an E. coli tree takes 0.25 s to read back and write: on a worker thread (like the tree cache),
    while the reads are scanned -- it only reads the index arrays, scans only add to the counters.  The handle must outlive
    the writer: wait_cache_writes() runs before an image is dropped (tree_image, clear_cache, TreeImage.__del__)."""

    def work():
        try:
            _export_image(kdb, cdir, img)
        except (RuntimeError, OSError):
            pass

    with _CACHE_WRITERS_LOCK:
        old = _CACHE_WRITERS.get(img)
    if old is not None:
        old.join()
    th = threading.Thread(target=work, name="ss-export-image")
    with _CACHE_WRITERS_LOCK:
        _CACHE_WRITERS[img] = th
    th.start()


def cache_tag(text):
    """Name of a cache entry from the string that identifies it (path | size | mtime | ...): 128 bits of a multiplicative
    mix over the bytes, two lanes with different odd multipliers (non-linear in the input, unlike a CRC: the tag is the only
    identity of an entry).  Not hashlib: importing it costs a fresh CLI process 0.05-0.1 s (OpenSSL) for what is a file name;
    the strings are ~150 bytes."""
    b = text.encode()
    M = (1 << 64) - 1
    h1, h2 = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F
    b += b"\x80" + b"\0" * (-(len(b) + 1) % 8)
    for i in range(0, len(b), 8):
        w = int.from_bytes(b[i:i + 8], "little")
        h1 = ((h1 ^ w) * 0xFF51AFD7ED558CCD) & M
        h1 ^= h1 >> 32
        h2 = ((h2 + w) * 0xD6E8FEB86659FD93) & M
        h2 ^= h2 >> 29
    h1 = ((h1 ^ len(text)) * 0xC4CEB9FE1A85EC53) & M
    h2 = ((h2 ^ h1) * 0x9FB21C651E98DF25) & M
    return "%016x%016x" % (h1 ^ (h1 >> 33), h2 ^ (h2 >> 31))


def _cache_dir():
    d = os.environ.get("SS_IMAGE_CACHE", os.path.join(os.path.expanduser("~"), ".cache", "strainscan_amd"))
    return None if d in ("", "0", "off") else d


class TreeArrays:
    """kmer.fa + kmers/<id> as arrays.  keys u64[n] / flags u8[n]: the encoded rows of kmer.fa (only needed
    to BUILD the device index); ids: node ids ascending; lists[i]: rows of node ids[i] in FILE order
    (adjust_profile indexes them); urows / uoffs: the same lists de-duplicated and sorted, back to back
    (what the device-side NodeSet holds: set(map(int, ...)) at identify.py:118)."""

    def __init__(self, keys, flags, ids, rows, offs, urows, uoffs):
        self.keys, self.flags, self.ids = keys, flags, ids
        self.rows, self.offs, self.urows, self.uoffs = rows, offs, urows, uoffs
        self.lists = [rows[offs[i]:offs[i + 1]] for i in range(len(ids))]


_TREE_MAGIC = b"SSTREE02"


def _pad64(n):
    return (n + 63) & ~63


def _write_tree_cache(path, t):
    """One raw file, arrays at 64-byte aligned offsets (read back through one memory map: no decompression,
    no checksum pass, and the 8-byte keys are only paged in when the device index has to be rebuilt)."""
    same = t.urows is t.rows
    arrays = [np.asarray(t.ids, np.int64), np.asarray(t.offs, np.int64), np.asarray(t.rows, np.uint32),
              np.asarray(t.uoffs, np.int64), np.zeros(0, np.uint32) if same else np.asarray(t.urows, np.uint32),
              np.asarray(t.flags, np.uint8), np.asarray(t.keys, np.uint64)]
    hdr = np.array([t.keys.size, len(t.ids), t.rows.size, 0 if same else t.urows.size, int(same), 0], np.uint64)
    tmp = _cache_tmp(path)
    try:
        with open(tmp, "wb") as f:
            f.write(_TREE_MAGIC)
            f.write(hdr.tobytes())
            pos = 8 + hdr.nbytes
            for a in arrays:
                f.write(b"\0" * (_pad64(pos) - pos))
                pos = _pad64(pos)
                f.write(memoryview(np.ascontiguousarray(a)).cast("B"))
                pos += a.nbytes
        os.replace(tmp, path)
    except BaseException:
        _unlink_quiet(tmp)
        raise


def _cache_tmp(path):
    """A temp file of its own in the cache directory for every writer (thread or process): `path.<pid>.tmp` was shared
    by two writer threads of one process, the second truncating what the first was still writing.  The finished
    file reaches `path` through os.replace, so a reader sees the old image, none, or a complete new one."""
    import tempfile
    fd, tmp = tempfile.mkstemp(dir=os.path.dirname(path), prefix=os.path.basename(path) + ".", suffix=".tmp")
    os.close(fd)
    return tmp


def _unlink_quiet(p):
    try:
        os.unlink(p)
    except OSError:
        pass


_CACHE_WRITERS = {}                  # cache path -> thread writing it
_CACHE_WRITERS_LOCK = threading.Lock()


def _write_tree_cache_later(cdir, path, t):
    """The tree cache is written on a worker thread (0.2 s for an E. coli tree) while the first scan runs.  At most
    one writer per path: load_tree() of the same database joins it before it looks for the file (`-b 1` on a new
    database loads the tree twice, identify_low_depth.py:119 then identify.py:402); the interpreter waits for the
    writers at exit, wait_cache_writes() before that."""

    def work():
        try:
            os.makedirs(cdir, exist_ok=True)
            _write_tree_cache(path, t)
        except OSError:
            pass

    with _CACHE_WRITERS_LOCK:
        old = _CACHE_WRITERS.get(path)
    if old is not None:
        old.join()
    th = threading.Thread(target=work)
    with _CACHE_WRITERS_LOCK:
        _CACHE_WRITERS[path] = th
    th.start()


def _join_cache_writer(path):
    with _CACHE_WRITERS_LOCK:
        th = _CACHE_WRITERS.get(path)
    if th is not None:
        th.join()
        with _CACHE_WRITERS_LOCK:
            if _CACHE_WRITERS.get(path) is th:
                del _CACHE_WRITERS[path]


def wait_cache_writes():
    while True:
        with _CACHE_WRITERS_LOCK:
            paths = list(_CACHE_WRITERS)
        if not paths:
            return
        for p in paths:
            _join_cache_writer(p)


def _read_tree_cache(path):
    size = os.path.getsize(path)
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    if size < 56 or bytes(mm[:8]) != _TREE_MAGIC:
        raise ValueError("not a tree cache")
    n_rows, n_ids, n_total, n_utotal, same, _ = (int(x) for x in np.frombuffer(mm[8:56], np.uint64))
    pos = [56]

    def take(dtype, n):
        o = _pad64(pos[0])
        nb = n * np.dtype(dtype).itemsize
        if o + nb > size:
            raise ValueError("truncated tree cache")
        pos[0] = o + nb
        return mm[o:o + nb].view(dtype)

    ids = take(np.int64, n_ids).tolist()
    offs = np.array(take(np.int64, n_ids + 1))
    rows = take(np.uint32, n_total)
    uoffs = np.array(take(np.int64, n_ids + 1))
    urows = take(np.uint32, n_utotal)
    flags = take(np.uint8, n_rows)
    keys = take(np.uint64, n_rows)
    if pos[0] != size or offs[-1] != n_total or uoffs[-1] != (n_total if same else n_utotal):
        raise ValueError("inconsistent tree cache")
    return TreeArrays(keys, flags, ids, rows, offs, rows if same else urows, uoffs)


def _node_lists_native(kdir, ids, n_rows):
    """The same through ss_node_lists_parse (the host's threads: 40 ms for the 1645 files of an E. coli tree where numpy
    takes 0.7 s); None when a file holds anything but row numbers of kmer.fa -- the loop below then raises what it raises."""
    ida = np.ascontiguousarray(ids, np.int64)
    counts = np.zeros(ida.size, np.uint64)
    bad = _lib.C.c_uint32()
    if _lib.lib().ss_node_lists_parse(os.fsencode(kdir), _lib.ptr(ida), ida.size, int(n_rows), _lib.ptr(counts), None, None,
                                      _lib.C.byref(bad)) != _lib.SS_OK:
        return None
    offs = np.zeros(ida.size + 1, np.int64)
    np.cumsum(counts.astype(np.int64), out=offs[1:])
    rows = np.empty(int(offs[-1]), np.uint32)
    uoffs = offs.astype(np.uint64)
    if _lib.lib().ss_node_lists_parse(os.fsencode(kdir), _lib.ptr(ida), ida.size, int(n_rows), _lib.ptr(counts), _lib.ptr(uoffs),
                                      _lib.ptr(rows), _lib.C.byref(bad)) != _lib.SS_OK:
        return None
    # set(map(int, ...)) of identify.py:118: lists that are already strictly increasing (the builder writes them so) are
    # their own de-duplicated form
    inc = rows[1:] > rows[:-1] if rows.size > 1 else np.ones(0, bool)
    if rows.size > 1:
        inner = offs[1:-1]
        inc[inner[(inner > 0) & (inner < rows.size)] - 1] = True
    if inc.all():
        return rows, offs, rows, offs
    ul = [np.unique(rows[offs[i]:offs[i + 1]]) for i in range(ida.size)]
    uo = np.zeros(ida.size + 1, np.int64)
    for i, r in enumerate(ul):
        uo[i + 1] = uo[i] + r.size
    return rows, offs, (np.concatenate(ul) if ul else np.zeros(0, np.uint32)), uo


def _node_lists(db_dir, ids, n_rows):
    """kmers/<id> (one line of row numbers each, identify.py:116-118) -> rows in file order, their offsets, and the
    de-duplicated sorted form the node statistics use."""
    kdir = os.path.join(db_dir, "kmers")
    native = _node_lists_native(kdir, ids, n_rows)
    if native is not None:
        return native
    lists = []
    for i in ids:
        with open(os.path.join(kdir, str(i)), "rb") as f:
            first = f.readline()
        r = (np.array(first.split(), dtype=np.int64) if len(first) < 4096 else np.fromstring(first, dtype=np.int64, sep=" "))
        if r.size and (r.min() < 0 or r.max() >= max(1, n_rows)):
            raise ValueError("%s/kmers/%d lists a row outside kmer.fa" % (db_dir, i))
        lists.append(r.astype(np.uint32))
    offs = np.zeros(len(ids) + 1, np.int64)
    for i, r in enumerate(lists):
        offs[i + 1] = offs[i] + r.size
    rows = np.concatenate(lists) if lists else np.zeros(0, np.uint32)
    # set(map(int, ...)) of identify.py:118: lists that are already strictly increasing (the builder writes them
    # so) are their own de-duplicated form
    inc = rows[1:] > rows[:-1] if rows.size > 1 else np.ones(0, bool)
    if rows.size > 1:
        inc[offs[1:-1][(offs[1:-1] > 0) & (offs[1:-1] < rows.size)] - 1] = True
    if inc.all():
        urows, uoffs = rows, offs
    else:
        ul = [np.unique(r) for r in lists]
        uoffs = np.zeros(len(ids) + 1, np.int64)
        for i, r in enumerate(ul):
            uoffs[i + 1] = uoffs[i] + r.size
        urows = np.concatenate(ul) if ul else np.zeros(0, np.uint32)
    return rows, offs, urows, uoffs


def load_tree(db_dir, k=L1_K, with_keys=None):
    """kmer.fa + kmers/<id> -> TreeArrays.  The text/directory parse (tens of millions of tokens) is done
    once per database: a binary image is kept under SS_IMAGE_CACHE (default ~/.cache/strainscan_amd), keyed
    by the database path, size and mtime of kmer.fa.

    `with_keys(keys, flags)`: called on this thread as soon as kmer.fa is encoded -- the caller builds the device index
    there (native code, the interpreter lock is free) WHILE a worker thread parses the 1645 node files (numpy, 0.7 s
    for an E. coli tree); its result comes back as the second element of the returned pair."""
    fa = os.path.join(db_dir, "kmer.fa")
    st = os.stat(fa)
    kdir = os.path.join(db_dir, "kmers")
    tag = cache_tag("%s|%d|%d|%d|%d" % (os.path.realpath(db_dir), st.st_size, st.st_mtime_ns, k,
                                             os.stat(kdir).st_mtime_ns))
    cdir = _cache_dir()
    path = os.path.join(cdir, "tree_%s.bin" % tag) if cdir else None
    if path:
        _join_cache_writer(path)          # an earlier load_tree of this database may still be writing it
    if path and os.path.exists(path):
        try:
            t = _read_tree_cache(path)
            return (t, with_keys(t.keys, t.flags)) if with_keys else t
        except (ValueError, OSError):
            pass
    n = _lib.C.c_uint64()
    _lib.check(_lib.lib().ss_kmerfa_count_rows(os.fsencode(fa), _lib.C.byref(n)), "ss_kmerfa_count_rows(%s)" % fa)
    keys = np.empty(n.value, np.uint64)
    flags = np.empty(n.value, np.uint8)
    _lib.check(_lib.lib().ss_kmerfa_encode(os.fsencode(fa), int(k), n.value, _lib.ptr(keys), _lib.ptr(flags), 0),
               "ss_kmerfa_encode(%s)" % fa)
    ids = sorted(int(f) for f in os.listdir(kdir) if f.isdigit())
    extra = None
    if with_keys:
        import threading
        box = {}

        def work():
            try:
                box["lists"] = _node_lists(db_dir, ids, n.value)
            except BaseException as e:  # noqa: B902 -- handed to the caller's thread
                box["err"] = e

        th = threading.Thread(target=work)
        th.start()
        try:
            extra = with_keys(keys, flags)
        finally:
            th.join()
        if "err" in box:
            raise box["err"]
        rows, offs, urows, uoffs = box["lists"]
    else:
        rows, offs, urows, uoffs = _node_lists(db_dir, ids, n.value)
    t = TreeArrays(keys, flags, ids, rows, offs, urows, uoffs)
    if path:
        _write_tree_cache_later(cdir, path, t)
    return (t, extra) if with_keys else t


def load_tree_text(db_dir, k=L1_K):
    """-> (keys u64[n], flags u8[n], node ids, node row lists in FILE order); see load_tree."""
    t = load_tree(db_dir, k)
    return t.keys, t.flags, t.ids, t.lists


class TreeImage:
    def __init__(self, db_dir, upper_keys=True):
        self.db_dir = db_dir
        self.upper_keys = upper_keys
        t, self.kdb = rank0_first(lambda: load_tree(db_dir, L1_K, with_keys=lambda keys, flags:
                                                    self._index(db_dir, keys, flags, upper_keys)))
        self.node_ids = list(t.ids)
        self.node_rows = dict(zip(t.ids, t.lists))   # id -> rows in FILE order (adjust_profile indexes it)
        self.node_index = {i: j for j, i in enumerate(self.node_ids)}
        self.nodes = _lib.NodeSet.from_sorted(t.urows, t.uoffs)
        self._scanned = None          # key of the inputs whose counts are in the table
        self._counts = None
        self._stats = None
        self._rows_global = True      # False: several ranks, the table holds THIS rank's counts only

    def __del__(self):
        try:
            wait_cache_writes()      # the index may still be on its way to the image cache
        except Exception:            # noqa: B902 -- interpreter shutdown
            pass

    @staticmethod
    def _index(db_dir, keys, flags, upper_keys):
        """Device index of kmer.fa: imported from the image cache when present, else built and exported."""
        cdir = _cache_dir()
        path = None
        if cdir:
            st = os.stat(os.path.join(db_dir, "kmer.fa"))
            tag = cache_tag("%s|%d|%d|%d|%d" % (os.path.realpath(db_dir), st.st_size, st.st_mtime_ns, L1_K,
                                                     int(upper_keys)))
            path = os.path.join(cdir, "index_%s.bin" % tag)
            if os.path.exists(path):
                try:
                    kdb = _lib.KmerDB.from_image(path)
                    if kdb.n_rows == keys.size:
                        INDEX_EVENTS["imported"] += 1
                        return kdb
                    kdb.close()
                except RuntimeError:
                    pass
        kdb = _lib.KmerDB(keys, flags, L1_K, upper_keys)
        INDEX_EVENTS["built"] += 1
        if path:
            _export_image_later(kdb, cdir, path)
        return kdb

    # -- scanning ---------------------------------------------------------------------------
    def scan(self, paths):
        """Count the table's k-mers in the given FASTA/FASTQ(.gz) files (replaces the
        `jellyfish count` + `dump -c` pair, identify.py:82-87)."""
        key = _scan_key(paths)
        if self._scanned == key:
            return
        scan_into(self.kdb, paths, allreduce=False)
        self._mark_scanned(key)

    def _mark_scanned(self, key):
        """The table holds the counts of the inputs `key` (this rank's share of them under torch.distributed)."""
        from . import dist
        self._rows_global = not dist.is_distributed()
        self._scanned = key
        self._counts = None
        self._stats = None

    def mark_external(self, tag):
        """The table now holds counts produced elsewhere (multi-GPU: every rank scanned a shard,
        the row vectors were all-reduced and loaded back with KmerDB.load_counts_rows_dev)."""
        self._scanned = ("external", tag)
        self._counts = None
        self._stats = None
        self._rows_global = True

    @property
    def is_external(self):
        return bool(self._scanned) and self._scanned[0] == "external"

    def _global_rows(self):
        """Several ranks: single rows are asked for (adjust_profile's Poisson branch, identify.py:203-218; the `remain`
        set, :181-189) -> now the whole row vector is summed over the ranks and loaded back.  A collective: every rank
        runs the same walk on the same node statistics, so all of them get here at the same point."""
        if not self._rows_global:
            from . import dist
            self.node_stats()                     # while the table still holds this rank's own counts
            dist.allreduce_table(self.kdb)
            self._rows_global = True

    @property
    def counts(self):
        if self._counts is None:
            self._global_rows()
            self._counts = self.kdb.counts_rows()
        return self._counts

    @property
    def valid(self):
        return self.kdb.row_valid

    def match_results(self):
        return CountsView(self.counts, self.valid)

    def node_stats(self):
        """match_node + del_outlier for every node in one launch (identify.py:106-127)."""
        if self._stats is None:
            # harvest path (ss_nodes.hip): one streaming pass over the counters, reductions over the nodes with hits;
            # several ranks: their counts are exchanged in between (a few MB instead of the row vector)
            from . import dist
            between = None
            if not self._rows_global:
                between = lambda ns: dist.exchange_touched(ns, device=dist.exchange_device())    # noqa: E731
            self._stats = self.nodes.harvest(self.kdb, between)
        return self._stats

    def rows_stat(self, rows):
        """Ad-hoc row set (adjust_profile's `remain`, identify.py:181-189)."""
        self._global_rows()
        return _lib.rows_reduce(self.kdb, rows)


def _scan_key(paths):
    return tuple((os.path.abspath(p), os.path.getmtime(p), os.path.getsize(p)) for p in paths if p) + (("min_base_qual", _lib.get_min_base_qual()),)


def scan_images(images, paths):
    """Count the sample's reads against the tables of several TreeImages in ONE pass over the resident reads
    (ReadSet.scan_into_many: a tile's codes and minimizers are made once, every table behind its own Bloom filter), and mark
    each image as holding this sample's counts, so that its own scan(paths) -- the walk's, -b's -- is a no-op.  Under
    torch.distributed every rank scans its shard; the walk then exchanges the touched nodes per image (node_stats).
    Returns False, and scans nothing, when the reads do not fit the resident budget: every image then scans the files
    itself when it is asked to."""
    key = _scan_key(paths)
    todo = [img for img in images if img._scanned != key]
    if not todo:
        return True
    rs = resident_reads(paths)
    if rs is None:
        return False
    for img in todo:
        img.kdb.reset()
    rs.scan_into_many([img.kdb for img in todo])
    for img in todo:
        img._mark_scanned(key)
    return True


_CACHE = {}
_PINNED = {}         # key -> TreeImage held resident by pinned_images(), whatever _CACHE does meanwhile


def _image_key(db_dir, upper_keys):
    return (os.path.realpath(db_dir), bool(upper_keys), os.path.getmtime(os.path.join(db_dir, "kmer.fa")))


class pinned_images:
    """`with pinned_images([(tree_db_dir, upper_keys), ...], reads=paths) as imgs:` several database images resident together
    (one per entry, in order): inside the scope tree_image(dir, upper_keys) returns the pinned image of that key instead of
    replacing the one cached image, so the walk modules run unchanged against the right table.  Outside the scope
    tree_image() is what it always was.  With `reads`, the sample is loaded on prefetch_reads' worker thread while this
    thread loads the images (native parse / index import; under torch.distributed rank0_first orders them, one after the
    other, the same on every rank).  An image that fails to load is None in the list and is not pinned: tree_image() of
    that database then raises its error again, in that database's turn."""

    def __init__(self, specs, reads=None):
        self.specs = [(d, bool(u)) for d, u in specs]
        self.reads = reads
        self.images = []
        self._keys = []

    def __enter__(self):
        pre = prefetch_reads(self.reads) if self.reads else None
        try:
            for d, u in self.specs:
                try:
                    img = TreeImage(d, u)
                except Exception:           # noqa: B902 -- raised again by that database's own tree_image()
                    img = None
                self.images.append(img)
                if img is not None:
                    key = _image_key(d, u)
                    _PINNED[key] = img
                    self._keys.append(key)
        except BaseException:
            self.__exit__()
            raise
        finally:
            if pre is not None:
                pre.join()
        return self.images

    def __exit__(self, *exc):
        for key in self._keys:
            _PINNED.pop(key, None)
        self._keys = []
        self.images = []
        wait_cache_writes()          # (an image that is still being exported must not be dropped)
        return False


def tree_image(db_dir, upper_keys=True):
    key = _image_key(db_dir, upper_keys)
    img = _PINNED.get(key)
    if img is not None:
        return img
    img = _CACHE.get(key)
    if img is None:
        img = TreeImage(db_dir, upper_keys)
        if _CACHE:
            wait_cache_writes()      # (an image that is still being exported must not be dropped)
        _CACHE.clear()               # one database image at a time on the device
        _CACHE[key] = img
    return img


def clear_cache():
    wait_cache_writes()
    _CACHE.clear()
    for rs in _READS.values():
        rs.close()
    _READS.clear()
    _close_pairs()
    _close_ordered()
