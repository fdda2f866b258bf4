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
database once.
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


# --read_support (StrainScan.apply_read_support turns it on): how many reads carry k-mers of each table the run scans.  Rows are
# collected while the tables are open -- the tree's after the tree scan (TreeImage), a cluster's in cluster_counts /
# cluster_counts_many -- under the scope of the database at work (strainscan-multi: its label), and written by the command when
# it ends.  "skipped": why nothing is written (said once on stderr).
READ_SUPPORT = {"on": False, "scope": None, "rows": {}, "skipped": None}
READ_SUPPORT_FILE = "read_support.tsv"
READ_SUPPORT_BINS = 65
READ_SUPPORT_GE = (1, 2, 4, 8, 16, 32, 64)
_READ_SUPPORT_LOCK = threading.Lock()


def read_support_reset(on=False):
    READ_SUPPORT.update(on=bool(on), scope=None, rows={}, skipped=None)


def read_support_ge(hist):
    """A 65-bin histogram (hist[b]: records with exactly b hits, hist[64]: 64 and more) -> records with >= 1, 2, 4, ... 64 hits."""
    h = [int(v) for v in hist]
    assert len(h) == READ_SUPPORT_BINS
    return [sum(h[t:]) for t in READ_SUPPORT_GE]


def read_support_text(rows):
    """The text of read_support.tsv for rows of (table, kmers, reads, hits, hist)."""
    out = ["table\tkmers\treads\thits\t" + "\t".join("ge%d" % t for t in READ_SUPPORT_GE) + "\n"]
    for table, kmers, reads, hits, hist in rows:
        out.append("\t".join([table] + [str(int(v)) for v in [kmers, reads, hits] + read_support_ge(hist)]) + "\n")
    return "".join(out)


def _read_support_skip(why):
    import sys
    if READ_SUPPORT["skipped"] is None:
        READ_SUPPORT["skipped"] = why
        print("read_support: %s and was not computed" % why, file=sys.stderr)
        sys.stderr.flush()


def collect_read_support(table, kdb, paths):
    """One row of read_support.tsv: the resident reads of `paths` against `kdb` (ReadSet.support), summed over the ranks.  A no-op
    unless --read_support is on; a table that already has its row under the current scope keeps it.  Every rank calls this at the
    same point (it holds a collective)."""
    if not READ_SUPPORT["on"] or READ_SUPPORT["skipped"] is not None:
        return
    with _READ_SUPPORT_LOCK:
        rows = READ_SUPPORT["rows"].setdefault(READ_SUPPORT["scope"], {})
        if table in rows:
            return
        if kdb.k < 17:
            return _read_support_skip("needs page-index tables (17 <= k <= 31), this run's k is %d," % kdb.k)
        rs = resident_reads(paths)
        if rs is None:
            return _read_support_skip("needs the sample resident on the device (SS_READS_RESIDENT_GB)")
        hist, hits = rs.support(kdb, READ_SUPPORT_BINS)
        v = np.concatenate([hist.astype(np.int64), np.array([hits, rs.info()["n_records"]], np.int64)])
        from . import dist
        if dist.is_distributed():
            v = dist.allreduce_int64(v)
        rows[table] = (table, kdb.info()["n_distinct"], int(v[-1]), int(v[-2]), [int(x) for x in v[:-2]])


def write_read_support(out_dir, scope=None):
    """out_dir/read_support.tsv from the rows collected under `scope`; nothing without the flag, without rows, or after a skip."""
    rows = READ_SUPPORT["rows"].get(scope)
    if not READ_SUPPORT["on"] or READ_SUPPORT["skipped"] is not None or not rows:
        return None
    path = os.path.join(out_dir, READ_SUPPORT_FILE)
    with open(path, "w") as f:
        f.write(read_support_text(rows.values()))
    return path


# -x N / --extract_reads N (StrainScan.apply_extract_reads turns it on): the reads that carry at least N k-mers of a table, written
# beside the reports as `dir`/extracted/<table>_1.<ext> (and _2 with a second mate), at the points where --read_support collects
# its rows and while the table is open.  The device selects the records (ReadSet.select); they are found in the input files again
# by the digest of their sequence, not by position -- a resident set keeps no map back to file order.  "done": the tables written
# under each scope (strainscan-multi: a database's label, with `dir` = its report directory); "skipped": why nothing is written.
# "files": what this run has written so far (a skip takes them away again: after a skip the run leaves no extracted/ of its own).
# A BAM sample (every input a BAM) takes another way: ss_bam_extract per input file and table, from the file and the open table alone --
# extracted/<table>_<i>.bam holds the input's header and the kept records of the selected templates (_write_selected_bam).
EXTRACT_READS = {"n": 0, "scope": None, "dir": None, "done": {}, "skipped": None, "files": []}
EXTRACT_READS_DIR = "extracted"
_EXTRACT_READS_LOCK = threading.Lock()


def extract_reads_reset(n=0, out_dir=None):
    EXTRACT_READS.update(n=int(n or 0), scope=None, dir=out_dir, done={}, skipped=None, files=[])


def _extract_reads_skip(why):
    import sys
    from . import dist
    if EXTRACT_READS["skipped"] is None:
        EXTRACT_READS["skipped"] = why
        for f in EXTRACT_READS["files"]:
            try:
                os.remove(f)
                os.rmdir(os.path.dirname(f))      # (once it is empty)
            except OSError:
                pass
        EXTRACT_READS["files"] = []
        if dist.rank_world()[0] == 0:
            print("extract_reads: %s and nothing was extracted" % why, file=sys.stderr)
            sys.stderr.flush()


def fastx_record_type(path):
    """'fasta' or 'fastq': the record type of a FASTA/FASTQ file, plain or gzip, by its first record's marker."""
    import gzip
    with open(path, "rb") as f:
        head = f.read(2)
    with (gzip.open(path, "rb") if head == b"\x1f\x8b" else open(path, "rb")) as f:
        for line in f:
            if line.strip():
                return "fasta" if line.startswith(b">") else "fastq"
    return "fastq"


def collect_extract_reads(table, kdb, paths):
    """extracted/<table>_1.<ext> (and _2): every read of `paths` with at least N k-mer hits against `kdb`, a pair when either
    mate has them.  A no-op unless -x is on; a table that was written under the current scope is not written again."""
    n = EXTRACT_READS["n"]
    if not n or EXTRACT_READS["skipped"] is not None:
        return
    from . import dist
    with _EXTRACT_READS_LOCK:
        done = EXTRACT_READS["done"].setdefault(EXTRACT_READS["scope"], set())
        if table in done:
            return
        if dist.is_distributed():
            return _extract_reads_skip("runs on one rank only (this run has several)")
        if kdb.k < 17:
            return _extract_reads_skip("needs page-index tables (17 <= k <= 31), this run's k is %d," % kdb.k)
        ps = [p for p in paths if p]
        bam = _extract_inputs_bam(ps)
        if bam is None:
            return
        if bam:
            return _write_selected_bam(table, kdb, None, 0, 0, ps, n, done)
        rs = resident_reads(paths)
        if rs is None:
            return _extract_reads_skip("needs the sample resident on the device (SS_READS_RESIDENT_GB)")
        _write_selected(table, lambda: rs.select(kdb, n), ps, n, done)


def _extract_inputs_bam(ps):
    """True: every input is a BAM (-x writes BAM subsets, from the files and the open table alone); False: none is; None: a mix,
    refused (_EXTRACT_READS_LOCK held)."""
    bam = [_lib.input_kind(p) == "bam" for p in ps]
    if any(bam) and not all(bam):
        _extract_reads_skip("takes BAM inputs or FASTA/FASTQ inputs, not both (this run mixes them)")
        return None
    return bool(bam) and all(bam)


def _write_selected_bam(table, kdb, labels, n_labels, label, ps, n, done):
    """extracted/<table>_<i>.bam for each BAM input i: its header and the kept records of the templates with a record of at least
    n hits against kdb (of `label` when labels are given), selected and copied on the device (_lib.bam_extract;
    _EXTRACT_READS_LOCK held)."""
    import sys
    out_dir = os.path.join(EXTRACT_READS["dir"] or ".", EXTRACT_READS_DIR)
    os.makedirs(out_dir, exist_ok=True)
    for i, p in enumerate(ps):
        out = os.path.join(out_dir, "%s_%d.bam" % (table, i + 1))
        c = _lib.bam_extract(p, kdb, n, out, labels, n_labels, label)
        EXTRACT_READS["files"].append(out)
        print("extract_reads: %s\tN=%d\tfile %d\tkept %d\tselected on the device %d\twritten %d" %
              (table, n, i + 1, c["kept"], c["selected"], c["written"]), file=sys.stderr)
    done.add(table)
    sys.stderr.flush()


def _write_selected(table, select, ps, n, done):
    """select() -> the ReadSet of the selected records; read back, digested, found in the files `ps` again and written as
    extracted/<table>_<mate>.<ext> (_EXTRACT_READS_LOCK held)."""
    import sys
    try:
        sub = select()
    except _lib.SSError as e:
        if e.code != _lib.SS_ERANGE:
            raise
        return _extract_reads_skip("cannot name the reads of a sample with a record longer than a block (it was cut)")
    try:
        selected = sub.info()["n_records"]
        flat = sub.read_back()
    finally:
        sub.close()
    keys = _lib.flat_record_keys(flat)
    del flat
    out_dir = os.path.join(EXTRACT_READS["dir"] or ".", EXTRACT_READS_DIR)
    os.makedirs(out_dir, exist_ok=True)
    outs = [os.path.join(out_dir, "%s_%d.%s" % (table, i + 1, fastx_record_type(p))) for i, p in enumerate(ps)]
    c = _lib.extract_write(ps, keys, outs)
    done.add(table)
    EXTRACT_READS["files"].extend(outs)
    print("extract_reads: %s\tN=%d\tselected on the device %d\twritten %d" % (table, n, selected, c["written"]), file=sys.stderr)
    sys.stderr.flush()


# --by_strain (StrainScan.apply_by_strain turns it on; it needs --read_support and/or -x): a cluster table holds the k-mers of ALL
# strains of its cluster, so its row of read_support.tsv and its extracted/C<id>_* are the cluster's reads.  After a cluster's
# StrainVote.report has been written, collect_by_strain labels the table's rows by the called strain that alone has them
# (strain_row_labels) and asks the device the same two questions per label (ReadSet.support_labeled / select_labeled): rows of
# strain_support.tsv, and extracted/C<id>.<n>_1.<ext>.  Rows are kept per scope and cluster (READ_SUPPORT's scope: strainscan-multi
# sets one per database) and written in the order the clusters were scanned.
BY_STRAIN = {"on": False, "rows": {}}
STRAIN_SUPPORT_FILE = "strain_support.tsv"
_BY_STRAIN_LOCK = threading.Lock()
EXTRA_REGION_MARK = " (With_ExtraRegion_covered)"      # what -e 1 appends to a strain's name in StrainVote.report


def by_strain_reset(on=False):
    BY_STRAIN.update(on=bool(on), rows={})


def strain_support_text(rows):
    """The text of strain_support.tsv for rows of (table, strain, kmers, reads, hits, hist)."""
    out = ["table\tstrain\tkmers\treads\thits\t" + "\t".join("ge%d" % t for t in READ_SUPPORT_GE) + "\n"]
    for table, strain, kmers, reads, hits, hist in rows:
        out.append("\t".join([table, strain] + [str(int(v)) for v in [kmers, reads, hits] + read_support_ge(hist)]) + "\n")
    return "".join(out)


def called_strains(report_path):
    """[(n, name)] of a StrainVote.report: its rows in order, n = column 1, name = column 2 without -e's mark."""
    out = []
    with open(report_path) as f:
        f.readline()
        for line in f:
            ele = line.rstrip("\n").split("\t")
            if len(ele) < 2 or not ele[0].strip():
                break
            name = ele[1][:-len(EXTRA_REGION_MARK)] if ele[1].endswith(EXTRA_REGION_MARK) else ele[1]
            out.append((int(ele[0]), name))
    return out


def strain_row_labels(indptr, indices, data, n_rows, called_cols):
    """np.uint8[n_rows] from a cluster's CSR matrix (row = k-mer, column = strain) and the called columns c_1 .. c_L: row r has
    label j when it is non-zero in column c_j and in no other called column; every other row -- shared between called strains, or
    in none of them -- has label 0.  Uncalled columns are not looked at."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices)
    n_mat = indptr.size - 1
    n_cols = int(indices.max()) + 1 if indices.size else 0
    col_label = np.zeros(max(n_cols, max(list(called_cols) + [0]) + 1), np.uint8)
    for j, c in enumerate(called_cols, 1):
        col_label[c] = j
    lab = col_label[indices]                                         # the called columns only ...
    if data is not None and not np.asarray(data).all():
        lab = np.where(np.asarray(data) != 0, lab, 0).astype(np.uint8)
    at = np.flatnonzero(lab)                                         # (a few of a cluster's many columns: short from here on)
    rows = np.searchsorted(indptr, at, side="right") - 1
    called = np.bincount(rows, minlength=n_mat)                      # ... a row sum over them ...
    which = np.bincount(rows, weights=lab[at], minlength=n_mat).astype(np.int64)      # ... and, where it is 1, the arg-max
    out = np.zeros(n_rows, np.uint8)
    m = min(n_rows, n_mat)
    out[:m] = np.where(called == 1, which, 0)[:m]
    return out


def cluster_csr_arrays(path):
    """(indptr, indices, data) of a cluster's all_strains_re.npz.  Members that the archive stores without compression are
    mapped, not read: np.load copies and checksums them (~7 ms per million non-zeros), and the solver has read and checked this
    same file in this run already.  Anything else goes the solver's way (_load_npz_csr)."""
    import zipfile
    from .identify_strains_L2_Enet_Pscan_new_sp import _load_npz_csr, _npy_header, _npz_directory
    try:
        d = _npz_directory(path)
        out = []
        with open(path, "rb") as f:
            for name in ("indptr", "indices", "data"):
                off, _, _, usize, method = d[name + ".npy"]
                if method != zipfile.ZIP_STORED:
                    raise ValueError(name)
                f.seek(off)
                dtype, shape, _, hlen = _npy_header(f.read(min(usize, 4096)))
                if len(shape) != 1 or dtype.hasobject or hlen + dtype.itemsize * shape[0] != usize:
                    raise ValueError(name)
                out.append(np.memmap(path, dtype=dtype, mode="r", offset=off + hlen, shape=shape) if shape[0] else np.zeros(0, dtype))
        with np.load(path, allow_pickle=False) as z:
            fmt = z["format"].item()
        if (fmt.decode() if isinstance(fmt, bytes) else fmt) != "csr" or out[0].size < 1 or out[1].size != out[2].size:
            raise ValueError("format")
        return tuple(out)
    except (OSError, KeyError, ValueError, zipfile.BadZipFile):
        m = _load_npz_csr(path)
        return m.indptr, m.indices, m.data


def collect_by_strain(cls, cls_db_dir, report_path, ksize, paths):
    """After cluster `cls` ('C<id>') has written report_path: its called strains' rows of strain_support.tsv (--read_support)
    and their extracted/<cls>.<n>_* files (-x).  A no-op unless --by_strain is on.  Every rank calls this at the same point (it
    holds collectives)."""
    if not BY_STRAIN["on"] or not os.path.exists(report_path):
        return
    support = READ_SUPPORT["on"] and READ_SUPPORT["skipped"] is None
    extract = bool(EXTRACT_READS["n"]) and EXTRACT_READS["skipped"] is None
    if not (support or extract):
        return
    from . import dist
    from .tree import load_plain_pkl
    with _BY_STRAIN_LOCK:
        scope = READ_SUPPORT["scope"]
        rows = BY_STRAIN["rows"].setdefault(scope, {})
        if cls in rows:
            return
        called = called_strains(report_path)
        if not called:
            return
        sid = load_plain_pkl(os.path.join(cls_db_dir, "id2strain_re.pkl"))
        col_of = {name: c for c, name in (sid.items() if isinstance(sid, dict) else enumerate(sid))}
        indptr, indices, data = cluster_csr_arrays(os.path.join(cls_db_dir, "all_strains_re.npz"))
        ps = [p for p in paths if p]
        bam = extract and bool(ps) and all(_lib.input_kind(p) == "bam" for p in ps)      # (-x on a BAM needs no resident set)
        rs = resident_reads(paths)
        if rs is None:                                               # (said by --read_support / -x already)
            support = False
            if not bam:
                return
        kdb = fasta_index(os.path.join(cls_db_dir, "all_kmer.fasta"), int(ksize), 2)
        try:
            if kdb.k < 17:
                return
            labels = strain_row_labels(indptr, indices, data, kdb.n_rows, [col_of[name] for _, name in called])
            n_reads = rs.info()["n_records"] if support else 0
            out = []
            for j0 in range(0, len(called), _lib.LABELS_MAX):        # (more called strains than a call takes: several calls)
                part = called[j0:j0 + _lib.LABELS_MAX]
                lab = np.where((labels > j0) & (labels <= j0 + len(part)), labels - j0, 0).astype(np.uint8)
                if support:
                    hist, hits, kmers = rs.support_labeled(kdb, lab, len(part), READ_SUPPORT_BINS)
                    v = np.concatenate([hist.astype(np.int64).ravel(), hits.astype(np.int64), [n_reads]])
                    if dist.is_distributed():
                        v = dist.allreduce_int64(v)
                    hist = v[:hist.size].reshape(hist.shape)
                    for i, (n, name) in enumerate(part):
                        out.append(("%s.%d" % (cls, n), name, int(kmers[i]), int(v[-1]), int(v[hist.size + i]), [int(x) for x in hist[i]]))
                if extract:
                    with _EXTRACT_READS_LOCK:
                        done = EXTRACT_READS["done"].setdefault(EXTRACT_READS["scope"], set())
                        for i, (n, name) in enumerate(part):
                            if EXTRACT_READS["skipped"] is not None or "%s.%d" % (cls, n) in done:
                                continue
                            if bam:
                                _write_selected_bam("%s.%d" % (cls, n), kdb, lab, len(part), i + 1, ps, EXTRACT_READS["n"], done)
                            else:
                                _write_selected("%s.%d" % (cls, n), lambda i=i: rs.select_labeled(kdb, lab, len(part), i + 1, EXTRACT_READS["n"]),
                                                    ps, EXTRACT_READS["n"], done)
            rows[cls] = out
        finally:
            kdb.close()


def write_strain_support(out_dir, scope=None):
    """out_dir/strain_support.tsv from the rows collected under `scope`, clusters in the order of read_support.tsv's rows;
    nothing without --by_strain and --read_support, without rows, or after a skip."""
    rows = BY_STRAIN["rows"].get(scope)
    if not BY_STRAIN["on"] or not READ_SUPPORT["on"] or READ_SUPPORT["skipped"] is not None or not rows or not any(rows.values()):
        return None
    order = [t for t in READ_SUPPORT["rows"].get(scope, {}) if t in rows]
    order += sorted(t for t in rows if t not in order)
    path = os.path.join(out_dir, STRAIN_SUPPORT_FILE)
    with open(path, "w") as f:
        f.write(strain_support_text([r for t in order for r in sorted(rows[t], key=lambda r: int(r[0].rsplit(".", 1)[1]))]))
    return path


# --bootstrap B (StrainScan.apply_bootstrap turns it on): how firm are a multi-strain cluster's numbers?  After the cluster has
# written its StrainVote.report, collect_bootstrap resamples the reads that carry k-mers of its table B times on the device
# (ReadSet.resample: a Poisson bootstrap over reads, replicate b of seed S), re-counts the table from each resampled set and solves
# each replicate again with the main solve's strains and alpha held fixed (replicate_coefs).
# "solve": the main solve's state, left by detect_core per solving thread while the flag is on; "rows": per scope (READ_SUPPORT's)
# and cluster, the report's rows and the [B, p] matrix of replicate coefficients; "order": the clusters as they were scanned;
# "skipped": why nothing is written (said once on stderr).  strain_bootstrap.tsv is a pure function of the rows (bootstrap_text).
BOOTSTRAP = {"b": 0, "seed": 1, "solve": {}, "rows": {}, "order": {}, "skipped": None}
BOOTSTRAP_FILE = "strain_bootstrap.tsv"
BOOTSTRAP_QUANTILES = (0.025, 0.975)
_BOOTSTRAP_LOCK = threading.Lock()


def bootstrap_reset(b=0, seed=1):
    BOOTSTRAP.update(b=int(b or 0), seed=int(seed), solve={}, rows={}, order={}, skipped=None)


def bootstrap_note_solve(**state):
    """detect_core and enet_cv_fit leave the main solve's state here (columns, strains, alpha, the row filter's bounds, the
    identified clusters), under the solving thread; a no-op unless --bootstrap is on."""
    if BOOTSTRAP["b"]:
        if state.pop("begin", False):
            BOOTSTRAP["solve"][threading.get_ident()] = {}
        BOOTSTRAP["solve"].setdefault(threading.get_ident(), {}).update(state)


def bootstrap_scanned(table):
    """A cluster table has been scanned: strain_bootstrap.tsv lists the clusters in this order."""
    if BOOTSTRAP["b"]:
        order = BOOTSTRAP["order"].setdefault(READ_SUPPORT["scope"], [])
        if table not in order:
            order.append(table)


def bootstrap_replicates(scope=None):
    """{cluster: (strain names, np.float64[B, p])}: the replicate coefficients collected under `scope`, a column per selected
    strain in pre-scan order (tests; strain_bootstrap.tsv is bootstrap_text of these and the reports' rows)."""
    return {cls: (list(r["strains"]), r["coefs"].copy()) for cls, r in BOOTSTRAP["rows"].get(scope, {}).items()}


def bootstrap_index(q, b):
    """Which of b ascending values stands for quantile q: floor(q * (b - 1) + 0.5)."""
    return int(np.floor(q * (b - 1) + 0.5))


def bootstrap_summary(coefs):
    """np.float64[B, p] replicate coefficients -> per column (depth_lo, depth_hi, frac_lo, frac_hi, present): the values at
    bootstrap_index(0.025 / 0.975, B) of the ascending coefficients and of the ascending fractions coef / sum over the
    replicate's columns (0 where that sum is 0), and the replicates with coef > 0."""
    coefs = np.asarray(coefs, np.float64)
    b = coefs.shape[0]
    tot = coefs.sum(axis=1, keepdims=True)
    frac = np.divide(coefs, tot, out=np.zeros_like(coefs), where=tot != 0)
    lo, hi = (bootstrap_index(q, b) for q in BOOTSTRAP_QUANTILES)
    cs, fs = np.sort(coefs, axis=0), np.sort(frac, axis=0)
    return [(float(cs[lo, j]), float(cs[hi, j]), float(fs[lo, j]), float(fs[hi, j]), int((coefs[:, j] > 0).sum()))
            for j in range(coefs.shape[1])]


def bootstrap_text(rows):
    """The text of strain_bootstrap.tsv for rows of (table, strain, depth text, frac text, column, coefs [B, p]): depth and frac
    are copied from the strain's report row, `column` is the strain's column of the replicate matrix."""
    out = ["table\tstrain\treplicates\tdepth\tdepth_lo\tdepth_hi\tfrac\tfrac_lo\tfrac_hi\tpresent\n"]
    summaries = {}
    for table, strain, depth, frac, col, coefs in rows:
        if id(coefs) not in summaries:
            summaries[id(coefs)] = bootstrap_summary(coefs)
        d_lo, d_hi, f_lo, f_hi, present = summaries[id(coefs)][col]
        out.append("\t".join([table, strain, str(int(np.asarray(coefs).shape[0])), depth, str(d_lo), str(d_hi), frac, str(f_lo), str(f_hi),
                              str(present)]) + "\n")
    return "".join(out)


def _bootstrap_skip(why):
    import sys
    from . import dist
    if BOOTSTRAP["skipped"] is None:
        BOOTSTRAP["skipped"] = why
        if dist.rank_world()[0] == 0:
            print("bootstrap: %s and no intervals were computed" % why, file=sys.stderr)
            sys.stderr.flush()


def report_rows(report_path):
    """[(n, name, frac text, depth text)] of a StrainVote.report: columns 1, 2 (without -e's mark), 4 and 5 of its rows."""
    out = []
    with open(report_path) as f:
        f.readline()
        for line in f:
            ele = line.rstrip("\n").split("\t")
            if len(ele) < 5 or not ele[0].strip():
                break
            name = ele[1][:-len(EXTRA_REGION_MARK)] if ele[1].endswith(EXTRA_REGION_MARK) else ele[1]
            out.append((int(ele[0]), name, ele[3], ele[4]))
    return out


def replicate_coefs(img, om, solve, counts):
    """One bootstrap replicate of a cluster (--bootstrap, db.collect_bootstrap): the coefficients of the strains the main solve
    selected, from the k-mer counts of a resampled read set.  Held fixed from the main solve (`solve`, what detect_core and
    enet_cv_fit left with bootstrap_note_solve): the selected columns in pre-scan order, the alpha lasso_mpm picked, npp25,
    npp75, npp_out and the identified clusters.  Recomputed: y = remove_1(counts), the device vectors and with them the kept rows.
    p >= 2: the pattern statistics of all kept rows -> Gram -> one elastic-net fit at that alpha, with the arguments of
    enet_cv_fit's refit; no kept row: zeros.  p = 1 (the main solve never reached the elastic net): pre_scan's get_avg_depth
    of the one column, 0.0 where the column has no count."""
    from . import l2 as L2
    from .Vote_Strain_L2_Lasso_new_sp import remove_1
    from .identify_strains_L2_Enet_Pscan_new_sp import MAX_NITER
    cols = list(solve["columns"])
    p = len(cols)
    if img.om_cols is None:
        img.set_overlap(om)
    vec = img.prepare(remove_1(counts), solve["new_als"], solve["npp25"], solve["npp75"], solve["npp_out"])
    try:
        if p == 1:
            qd = img.quantile_sums(vec.yu if vec.use_u else vec.y, cols, 25, 75)
            if qd["n_nz"][0] == 0 or qd["cnt_in"][0] == 0:
                return np.zeros(1)
            return np.array([float(qd["sum_in"][0]) / float(qd["cnt_in"][0])])
        n = vec.n_keep
        if n == 0:
            return np.zeros(p)
        fold = img.fold_words(vec.keep, np.zeros(n, np.uint32), n)
        try:
            stats = img.pattern_stats(cols, vec.ykeep, fold, 0)
        finally:
            fold.close()
        Qt, qt, yyt, nt = L2.gram_from_stats(stats[0], p)
        fit = L2.enet_path_gram(Qt[None], qt[None], [yyt], [nt], [solve["alpha"]], l1_ratio=0.5, max_iter=MAX_NITER, tol=1e-4,
                                positive=True)
        return fit["coefs"][0, 0].copy()
    finally:
        vec.close()


def collect_bootstrap(cls, cls_db_dir, report_path, ksize, paths):
    """After cluster `cls` ('C<id>') has written report_path: B replicate solves of it.  A no-op unless --bootstrap is on.  Every
    rank calls this at the same point (it holds collectives): each resamples its own shard of the reads -- the weights depend on
    a read's bytes alone, so the summed counts are those of one process."""
    solve = BOOTSTRAP["solve"].pop(threading.get_ident(), None)
    b = BOOTSTRAP["b"]
    if not b or BOOTSTRAP["skipped"] is not None or solve is None or not solve.get("columns") or not os.path.exists(report_path):
        return
    from . import dist
    from . import identify_strains_L2_Enet_Pscan_new_sp as enet
    with _BOOTSTRAP_LOCK:
        if BOOTSTRAP["skipped"] is not None:
            return
        rows = BOOTSTRAP["rows"].setdefault(READ_SUPPORT["scope"], {})
        if cls in rows:
            return
        called = report_rows(report_path)
        if not called:
            return
        if int(ksize) < 17:
            return _bootstrap_skip("needs page-index tables (17 <= k <= 31), this run's k is %d," % int(ksize))
        rs = resident_reads(paths)
        if rs is None:
            return _bootstrap_skip("needs the sample resident on the device (SS_READS_RESIDENT_GB)")
        kdb = fasta_index(os.path.join(cls_db_dir, "all_kmer.fasta"), int(ksize), 2)
        kdb.expect_hits()
        sub = img = None
        try:
            try:
                sub = rs.select(kdb, 1)          # reads without a hit add nothing to any count: only these are resampled
            except _lib.SSError as e:
                if e.code != _lib.SS_ERANGE:
                    raise
                return _bootstrap_skip("cannot resample the reads of a sample with a record longer than a block (it was cut)")
            img, om = enet.open_cluster_image(cls_db_dir + "/all_strains_re.npz", cls_db_dir + "/overlap_matrix.npz")
            coefs = np.zeros((b, len(solve["columns"])), np.float64)
            for rep in range(b):
                rb = sub.resample(BOOTSTRAP["seed"], rep)
                try:
                    kdb.reset()
                    rb.order().scan_into(kdb)    # binned first: 2.2 + 6.2 ms beside 16.6 ms for 20 M reads (profiles/r21_bootstrap.md)
                    if dist.is_distributed():
                        dist.allreduce_table(kdb)
                    _lib.check(_lib.lib().ss_device_sync(), "ss_device_sync")
                    counts = kdb.counts_rows()
                finally:
                    rb.close()
                coefs[rep] = replicate_coefs(img, om, solve, counts)
        finally:
            if img is not None:
                img.close()
            if sub is not None:
                sub.close()
            kdb.close()
        col_of = {str(name): j for j, name in enumerate(solve["strains"])}
        rows[cls] = dict(strains=[str(s) for s in solve["strains"]], coefs=coefs,
                         called=[(n, name, depth, frac, col_of[name]) for n, name, frac, depth in called if name in col_of])


def write_bootstrap(out_dir, scope=None):
    """out_dir/strain_bootstrap.tsv from the replicates collected under `scope`, clusters in the order scanned, strains in report
    order; nothing without the flag, without a solved multi-strain cluster, or after a skip."""
    rows = BOOTSTRAP["rows"].get(scope)
    if not BOOTSTRAP["b"] or BOOTSTRAP["skipped"] is not None or not rows:
        return None
    order = [t for t in BOOTSTRAP["order"].get(scope, []) if t in rows]
    order += sorted(t for t in rows if t not in order)
    lines = [("%s.%d" % (t, n), name, depth, frac, col, rows[t]["coefs"]) for t in order for n, name, depth, frac, col in rows[t]["called"]]
    if not lines:
        return None
    path = os.path.join(out_dir, BOOTSTRAP_FILE)
    with open(path, "w") as f:
        f.write(bootstrap_text(lines))
    return path


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
            # (.gz under torch.distributed: all ranks take the same inflate path for a file, dist.load_agreed)
            before = _lib.mask_counters() if MASK_REPORT["on"] else None
            rs = dist.load_agreed([p for p in paths if p], lambda use: _lib.ReadSet(use, rank, world), discard=lambda r: r.close())
            _READS[key] = rs
            if before is not None:
                after, inf = _lib.mask_counters(), rs.info()
                report_mask(after["masked"] - before["masked"], after["bam_no_qual"] - before["bam_no_qual"],
                            inf["n_bases"] - inf["n_records"])
    return rs


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
