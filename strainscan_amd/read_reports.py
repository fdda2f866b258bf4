"""The opt-in reports about the sample's reads: --read_support, -x / --extract_reads, --by_strain, --bootstrap,
--bootstrap_clusters, --classify_reads, --extract_class, --tag_bam, --read_calls, --classify_strains, --extract_strains, --em_strains and --divergence; and --pairs, which makes all of them work on read pairs as fragments.

Each report has a state dict (its flag, what it has collected per scope, and "skipped": why nothing is written, said once on
stderr), a lock, a `*_reset`, its `collect_*` and its `write_*`, all no-ops while the flag is off.  The scans and the solver reach
them through tree_scanned, table_scanned and cluster_reported, the commands end with write_all and reset_all.  The scope is the database at
work: SCOPE["label"], None but inside strainscan-multi's database_scope.
"""
import contextlib
import functools
import os
import sys
import threading

import numpy as np

from . import _lib, db, dist

SCOPE = {"label": None}
EXTRA_REGION_MARK = " (With_ExtraRegion_covered)"      # what -e 1 appends to a strain's name in StrainVote.report
NEEDS_PAGE_INDEX = "needs page-index tables (17 <= k <= 31), this run's k is %d,"
NEEDS_RESIDENT = "needs the sample resident on the device (SS_READS_RESIDENT_GB)"
RECORD_WAS_CUT = "cannot %s the reads of a sample with a record longer than a block (it was cut)"


@contextlib.contextmanager
def database_scope(label, out_dir):
    """strainscan-multi, around one database's work: its rows are kept under `label`, -x writes to out_dir/extracted/,
    --tag_bam and --read_calls to out_dir."""
    before = SCOPE["label"], EXTRACT_READS["dir"], TAG_BAM["dir"], READ_CALLS["dir"]
    SCOPE["label"], EXTRACT_READS["dir"], TAG_BAM["dir"], READ_CALLS["dir"] = label, out_dir, out_dir, out_dir
    try:
        yield
    finally:
        SCOPE["label"], EXTRACT_READS["dir"], TAG_BAM["dir"], READ_CALLS["dir"] = before


def tree_scanned(img, paths):
    """The tree image `img` (db.TreeImage) holds the scan of `paths`, or counts made elsewhere (img.is_external): the tree's
    table_scanned, then --classify_reads, which needs the node lists and the tree as well as the table."""
    if not _pairs_gate(paths):
        return
    if not img.is_external:
        table_scanned("tree", img.kdb, paths)
    collect_read_classes(img, paths)


def table_scanned(table, kdb, paths):
    """`kdb` is open and holds the scan of `paths`: --read_support's row, -x's files and --bootstrap's order of the clusters.
    ("tree" enters that order too; write_bootstrap keeps only tables with rows, and the tree never has any.)"""
    if not _pairs_gate(paths):
        return
    collect_read_support(table, kdb, paths)
    collect_extract_reads(table, kdb, paths)
    bootstrap_scanned(table)
    strain_classes_scanned(table)
    divergence_scanned(table)


def cluster_reported(cls, cls_db_dir, report_path, ksize, paths):
    """Cluster `cls` ('C<id>') has written report_path: --by_strain, --classify_strains, --divergence, then --bootstrap."""
    if not _pairs_gate(paths):
        return
    collect_by_strain(cls, cls_db_dir, report_path, ksize, paths)
    collect_strain_classes(cls, cls_db_dir, report_path, ksize, paths)
    collect_divergence(cls, cls_db_dir, report_path, ksize, paths)
    collect_bootstrap(cls, cls_db_dir, report_path, ksize, paths)


def write_all(out_dir, scope=None):
    write_read_support(out_dir, scope)
    write_strain_support(out_dir, scope)
    write_bootstrap(out_dir, scope)
    write_cluster_bootstrap(out_dir, scope)
    write_read_classes(out_dir, scope)
    write_strain_classes(out_dir, scope)
    write_em_strains(out_dir, scope)
    write_divergence(out_dir, scope)


def reset_all():
    read_support_reset()
    extract_reads_reset()
    by_strain_reset()
    bootstrap_reset()
    cluster_bootstrap_reset()
    classify_reads_reset()
    extract_class_reset()
    tag_bam_reset()
    read_calls_reset()
    classify_strains_reset()
    extract_strains_reset()
    em_strains_reset()
    divergence_reset()
    pairs_reset()


def _skip(state, name, closing, rank0_only, why):
    """The report `name` writes nothing from here on: remember why in its state and say it once on stderr, every rank or rank 0."""
    if state["skipped"] is None:
        state["skipped"] = why
        if not rank0_only or dist.rank_world()[0] == 0:
            print("%s: %s %s" % (name, why, closing), file=sys.stderr)
            sys.stderr.flush()


def _select_or_skip(select, skip, verb):
    """select() -> the ReadSet of the selected records, or None after skip(): a record of the sample was cut (SS_ERANGE)."""
    try:
        return select()
    except _lib.SSError as e:
        if e.code != _lib.SS_ERANGE:
            raise
        return skip(RECORD_WAS_CUT % verb)


# --pairs (StrainScan.apply_pairs turns it on; it needs -j or a BAM under -i, and one of the reports below): the reports work on FRAGMENTS.  The
# device calls decide per record from the record's bytes alone, so they are handed a second resident set whose records are the
# pairs -- record i of the first file, an N, record i of the second; for one BAM under -i, the mates its names and flags link
# (db.resident_pairs) -- and run unchanged; -x on a BAM selects by fragment (_write_selected_bam); no k-mer spans the
# N, so a fragment's hits are its mates' added up.  The scans of the identification keep the plain set.  _report_reads is where
# every collect_* gets its set; _pairs_gate stands in front of the three hooks: where the pairs cannot be joined it says one line
# and every per-read report of the run writes nothing (no silent fall-back to mates).
PAIRS = {"on": False, "skipped": None}
_PAIRS_LOCK = threading.Lock()


def pairs_reset(on=False):
    PAIRS.update(on=bool(on), skipped=None)


def _pairs_gate(paths):
    """True: the per-read reports may run on `paths` -- --pairs is off, or the joined set is there (built here the first time)."""
    if not PAIRS["on"]:
        return True
    with _PAIRS_LOCK:
        if PAIRS["skipped"] is None:
            js, why = db.resident_pairs(paths)
            if js is not None:
                return True
            PAIRS["skipped"] = why
            for state in (READ_SUPPORT, EXTRACT_READS, BOOTSTRAP, CLASSIFY_READS, EXTRACT_CLASS, CLASSIFY_STRAINS, EXTRACT_STRAINS, EM_STRAINS, DIVERGENCE):
                if state["skipped"] is None:
                    state["skipped"] = "--pairs " + why
            if dist.rank_world()[0] == 0:
                print("pairs: %s and no per-read report was written" % why, file=sys.stderr)
                sys.stderr.flush()
    return False


def _report_reads(paths):
    """The resident set the per-read reports work on: the joined pairs with --pairs, else the sample's reads; None when it is
    not there."""
    if PAIRS["on"]:
        return db.resident_pairs(paths)[0] if PAIRS["skipped"] is None else None
    return db.resident_reads(paths)


def _extract_write(ps, keys, outs):
    """-x's writer: with --pairs the keys name pairs and both records of a named pair are written"""
    if PAIRS["on"]:
        return _lib.extract_write_pairs(ps, keys, outs)
    return _lib.extract_write(ps, keys, outs)


def _write(out_dir, name, text):
    path = os.path.join(out_dir, name)
    with open(path, "w") as f:
        f.write(text)
    return path


def _in_order(first, rows):      # the tables of `rows`: those that `first` names, in its order, then the others sorted
    order = [t for t in first if t in rows]
    return order + sorted(t for t in rows if t not in order)


# --read_support (StrainScan.apply_read_support turns it on): how many reads carry k-mers of each table the run scans.  Rows are
# collected while the tables are open -- the tree's after the tree scan (TreeImage), a cluster's in cluster_counts /
# cluster_counts_many -- and written by the command when it ends.
READ_SUPPORT = {"on": False, "rows": {}, "skipped": None}
READ_SUPPORT_FILE = "read_support.tsv"
READ_SUPPORT_BINS = 65
READ_SUPPORT_GE = (1, 2, 4, 8, 16, 32, 64)
_READ_SUPPORT_LOCK = threading.Lock()
_read_support_skip = functools.partial(_skip, READ_SUPPORT, "read_support", "and was not computed", False)


def read_support_reset(on=False):
    READ_SUPPORT.update(on=bool(on), rows={}, skipped=None)


def read_support_ge(hist):
    """A 65-bin histogram (hist[b]: records with exactly b hits, hist[64]: 64 and more) -> records with >= 1, 2, 4, ... 64 hits."""
    h = [int(v) for v in hist]
    assert len(h) == READ_SUPPORT_BINS
    return [sum(h[t:]) for t in READ_SUPPORT_GE]


def _support_text(names, rows):
    """Rows of (one text per name ..., kmers, reads, hits, hist) under the header names ..., kmers, reads, hits, ge1 .. ge64."""
    out = ["\t".join(names + ["kmers", "reads", "hits"] + ["ge%d" % t for t in READ_SUPPORT_GE]) + "\n"]
    for *texts, kmers, reads, hits, hist in rows:
        out.append("\t".join(texts + [str(int(v)) for v in [kmers, reads, hits] + read_support_ge(hist)]) + "\n")
    return "".join(out)


def read_support_text(rows):
    """The text of read_support.tsv for rows of (table, kmers, reads, hits, hist)."""
    return _support_text(["table"], rows)


def collect_read_support(table, kdb, paths):
    """One row of read_support.tsv: the resident reads of `paths` against `kdb` (ReadSet.support), summed over the ranks.  A no-op
    unless --read_support is on; a table that already has its row under the current scope keeps it.  Every rank calls this at the
    same point (it holds a collective)."""
    if not READ_SUPPORT["on"] or READ_SUPPORT["skipped"] is not None:
        return
    with _READ_SUPPORT_LOCK:
        rows = READ_SUPPORT["rows"].setdefault(SCOPE["label"], {})
        if table in rows:
            return
        if kdb.k < 17:
            return _read_support_skip(NEEDS_PAGE_INDEX % kdb.k)
        rs = _report_reads(paths)
        if rs is None:
            return _read_support_skip(NEEDS_RESIDENT)
        hist, hits = rs.support(kdb, READ_SUPPORT_BINS)
        v = np.concatenate([hist.astype(np.int64), np.array([hits, rs.info()["n_records"]], np.int64)])
        if dist.is_distributed():
            v = dist.allreduce_int64(v)
        rows[table] = (table, kdb.info()["n_distinct"], int(v[-1]), int(v[-2]), [int(x) for x in v[:-2]])


def write_read_support(out_dir, scope=None):
    """out_dir/read_support.tsv from the rows collected under `scope`; nothing without the flag, without rows, or after a skip."""
    rows = READ_SUPPORT["rows"].get(scope)
    if not READ_SUPPORT["on"] or READ_SUPPORT["skipped"] is not None or not rows:
        return None
    return _write(out_dir, READ_SUPPORT_FILE, read_support_text(rows.values()))


# -x N / --extract_reads N (StrainScan.apply_extract_reads turns it on): the reads that carry at least N k-mers of a table, written
# beside the reports as `dir`/extracted/<table>_1.<ext> (and _2 with a second mate), at the points where --read_support collects
# its rows and while the table is open.  The device selects the records (ReadSet.select); they are found in the input files again
# by the digest of their sequence, not by position -- a resident set keeps no map back to file order (_write_selected).  A sample
# whose every input is a BAM gets BAM subsets instead (_write_selected_bam).  "done": the tables written under each scope;
# "files": what this run has written so far (a skip takes them away again: after a skip the run leaves no extracted/ of its own).
EXTRACT_READS = {"n": 0, "dir": None, "done": {}, "skipped": None, "files": []}
EXTRACT_READS_DIR = "extracted"
_EXTRACT_READS_LOCK = threading.Lock()


def extract_reads_reset(n=0, out_dir=None):
    EXTRACT_READS.update(n=int(n or 0), dir=out_dir, done={}, skipped=None, files=[])


def _extract_reads_skip(why):
    for f in EXTRACT_READS["files"]:        # (none are left after the first skip: nothing is written after one)
        with contextlib.suppress(OSError):
            os.remove(f)
            os.rmdir(os.path.dirname(f))      # (once it is empty)
    EXTRACT_READS["files"] = []
    _skip(EXTRACT_READS, "extract_reads", "and nothing was extracted", True, why)


def fastx_record_type(path):
    """'fasta' or 'fastq': the record type of a FASTA/FASTQ file, plain or gzip, by its first record's marker."""
    import gzip
    with open(path, "rb") as f:
        head = f.read(2)
    with (gzip.open if head == b"\x1f\x8b" else open)(path, "rb") as f:
        first = next((line for line in f if line.strip()), b"")
    return "fasta" if first.startswith(b">") else "fastq"


def collect_extract_reads(table, kdb, paths):
    """extracted/<table>_1.<ext> (and _2): every read of `paths` with at least N k-mer hits against `kdb`, a pair when either
    mate has them.  A no-op unless -x is on; a table that was written under the current scope is not written again."""
    n = EXTRACT_READS["n"]
    if not n or EXTRACT_READS["skipped"] is not None:
        return
    with _EXTRACT_READS_LOCK:
        done = EXTRACT_READS["done"].setdefault(SCOPE["label"], set())
        if table in done:
            return
        if dist.is_distributed():
            return _extract_reads_skip("runs on one rank only (this run has several)")
        if kdb.k < 17:
            return _extract_reads_skip(NEEDS_PAGE_INDEX % kdb.k)
        ps = [p for p in paths if p]
        bam = {_lib.input_kind(p) == "bam" for p in ps}
        if len(bam) == 2:
            return _extract_reads_skip("takes BAM inputs or FASTA/FASTQ inputs, not both (this run mixes them)")
        if True in bam:               # (BAM subsets, from the files and the open table alone: no resident set)
            return _write_selected_bam(table, kdb, None, 0, 0, ps, n, done)
        rs = _report_reads(paths)
        if rs is None:
            return _extract_reads_skip(NEEDS_RESIDENT)
        _write_selected(table, lambda: rs.select(kdb, n), ps, n, done)


def _write_selected_bam(table, kdb, labels, n_labels, label, ps, n, done):
    """extracted/<table>_<i>.bam for each BAM input i: its header and the kept records of the templates with a record of at least n
    hits against kdb (of `label` when labels are given), selected and copied on the device (bam_extract; _EXTRACT_READS_LOCK held).
    With --pairs the unit is the fragment: both records of a pair whose hits together reach n, and the line counts fragments."""
    out_dir = os.path.join(EXTRACT_READS["dir"] or ".", EXTRACT_READS_DIR)
    os.makedirs(out_dir, exist_ok=True)
    for i, p in enumerate(ps):
        out = os.path.join(out_dir, "%s_%d.bam" % (table, i + 1))
        c = _lib.bam_extract(p, kdb, n, out, labels, n_labels, label, pairs=PAIRS["on"])
        EXTRACT_READS["files"].append(out)
        print("extract_reads: %s\tN=%d\tfile %d\tkept %d\t%s on the device %d\twritten %d" %
              (table, n, i + 1, c["kept"], "fragments selected" if PAIRS["on"] else "selected", c["selected"], c["written"]), file=sys.stderr)
    done.add(table)
    sys.stderr.flush()


def _write_selected(table, select, ps, n, done):
    """select() -> the ReadSet of the selected records; read back, digested, found in the files `ps` again and written as
    extracted/<table>_<mate>.<ext> (_EXTRACT_READS_LOCK held)."""
    sub = _select_or_skip(select, _extract_reads_skip, "name")
    if sub is None:
        return
    with contextlib.closing(sub):
        selected = sub.info()["n_records"]
        flat = sub.read_back()
    keys = _lib.flat_record_keys(flat)
    del flat
    out_dir = os.path.join(EXTRACT_READS["dir"] or ".", EXTRACT_READS_DIR)
    os.makedirs(out_dir, exist_ok=True)
    outs = [os.path.join(out_dir, "%s_%d.%s" % (table, i + 1, fastx_record_type(p))) for i, p in enumerate(ps)]
    c = _extract_write(ps, keys, outs)
    done.add(table)
    EXTRACT_READS["files"].extend(outs)
    print("extract_reads: %s\tN=%d\tselected on the device %d\twritten %d" % (table, n, selected, c["written"]), file=sys.stderr)
    sys.stderr.flush()


# --by_strain (StrainScan.apply_by_strain turns it on; it needs --read_support and/or -x): a cluster table holds the k-mers of ALL
# strains of its cluster, so its row of read_support.tsv and its extracted/C<id>_* are the cluster's reads.  After a cluster's
# StrainVote.report has been written, collect_by_strain labels the table's rows by the called strain that alone has them
# (strain_row_labels) and asks the device the same two questions per label (ReadSet.support_labeled / select_labeled): rows of
# strain_support.tsv, and extracted/C<id>.<n>_1.<ext>.  Rows are kept per scope and cluster, written in the order of the scans.
BY_STRAIN = {"on": False, "rows": {}}
STRAIN_SUPPORT_FILE = "strain_support.tsv"
_BY_STRAIN_LOCK = threading.Lock()


def by_strain_reset(on=False):
    BY_STRAIN.update(on=bool(on), rows={})


def strain_support_text(rows):
    """The text of strain_support.tsv for rows of (table, strain, kmers, reads, hits, hist)."""
    return _support_text(["table", "strain"], rows)


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


def called_strains(report_path):
    """[(n, name)] of a StrainVote.report: its rows in order, n = column 1, name = column 2 without -e's mark."""
    return [row[:2] for row in report_rows(report_path)]


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
    support = BY_STRAIN["on"] and READ_SUPPORT["on"] and READ_SUPPORT["skipped"] is None
    extract = BY_STRAIN["on"] and bool(EXTRACT_READS["n"]) and EXTRACT_READS["skipped"] is None
    if not (support or extract) or not os.path.exists(report_path):
        return
    from .tree import load_plain_pkl
    with _BY_STRAIN_LOCK:
        rows = BY_STRAIN["rows"].setdefault(SCOPE["label"], {})
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
        rs = _report_reads(paths)
        if rs is None:                                               # (said by --read_support / -x already)
            support = False
            if not bam:
                return
        with contextlib.closing(db.fasta_index(os.path.join(cls_db_dir, "all_kmer.fasta"), int(ksize), 2)) as kdb:
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
                        done = EXTRACT_READS["done"].setdefault(SCOPE["label"], set())
                        for i, (n, name) in enumerate(part):
                            if EXTRACT_READS["skipped"] is not None or "%s.%d" % (cls, n) in done:
                                continue
                            if bam:
                                _write_selected_bam("%s.%d" % (cls, n), kdb, lab, len(part), i + 1, ps, EXTRACT_READS["n"], done)
                            else:
                                _write_selected("%s.%d" % (cls, n), lambda i=i: rs.select_labeled(kdb, lab, len(part), i + 1, EXTRACT_READS["n"]),
                                                ps, EXTRACT_READS["n"], done)
            rows[cls] = out


def write_strain_support(out_dir, scope=None):
    """out_dir/strain_support.tsv from the rows collected under `scope`, clusters in the order of read_support.tsv's rows;
    nothing without --by_strain and --read_support, without rows, or after a skip."""
    rows = BY_STRAIN["rows"].get(scope)
    if not BY_STRAIN["on"] or not READ_SUPPORT["on"] or READ_SUPPORT["skipped"] is not None or not rows or not any(rows.values()):
        return None
    order = _in_order(READ_SUPPORT["rows"].get(scope, {}), rows)
    return _write(out_dir, STRAIN_SUPPORT_FILE,
                  strain_support_text([r for t in order for r in sorted(rows[t], key=lambda r: int(r[0].rsplit(".", 1)[1]))]))


# --classify_strains M (StrainScan.apply_classify_strains turns it on): --by_strain sees only the reads with k-mers that ONE called
# strain has; this says, for every read, which of a cluster's called strains it is compatible with.  After a cluster's
# StrainVote.report has been written, collect_strain_classes gives every row of the cluster's table the MASK of the called strains
# that have its k-mer (strain_row_sets: bit j - 1 for the j-th row of the report) and the device votes per read: h[j] = the read's
# hits whose k-mer strain j has, the read's set = the strains with the most hits, empty below M (ReadSet.classify_strains;
# tests/strain_set_model.py restates it).  Written as strain_classes.tsv (a row per called strain) and strain_sets.tsv (a row per
# set with reads: the equivalence classes).  "rows": per scope and cluster, the called strains and the device's numbers (None: the
# cluster was passed over); "order": the tables as they were scanned.
# --extract_strains unique|compatible (apply_extract_strains; it needs --classify_strains): a second device call
# (ReadSet.select_strains) gives, per called strain, the reads whose set is that strain alone / holds that strain, written as
# extracted/strain_C<id>.<n>_<mate>.<ext> by -x's writer.  "files": what this run has written so far (a skip takes them away).
CLASSIFY_STRAINS = {"m": 0, "rows": {}, "order": {}, "skipped": None}
EXTRACT_STRAINS = {"mode": None, "skipped": None, "files": []}
EXTRACT_STRAINS_MODES = ("unique", "compatible")
STRAIN_CLASSES_FILE = "strain_classes.tsv"
STRAIN_SETS_FILE = "strain_sets.tsv"
_CLASSIFY_STRAINS_LOCK = threading.Lock()


def _classify_strains_skip(why):
    _skip(CLASSIFY_STRAINS, "classify_strains", "and no read was assigned", True, why)
    _em_strains_skip(why)      # (--em_strains starts from these sets: it writes nothing either, and says so itself)


def classify_strains_reset(m=0):
    CLASSIFY_STRAINS.update(m=int(m or 0), rows={}, order={}, skipped=None)


def extract_strains_reset(mode=None):
    EXTRACT_STRAINS.update(mode=mode or None, skipped=None, files=[])


def _extract_strains_skip(why):
    for f in EXTRACT_STRAINS["files"]:
        with contextlib.suppress(OSError):
            os.remove(f)
            os.rmdir(os.path.dirname(f))      # (once it is empty)
    EXTRACT_STRAINS["files"] = []
    _skip(EXTRACT_STRAINS, "extract_strains", "and nothing was extracted", True, why)


def strain_classes_scanned(table):
    """A table has been scanned: strain_classes.tsv and strain_sets.tsv list the clusters in this order."""
    if CLASSIFY_STRAINS["m"]:
        order = CLASSIFY_STRAINS["order"].setdefault(SCOPE["label"], [])
        if table not in order:
            order.append(table)


def strain_row_sets(indptr, indices, data, n_rows, called_cols):
    """np.uint16[n_rows] from a cluster's CSR matrix (row = k-mer, column = strain) and the called columns c_1 .. c_L, L <= 16: bit
    j - 1 of row r's mask is set when the row is non-zero in column c_j.  Uncalled columns are not looked at.  The mask twin of
    strain_row_labels: where a mask has one bit, that row has the bit's label there."""
    called_cols = list(called_cols)
    if len(called_cols) > _lib.STRAIN_SET_MAX:
        raise ValueError("%d called strains, a mask holds %d" % (len(called_cols), _lib.STRAIN_SET_MAX))
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices)
    n_mat = indptr.size - 1
    n_cols = int(indices.max()) + 1 if indices.size else 0
    col_bit = np.zeros(max(n_cols, max(called_cols + [0]) + 1), np.uint16)
    for j, c in enumerate(called_cols):
        col_bit[c] |= np.uint16(1 << j)
    bits = col_bit[indices]                                          # the called columns only ...
    if data is not None and not np.asarray(data).all():
        bits = np.where(np.asarray(data) != 0, bits, 0).astype(np.uint16)
    at = np.flatnonzero(bits)                                        # (a few of a cluster's many columns: short from here on)
    rows = np.searchsorted(indptr, at, side="right") - 1
    bits = bits[at]
    mat = np.zeros(n_mat, np.uint16)
    for j in range(len(called_cols)):                                # ... or-ed together row by row, a strain at a time
        mat[rows[(bits >> j) & 1 != 0]] |= np.uint16(1 << j)
    out = np.zeros(n_rows, np.uint16)
    m = min(n_rows, n_mat)
    out[:m] = mat[:m]
    return out


def strain_reads_share(set_reads, n):
    """[share of strain j, j = 0..n]: the sum over the sets that hold j, in ascending mask order, of set_reads / |set|; entry 0:
    the unassigned reads.  The entries add up to the sample's records."""
    share = [float(int(set_reads[0]))] + [0.0] * n
    for mask in np.flatnonzero(np.asarray(set_reads)[1:]) + 1:
        members = [j for j in range(1, n + 1) if (int(mask) >> (j - 1)) & 1]
        for j in members:
            share[j] += int(set_reads[mask]) / len(members)
    return share


def strain_classes_text(clusters):
    """The text of strain_classes.tsv for [(table, [(n, name)] in report order, the numbers of ReadSet.classify_strains)]."""
    out = ["table\tstrain\tkmers\thits\treads_unique\treads_tied\treads_share\n"]
    for table, called, r in clusters:
        share = strain_reads_share(r["set_reads"], len(called))
        out.append("%s\tunassigned\t0\t%d\t%d\t0\t%.3f\n" % (table, int(r["strain_hits"][0]), int(r["unique"][0]), share[0]))
        for j, (n, name) in enumerate(called, 1):
            out.append("%s.%d\t%s\t%d\t%d\t%d\t%d\t%.3f\n" % (table, n, name, int(r["kmers"][j]), int(r["strain_hits"][j]), int(r["unique"][j]),
                                                             int(r["tied"][j]), share[j]))
    return "".join(out)


def strain_sets_text(clusters):
    """The text of strain_sets.tsv: per cluster a row for every non-empty set with reads, the reads descending, then the mask
    ascending; `set`: the report numbers of its strains."""
    out = ["table\tset\tstrains\treads\n"]
    for table, called, r in clusters:
        sr = np.asarray(r["set_reads"])
        masks = [int(m) for m in np.flatnonzero(sr[1:]) + 1]
        for mask in sorted(masks, key=lambda m: (-int(sr[m]), m)):
            members = [str(n) for j, (n, _) in enumerate(called) if (mask >> j) & 1]
            out.append("%s\t%s\t%d\t%d\n" % (table, ",".join(members), len(members), int(sr[mask])))
    return "".join(out)


def collect_strain_classes(cls, cls_db_dir, report_path, ksize, paths):
    """After cluster `cls` ('C<id>') has written report_path: its numbers for strain_classes.tsv and strain_sets.tsv and, with
    --extract_strains, its called strains' extracted/strain_<cls>.<n>_* files.  A no-op unless --classify_strains is on.  The
    solver's threads call this; a cluster that has its numbers under the current scope keeps them."""
    m = CLASSIFY_STRAINS["m"]
    if not m or CLASSIFY_STRAINS["skipped"] is not None or not os.path.exists(report_path):
        return
    from .tree import load_plain_pkl
    with _CLASSIFY_STRAINS_LOCK:
        rows = CLASSIFY_STRAINS["rows"].setdefault(SCOPE["label"], {})
        if cls in rows or CLASSIFY_STRAINS["skipped"] is not None:
            return
        called = called_strains(report_path)
        if not called:
            return
        if dist.is_distributed():
            return _classify_strains_skip("runs on one rank only (this run has several)")
        if len(called) > _lib.STRAIN_SET_MAX:
            rows[cls] = None
            print("classify_strains: %s has %d called strains, a read's set holds up to %d, and the cluster was not written" %
                  (cls, len(called), _lib.STRAIN_SET_MAX), file=sys.stderr)
            if EM_STRAINS["on"] and EM_STRAINS["skipped"] is None:
                print("em_strains: %s has %d called strains, a read's set holds up to %d, and the cluster was not written" %
                      (cls, len(called), _lib.STRAIN_SET_MAX), file=sys.stderr)
            sys.stderr.flush()
            return
        rs = _report_reads(paths)
        if rs is None:
            return _classify_strains_skip(NEEDS_RESIDENT)
        sid = load_plain_pkl(os.path.join(cls_db_dir, "id2strain_re.pkl"))
        col_of = {name: c for c, name in (sid.items() if isinstance(sid, dict) else enumerate(sid))}
        indptr, indices, data = cluster_csr_arrays(os.path.join(cls_db_dir, "all_strains_re.npz"))
        with contextlib.closing(db.fasta_index(os.path.join(cls_db_dir, "all_kmer.fasta"), int(ksize), 2)) as kdb:
            if kdb.k < 17:
                return _classify_strains_skip(NEEDS_PAGE_INDEX % kdb.k)
            row_sets = strain_row_sets(indptr, indices, data, kdb.n_rows, [col_of[name] for _, name in called])
            res = _select_or_skip(lambda: rs.classify_strains(kdb, row_sets, len(called), m), _classify_strains_skip, "classify")
            if res is None:
                return
            rows[cls] = (called, res)
            records = int(res["unique"].sum() + res["tied"][0])
            print("classify_strains: %s\tM=%d\trecords %d\tunique %d\ttied %d\tunassigned %d\tsets %d" %
                  (cls, m, records, int(res["unique"][1:].sum()), int(res["tied"][0]), int(res["unique"][0]),
                   int((res["set_reads"][1:] > 0).sum())), file=sys.stderr)
            sys.stderr.flush()
            _write_strain_sets(cls, called, rs, kdb, row_sets, m, paths)
            collect_em_strains(cls, called, res, rs, kdb, row_sets, m, report_path)


def _write_strain_sets(cls, called, rs, kdb, row_sets, m, paths):
    """--extract_strains: extracted/strain_<cls>.<n>_<mate>.<ext> for every called strain of `cls`, from one ReadSet.select_strains
    (_CLASSIFY_STRAINS_LOCK held)."""
    mode = EXTRACT_STRAINS["mode"]
    if not mode or EXTRACT_STRAINS["skipped"] is not None:
        return
    ps = [p for p in paths if p]
    if any(_lib.input_kind(p) == "bam" for p in ps):
        return _extract_strains_skip("takes FASTA/FASTQ inputs (BAM subsets per strain are not built)")
    how = 0 if mode == "unique" else 1
    sets = _select_or_skip(lambda: rs.select_strains(kdb, row_sets, len(called), m, [1 << j for j in range(len(called))], [how] * len(called)),
                           _extract_strains_skip, "extract")
    if sets is None:
        return
    try:
        out_dir = os.path.join(EXTRACT_READS["dir"] or ".", EXTRACT_READS_DIR)
        os.makedirs(out_dir, exist_ok=True)
        for (n, _), sub in zip(called, sets):
            selected = sub.info()["n_records"]
            flat = sub.read_back()
            sub.close()
            keys = _lib.flat_record_keys(flat)
            del flat
            outs = [os.path.join(out_dir, "strain_%s.%d_%d.%s" % (cls, n, i + 1, fastx_record_type(p))) for i, p in enumerate(ps)]
            c = _extract_write(ps, keys, outs)
            EXTRACT_STRAINS["files"].extend(outs)
            print("extract_strains: %s.%d\t%s\tM=%d\tselected on the device %d\twritten %d" % (cls, n, mode, m, selected, c["written"]),
                  file=sys.stderr)
        sys.stderr.flush()
    finally:
        for sub in sets:
            sub.close()


def write_strain_classes(out_dir, scope=None):
    """out_dir/strain_classes.tsv and strain_sets.tsv from the numbers collected under `scope`, clusters in the order of the scans;
    nothing without the flag, without numbers, or after a skip."""
    rows = {t: r for t, r in (CLASSIFY_STRAINS["rows"].get(scope) or {}).items() if r is not None}
    if not CLASSIFY_STRAINS["m"] or CLASSIFY_STRAINS["skipped"] is not None or not rows:
        return None
    clusters = [(t,) + rows[t] for t in _in_order(CLASSIFY_STRAINS["order"].get(scope, []), rows)]
    _write(out_dir, STRAIN_SETS_FILE, strain_sets_text(clusters))
    return _write(out_dir, STRAIN_CLASSES_FILE, strain_classes_text(clusters))


# --em_strains B (StrainScan.apply_em_strains turns it on; it needs --classify_strains): the read-based abundance estimate that
# strain_sets.tsv's equivalence classes are the start of.  Behind a cluster's classification (collect_strain_classes, its lock
# held) collect_em_strains takes the sample's set counts, the set counts of B resampled replicates -- sixteen per device call, from
# one classification each and nothing materialised (ReadSet.strain_sets_resampled; replicate b of seed S is --bootstrap's) --
# compacts all B + 1 vectors to the masks that have reads in any of them and runs ONE batched EM (_lib.em_strain_sets; the rule is
# in strainscan_hip.h, tests/em_model.py restates it).  "rows": per scope and cluster, the called strains, their k-mers, the
# elastic-net fractions of the report, N, rho[B + 1, L] (row 0: the sample) and the iterations, of which strain_em.tsv is a pure
# function (em_text).  The clusters are listed in CLASSIFY_STRAINS' order.
EM_STRAINS = {"on": False, "b": 0, "seed": 1, "rows": {}, "skipped": None}
EM_STRAINS_FILE = "strain_em.tsv"
EM_MAX_ITER = 1000
EM_TOL = 1e-9


def em_strains_reset(b=None, seed=1):
    EM_STRAINS.update(on=b is not None, b=int(b or 0), seed=int(seed), rows={}, skipped=None)


def _em_strains_skip(why):
    if EM_STRAINS["on"]:
        _skip(EM_STRAINS, "em_strains", "and no abundance was estimated", True, why)


def em_replicates(scope=None):
    """{cluster: (strain names in report order, rho np.float64[B + 1, L], iters np.uint32[B + 1])} collected under `scope`: row 0
    is the sample's estimate, row 1 + b replicate b's."""
    return {cls: ([name for _, name in r["called"]], r["rho"].copy(), r["iters"].copy()) for cls, r in EM_STRAINS["rows"].get(scope, {}).items()}


def em_abundance(rho, kmers):
    """theta[v][j] = (rho[v][j] / kmers[j]) / the sum of that over the strains with kmers > 0 (0 where the sum is 0): reads per
    k-mer of the strain, as a share.  rho: [V, L]; kmers: [L]."""
    rho = np.asarray(rho, np.float64)
    km = np.asarray(kmers, np.float64)
    per = np.divide(rho, km[None, :], out=np.zeros_like(rho), where=km[None, :] > 0)
    tot = np.zeros(rho.shape[0], np.float64)
    for j in range(rho.shape[1]):      # (strain after strain: one order of summation, whatever the shape)
        tot += per[:, j]
    return np.divide(per, tot[:, None], out=np.zeros_like(per), where=tot[:, None] != 0)


def em_text(clusters):
    """The text of strain_em.tsv for [(table, dict(called=[(n, name)] in report order, kmers=[L], enet=[L] texts, reads=N,
    rho=[B + 1, L], iters=[B + 1]))]: the bounds are the replicates' abundances at bootstrap_index(0.025 / 0.975, B) of the
    ascending values, `-` without replicates."""
    out = ["table\tstrain\tkmers\treads_assigned\treads_em\tfrac_reads\tabundance\tabundance_lo\tabundance_hi\tpresent\tenet_frac\titerations\n"]
    for table, r in clusters:
        rho = np.asarray(r["rho"], np.float64)
        theta = em_abundance(rho, r["kmers"])
        b = rho.shape[0] - 1
        if b:
            lo, hi = (bootstrap_index(q, b) for q in BOOTSTRAP_QUANTILES)
            ts = np.sort(theta[1:], axis=0)
        for j, (n, name) in enumerate(r["called"]):
            bounds = ["%.6f" % ts[lo, j], "%.6f" % ts[hi, j], str(int((rho[1:, j] > 0).sum()))] if b else ["-", "-", "-"]
            out.append("\t".join(["%s.%d" % (table, n), name, str(int(r["kmers"][j])), str(int(r["reads"])), "%.3f" % (rho[0, j] * int(r["reads"])),
                                  "%.6f" % rho[0, j], "%.6f" % theta[0, j]] + bounds + [r["enet"][j], str(int(r["iters"][0]))]) + "\n")
    return "".join(out)


def collect_em_strains(cls, called, res, rs, kdb, row_sets, m, report_path):
    """Behind cluster `cls`' classification `res` (collect_strain_classes, _CLASSIFY_STRAINS_LOCK held): the EM on its set counts and
    on those of the replicates.  A no-op unless --em_strains is on."""
    if not EM_STRAINS["on"] or EM_STRAINS["skipped"] is not None:
        return
    b, seed, n = EM_STRAINS["b"], EM_STRAINS["seed"], len(called)
    vectors = [np.asarray(res["set_reads"], np.uint64)[None, :]]
    for first in range(0, b, _lib.SCAN_REPLICATES_MAX):
        got = _select_or_skip(lambda: rs.strain_sets_resampled(kdb, row_sets, n, m, seed, first, min(_lib.SCAN_REPLICATES_MAX, b - first)),
                              _em_strains_skip, "resample")
        if got is None:
            return
        vectors.append(got)
    counts = np.concatenate(vectors, axis=0)
    counts[:, 0] = 0                                                  # the unassigned reads take no part
    masks = np.flatnonzero(counts.any(axis=0))                        # the sets with reads in the sample or in any replicate
    if masks.size:
        rho, iters = _lib.em_strain_sets(counts[:, masks], masks.astype(np.uint16), n, EM_MAX_ITER, EM_TOL)
    else:
        rho, iters = np.zeros((b + 1, n), np.float64), np.zeros(b + 1, np.uint32)
    enet = {name: frac for _, name, frac, _ in report_rows(report_path)}
    EM_STRAINS["rows"].setdefault(SCOPE["label"], {})[cls] = dict(
        called=list(called), kmers=[int(k) for k in res["kmers"][1:]], enet=[enet[name] for _, name in called], reads=int(counts[0].sum()), rho=rho,
        iters=iters)
    print("em_strains: %s\tB=%d\tseed=%d\tsets %d\titerations %d\tlargest over the replicates %d\treplicates at max_iter %d" %
          (cls, b, seed, masks.size, int(iters[0]), int(iters[1:].max()) if b else 0, int((iters[1:] >= EM_MAX_ITER).sum())), file=sys.stderr)
    sys.stderr.flush()


def write_em_strains(out_dir, scope=None):
    """out_dir/strain_em.tsv from the numbers collected under `scope`, clusters in the order of the scans; nothing without the
    flag, without numbers, or after a skip."""
    rows = EM_STRAINS["rows"].get(scope) or {}
    if not EM_STRAINS["on"] or EM_STRAINS["skipped"] is not None or not rows:
        return None
    return _write(out_dir, EM_STRAINS_FILE, em_text([(t, rows[t]) for t in _in_order(CLASSIFY_STRAINS["order"].get(scope, []), rows)]))


# --divergence M (StrainScan.apply_divergence turns it on): every report above takes the called strains for the right ones; this asks
# whether the sample's organism IS a called strain or a relative of one.  After a cluster's StrainVote.report has been written,
# collect_divergence marks the rows of the cluster's table that any called strain has (called_rows: the union of their columns, no
# limit on their number) and the device walks every read's k-mer hits in order (ReadSet.gaps; the rule is in strainscan_hip.h,
# tests/gap_model.py restates it): a run of k missing k-mers between two k-mers of the called strains is one base that differs.
# Written as strain_divergence.tsv, a row per cluster.  "rows": per scope and cluster, the report numbers of the called strains and
# the device's totals; "order": the tables as they were scanned.
DIVERGENCE = {"m": 0, "rows": {}, "order": {}, "skipped": None}
DIVERGENCE_FILE = "strain_divergence.tsv"
DIVERGENCE_COLUMNS = ("windows", "hits_called", "hits_cluster", "misses", "gap_lt", "gap_km1", "gap_k", "gap_k_2k", "gap_ge2k", "gaps_in_cluster",
                      "sites", "reads_with_sites", "detectable")
_DIVERGENCE_LOCK = threading.Lock()
_divergence_skip = functools.partial(_skip, DIVERGENCE, "divergence", "and no divergence was estimated", True)


def divergence_reset(m=0):
    DIVERGENCE.update(m=int(m or 0), rows={}, order={}, skipped=None)


def divergence_scanned(table):
    """A table has been scanned: strain_divergence.tsv lists the clusters in this order."""
    if DIVERGENCE["m"]:
        order = DIVERGENCE["order"].setdefault(SCOPE["label"], [])
        if table not in order:
            order.append(table)


def called_rows(indptr, indices, data, n_rows, called_cols):
    """np.uint8[n_rows] from a cluster's CSR matrix (row = k-mer, column = strain) and the called columns, any number of them: 1
    where the row is non-zero in a called column.  Uncalled columns are not looked at."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices)
    n_mat = indptr.size - 1
    n_cols = int(indices.max()) + 1 if indices.size else 0
    is_called = np.zeros(max(n_cols, max(list(called_cols) + [0]) + 1), bool)
    is_called[list(called_cols)] = True
    hit = is_called[indices]
    if data is not None and not np.asarray(data).all():
        hit = hit & (np.asarray(data) != 0)
    rows = np.searchsorted(indptr, np.flatnonzero(hit), side="right") - 1
    mat = np.zeros(n_mat, np.uint8)
    mat[rows] = 1
    out = np.zeros(n_rows, np.uint8)
    m = min(n_rows, n_mat)
    out[:m] = mat[:m]
    return out


def divergence_text(clusters):
    """The text of strain_divergence.tsv for [(table, [report numbers of the called strains], the totals of ReadSet.gaps)]."""
    out = ["\t".join(("table", "strains", "kmers", "kmers_called", "reads") + DIVERGENCE_COLUMNS + ("per_kb",)) + "\n"]
    for table, numbers, r in clusters:
        per_kb = "%.3f" % (1000.0 * r["sites"] / r["detectable"]) if r["detectable"] else "-"
        out.append("\t".join([table, ",".join(str(n) for n in numbers), str(r["kmers"]), str(r["kmers_called"]), str(r["assessed"])] +
                             [str(r[c]) for c in DIVERGENCE_COLUMNS] + [per_kb]) + "\n")
    return "".join(out)


def collect_divergence(cls, cls_db_dir, report_path, ksize, paths):
    """After cluster `cls` ('C<id>') has written report_path: its row of strain_divergence.tsv.  A no-op unless --divergence is on.
    The solver's threads call this; a cluster that has its numbers under the current scope keeps them."""
    m = DIVERGENCE["m"]
    if not m or DIVERGENCE["skipped"] is not None or not os.path.exists(report_path):
        return
    from .tree import load_plain_pkl
    with _DIVERGENCE_LOCK:
        rows = DIVERGENCE["rows"].setdefault(SCOPE["label"], {})
        if cls in rows or DIVERGENCE["skipped"] is not None:
            return
        called = called_strains(report_path)
        if not called:
            return
        if dist.is_distributed():
            return _divergence_skip("runs on one rank only (this run has several)")
        rs = _report_reads(paths)
        if rs is None:
            return _divergence_skip(NEEDS_RESIDENT)
        sid = load_plain_pkl(os.path.join(cls_db_dir, "id2strain_re.pkl"))
        col_of = {name: c for c, name in (sid.items() if isinstance(sid, dict) else enumerate(sid))}
        indptr, indices, data = cluster_csr_arrays(os.path.join(cls_db_dir, "all_strains_re.npz"))
        with contextlib.closing(db.fasta_index(os.path.join(cls_db_dir, "all_kmer.fasta"), int(ksize), 2)) as kdb:
            if kdb.k < 17:
                return _divergence_skip(NEEDS_PAGE_INDEX % kdb.k)
            row_called = called_rows(indptr, indices, data, kdb.n_rows, [col_of[name] for _, name in called])
            res = _select_or_skip(lambda: rs.gaps(kdb, row_called, m), _divergence_skip, "walk")
            if res is None:
                return
            rows[cls] = ([n for n, _ in called], res)
            print("divergence: %s\tM=%d\trecords %d\tassessed %d\tsites %d\tdetectable %d" %
                  (cls, m, res["records"], res["assessed"], res["sites"], res["detectable"]), file=sys.stderr)
            sys.stderr.flush()


def write_divergence(out_dir, scope=None):
    """out_dir/strain_divergence.tsv from the numbers collected under `scope`, clusters in the order of the scans; nothing without
    the flag, without numbers, or after a skip."""
    rows = DIVERGENCE["rows"].get(scope) or {}
    if not DIVERGENCE["m"] or DIVERGENCE["skipped"] is not None or not rows:
        return None
    return _write(out_dir, DIVERGENCE_FILE, divergence_text([(t,) + rows[t] for t in _in_order(DIVERGENCE["order"].get(scope, []), rows)]))


# --bootstrap B (StrainScan.apply_bootstrap turns it on): how firm are a multi-strain cluster's numbers?  After the cluster has
# written its StrainVote.report, collect_bootstrap resamples the reads that carry k-mers of its table B times on the device
# (ReadSet.resample: a Poisson bootstrap over reads, replicate b of seed S), re-counts the table from each resampled set and solves
# each replicate again with the main solve's strains and alpha held fixed (replicate_coefs).
# "solve": the main solve's state, left by detect_core per solving thread while the flag is on; "rows": per scope and cluster, the
# report's rows and the [B, p] matrix of replicate coefficients, of which strain_bootstrap.tsv is a pure function (bootstrap_text);
# "order": the tables as they were scanned.
BOOTSTRAP = {"b": 0, "seed": 1, "solve": {}, "rows": {}, "order": {}, "skipped": None}
BOOTSTRAP_FILE = "strain_bootstrap.tsv"
BOOTSTRAP_QUANTILES = (0.025, 0.975)
_BOOTSTRAP_LOCK = threading.Lock()
_bootstrap_skip = functools.partial(_skip, BOOTSTRAP, "bootstrap", "and no intervals were computed", True)


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
    """A table has been scanned: strain_bootstrap.tsv lists the clusters in this order."""
    if BOOTSTRAP["b"]:
        order = BOOTSTRAP["order"].setdefault(SCOPE["label"], [])
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


def replicate_coefs(img, om, solve, counts):
    """One bootstrap replicate of a cluster (--bootstrap, collect_bootstrap): the coefficients of the strains the main solve
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
    with contextlib.closing(img.prepare(remove_1(counts), solve["new_als"], solve["npp25"], solve["npp75"], solve["npp_out"])) as vec:
        if p == 1:
            qd = img.quantile_sums(vec.yu if vec.use_u else vec.y, cols, 25, 75)
            if qd["n_nz"][0] == 0 or qd["cnt_in"][0] == 0:
                return np.zeros(1)
            return np.array([float(qd["sum_in"][0]) / float(qd["cnt_in"][0])])
        n = vec.n_keep
        if n == 0:
            return np.zeros(p)
        with contextlib.closing(img.fold_words(vec.keep, np.zeros(n, np.uint32), n)) as fold:
            stats = img.pattern_stats(cols, vec.ykeep, fold, 0)
        Qt, qt, yyt, nt = L2.gram_from_stats(stats[0], p)
        fit = L2.enet_path_gram(Qt[None], qt[None], [yyt], [nt], [solve["alpha"]], l1_ratio=0.5, max_iter=MAX_NITER, tol=1e-4,
                                positive=True)
        return fit["coefs"][0, 0].copy()


def collect_bootstrap(cls, cls_db_dir, report_path, ksize, paths):
    """After cluster `cls` ('C<id>') has written report_path: B replicate solves of it.  A no-op unless --bootstrap is on.  Every
    rank calls this at the same point (it holds collectives): each resamples its own shard of the reads -- the weights depend on
    a read's bytes alone, so the summed counts are those of one process."""
    solve = BOOTSTRAP["solve"].pop(threading.get_ident(), None)
    b = BOOTSTRAP["b"]
    if not b or BOOTSTRAP["skipped"] is not None or solve is None or not solve.get("columns") or not os.path.exists(report_path):
        return
    from . import identify_strains_L2_Enet_Pscan_new_sp as enet
    with _BOOTSTRAP_LOCK:
        if BOOTSTRAP["skipped"] is not None:
            return
        rows = BOOTSTRAP["rows"].setdefault(SCOPE["label"], {})
        if cls in rows:
            return
        called = report_rows(report_path)
        if not called:
            return
        if int(ksize) < 17:
            return _bootstrap_skip(NEEDS_PAGE_INDEX % int(ksize))
        rs = _report_reads(paths)
        if rs is None:
            return _bootstrap_skip(NEEDS_RESIDENT)
        with contextlib.closing(db.fasta_index(os.path.join(cls_db_dir, "all_kmer.fasta"), int(ksize), 2).expect_hits()) as kdb:
            # reads without a hit add nothing to any count: only the others are resampled
            sub = _select_or_skip(lambda: rs.select(kdb, 1), _bootstrap_skip, "resample")
            if sub is None:
                return
            with contextlib.closing(sub):
                img, om = enet.open_cluster_image(cls_db_dir + "/all_strains_re.npz", cls_db_dir + "/overlap_matrix.npz")
                with contextlib.closing(img):
                    coefs = np.zeros((b, len(solve["columns"])), np.float64)
                    for rep in range(b):
                        with contextlib.closing(sub.resample(BOOTSTRAP["seed"], rep)) as rb:
                            kdb.reset()
                            rb.order().scan_into(kdb)    # binned first: 2.2 + 6.2 ms beside 16.6 ms for 20 M reads (profiles/r21_bootstrap.md)
                            if dist.is_distributed():
                                dist.allreduce_table(kdb)
                            _lib.check(_lib.lib().ss_device_sync(), "ss_device_sync")
                            counts = kdb.counts_rows()
                        coefs[rep] = replicate_coefs(img, om, solve, counts)
        col_of = {str(name): j for j, name in enumerate(solve["strains"])}
        rows[cls] = dict(strains=[str(s) for s in solve["strains"]], coefs=coefs,
                         called=[(n, name, depth, frac, col_of[name]) for n, name, frac, depth in called if name in col_of])


def write_bootstrap(out_dir, scope=None):
    """out_dir/strain_bootstrap.tsv from the replicates collected under `scope`, clusters in the order scanned, strains in report
    order; nothing without the flag, without a solved multi-strain cluster, or after a skip."""
    rows = BOOTSTRAP["rows"].get(scope)
    if not BOOTSTRAP["b"] or BOOTSTRAP["skipped"] is not None or not rows:
        return None
    lines = [("%s.%d" % (t, n), name, depth, frac, col, rows[t]["coefs"])
             for t in _in_order(BOOTSTRAP["order"].get(scope, []), rows) for n, name, depth, frac, col in rows[t]["called"]]
    return _write(out_dir, BOOTSTRAP_FILE, bootstrap_text(lines)) if lines else None


# --bootstrap_clusters B (StrainScan.apply_bootstrap_clusters turns it on; it shares --bootstrap_seed): would a second sequencing
# run of the library have called the same clusters?  Once the tree walk has returned, collect_cluster_bootstrap takes the counts of
# the tree's table under B replicates of the reads -- ReadSet.scan_resampled: one pass over the resident reads per chunk of
# replicates, no replicate is materialised -- loads each vector into the table and runs the walk of this run's cutoff ladder on it;
# then the main run's counts go back.  "rows": per scope, the main run's {leaf id: (cls_ab, cls_cov)}, the list of the replicates'
# and the replicates that called nothing (failed); cluster_bootstrap.tsv is a pure function of the first two
# (cluster_bootstrap_text).  "skipped": per scope, why nothing is written (a database of strainscan-multi that cannot be walked
# does not take the others with it).
CLUSTER_BOOTSTRAP = {"b": 0, "seed": 1, "rows": {}, "skipped": {}}
CLUSTER_BOOTSTRAP_FILE = "cluster_bootstrap.tsv"
CLUSTER_BOOTSTRAP_VECTOR_BYTES = 1 << 30      # a chunk's row vectors take at most this much (and its slot counters 16 GB)
CLUSTER_BOOTSTRAP_SLOT_BYTES = 16 << 30
_CLUSTER_BOOTSTRAP_LOCK = threading.Lock()


def cluster_bootstrap_reset(b=0, seed=1):
    CLUSTER_BOOTSTRAP.update(b=int(b or 0), seed=int(seed), rows={}, skipped={})


def _cluster_bootstrap_skip(why):
    scope = SCOPE["label"]
    if scope not in CLUSTER_BOOTSTRAP["skipped"]:
        CLUSTER_BOOTSTRAP["skipped"][scope] = why
        if dist.rank_world()[0] == 0:
            print("bootstrap_clusters: %s and no intervals were computed" % why, file=sys.stderr)
            sys.stderr.flush()


def cluster_bootstrap_replicates(scope=None):
    """The replicates collected under `scope`: a list of B dicts {leaf id: (cls_ab, cls_cov)}, empty for a replicate that called
    no cluster (tests; cluster_bootstrap.tsv is cluster_bootstrap_text of these and the main run's dict)."""
    return [dict(r) for r in CLUSTER_BOOTSTRAP["rows"].get(scope, {}).get("replicates", [])]


def cluster_bootstrap_failed(scope=None):
    """The replicates under `scope` whose ladder ended without a cluster."""
    return int(CLUSTER_BOOTSTRAP["rows"].get(scope, {}).get("failed", 0))


def cluster_bootstrap_walk_seed(seed, replicate):
    """What numpy's global generator is seeded with before replicate `replicate`'s walk (the walk's Poisson draw,
    cst.Walk.adjust_profile, is unseeded as in the reference): the same S gives the same file.  The generator's state is put
    back afterwards, so the rest of the run draws what it draws without the flag."""
    return (int(seed) * 1000003 + int(replicate)) % (1 << 32)


def cluster_bootstrap_text(main, replicates):
    """The text of cluster_bootstrap.tsv: main = the main run's {leaf id: (cls_ab, cls_cov)}, replicates = a list of B such
    dicts.  One row per cluster that either identified, ascending by id; a replicate without the cluster contributes 0.0; the
    bounds are the values at bootstrap_index(0.025 / 0.975, B) of the ascending replicate values, as in strain_bootstrap.tsv."""
    b = len(replicates)
    out = ["cluster\tcalled\treplicates\tpresent\tdepth\tdepth_lo\tdepth_hi\tcov\tcov_lo\tcov_hi\n"]
    if not b:
        return out[0]
    lo, hi = (bootstrap_index(q, b) for q in BOOTSTRAP_QUANTILES)
    ids = set(main)
    for r in replicates:
        ids.update(r)
    for cid in sorted(ids):
        depths = sorted(float(r[cid][0]) if cid in r else 0.0 for r in replicates)
        covs = sorted(float(r[cid][1]) if cid in r else 0.0 for r in replicates)
        depth, cov = (str(float(main[cid][0])), str(float(main[cid][1]))) if cid in main else ("-", "-")
        out.append("\t".join(["C%s" % cid, "1" if cid in main else "0", str(b), str(sum(1 for r in replicates if cid in r)), depth,
                              str(depths[lo]), str(depths[hi]), cov, str(covs[lo]), str(covs[hi])]) + "\n")
    return "".join(out)


def _ladder_walk(img, tree_db_dir, ldep, params):
    """What StrainScan.identify_with_ladder runs for -l `ldep`, on the counts the image holds now: the walk at the first rung and,
    at -l 0, at the second when the first calls nothing.  The trace lines go nowhere."""
    from . import cst
    from .StrainScan import LADDER_CUTOFFS
    res = {}
    for cutoff in LADDER_CUTOFFS[ldep]:
        res = cst.Walk(cst.ImageProvider(img), tree_db_dir, list(cutoff), params, out=lambda *a: None).run()
        if len(res):
            break
    return res


def collect_cluster_bootstrap(cls_dict, tree_db_dir, ldep, mdb, paths):
    """Once the tree walk has returned `cls_dict` (final: nothing of the main result is made after this): B walks on resampled
    counts.  A no-op unless --bootstrap_clusters is on; a scope that has its replicates keeps them.  The table's counters and the
    image's cached counts and statistics are what they were when this returns, whatever happens in between."""
    b, seed = CLUSTER_BOOTSTRAP["b"], CLUSTER_BOOTSTRAP["seed"]
    if not b:
        return
    from . import identify, identify_low_mem
    from .tree import read_tree_structure
    with _CLUSTER_BOOTSTRAP_LOCK:
        scope = SCOPE["label"]
        if scope in CLUSTER_BOOTSTRAP["rows"] or scope in CLUSTER_BOOTSTRAP["skipped"]:
            return
        if dist.is_distributed():
            return _cluster_bootstrap_skip("runs on one rank (the replicates' counts are not summed over ranks),")
        if PAIRS["on"] and not _pairs_gate(paths):
            return _cluster_bootstrap_skip("--pairs %s" % PAIRS["skipped"])
        mod = identify_low_mem if mdb else identify
        img = db.tree_image(tree_db_dir, mod._UPPER_KEYS)
        if img.is_external:
            return _cluster_bootstrap_skip("needs the tree's table scanned by this process (its counts came from elsewhere)")
        kdb = img.kdb
        if kdb.k < 17:
            return _cluster_bootstrap_skip(NEEDS_PAGE_INDEX % kdb.k)
        if len(read_tree_structure(tree_db_dir)[0]) < 2:
            return _cluster_bootstrap_skip("needs a cluster search tree (this database has a single cluster)")
        if not len(cls_dict):
            return _cluster_bootstrap_skip("the main run detected no cluster")
        rs = _report_reads(paths)
        if rs is None:
            return _cluster_bootstrap_skip(NEEDS_RESIDENT)
        n_rows, n_slots = max(int(kdb.n_rows), 1), max(int(kdb.info()["n_slots"]), 1)
        chunk = max(1, min(_lib.SCAN_REPLICATES_MAX, CLUSTER_BOOTSTRAP_VECTOR_BYTES // (4 * n_rows), CLUSTER_BOOTSTRAP_SLOT_BYTES // (4 * n_slots)))
        replicates, failed = [], 0
        cached = img._counts, img._stats
        rng = np.random.get_state()
        saved = _lib.ReplicateCounts(1, kdb.n_rows)
        try:
            kdb.counts_rows_dev(saved.dptr)
            _lib.check(_lib.lib().ss_device_sync(), "ss_device_sync")
            try:
                for first in range(0, b, chunk):
                    n = min(chunk, b - first)
                    out = _select_or_skip(lambda: rs.scan_resampled(kdb, seed, first, n), _cluster_bootstrap_skip, "resample")
                    if out is None:
                        return
                    with contextlib.closing(out):
                        for j in range(n):
                            out.load_into(kdb, j)
                            img._counts = img._stats = None
                            np.random.seed(cluster_bootstrap_walk_seed(seed, first + j))
                            try:
                                res = _ladder_walk(img, tree_db_dir, ldep, mod._PARAMS)
                            except (ValueError, IndexError):      # (the empty max of the walk's last resort, as the reference raises it)
                                res = {}
                            failed += 0 if len(res) else 1
                            replicates.append({cid: (float(e["cls_ab"]), float(e["cls_cov"])) for cid, e in res.items()})
                        _lib.check(_lib.lib().ss_device_sync(), "ss_device_sync")
            finally:
                # everything after this point sees the main run's counts
                kdb.load_counts_rows_dev(saved.dptr)
                _lib.check(_lib.lib().ss_device_sync(), "ss_device_sync")
                img._counts, img._stats = cached
                np.random.set_state(rng)
        finally:
            saved.close()
        main = {cid: (float(e["cls_ab"]), float(e["cls_cov"])) for cid, e in cls_dict.items()}
        CLUSTER_BOOTSTRAP["rows"][scope] = dict(main=main, replicates=replicates, failed=failed)
        seen = set()
        for r in replicates:
            seen.update(r)
        print("bootstrap_clusters: B=%d\tS=%d\tcalled %d\tseen in a replicate %d\tfailed %d" % (b, seed, len(main), len(seen), failed),
              file=sys.stderr)
        sys.stderr.flush()


def write_cluster_bootstrap(out_dir, scope=None):
    """out_dir/cluster_bootstrap.tsv from the replicates collected under `scope`; nothing without the flag or after a skip."""
    r = CLUSTER_BOOTSTRAP["rows"].get(scope)
    if not CLUSTER_BOOTSTRAP["b"] or scope in CLUSTER_BOOTSTRAP["skipped"] or not r:
        return None
    return _write(out_dir, CLUSTER_BOOTSTRAP_FILE, cluster_bootstrap_text(r["main"], r["replicates"]))



# --classify_reads M (StrainScan.apply_classify_reads turns it on): every read assigned to a node of the cluster search tree.
# kmers/<id> lists each k-mer of the tree's table under one node, so a read's hits against that table point at nodes; the read goes
# to the node whose root path collects the most hits, ties to the tied nodes' lowest common ancestor, fewer than M hits on the best
# path to nobody (ReadSet.classify; tests/class_model.py restates it).  Collected once per scope behind the tree scan, summed over
# the ranks, written as read_classes.tsv: a row per node, reads_direct the reads of that class, reads_clade those of the node and
# everything below it.
CLASSIFY_READS = {"m": 0, "rows": {}, "skipped": None}
READ_CLASSES_FILE = "read_classes.tsv"
_CLASSIFY_READS_LOCK = threading.Lock()
_classify_reads_skip = functools.partial(_skip, CLASSIFY_READS, "classify_reads", "and no read was classified", True)


def classify_reads_reset(m=0):
    CLASSIFY_READS.update(m=int(m or 0), rows={}, skipped=None)


def tree_row_nodes(node_ids, node_rows, n_rows):
    """np.uint32[n_rows]: the node (1-based position in node_ids) that lists each row of the tree's table, 0 for a row that no
    node lists or that two different nodes list."""
    rows = [np.asarray(node_rows.get(nid, ()), np.int64).ravel() for nid in node_ids]
    node = np.concatenate([np.full(r.size, v, np.int64) for v, r in enumerate(rows, 1)] or [np.zeros(0, np.int64)])
    row = np.concatenate(rows or [np.zeros(0, np.int64)])
    keep = (row >= 0) & (row < n_rows)
    row, node = row[keep], node[keep]
    lo = np.full(n_rows, np.iinfo(np.int64).max, np.int64)
    hi = np.zeros(n_rows, np.int64)
    np.minimum.at(lo, row, node)
    np.maximum.at(hi, row, node)
    return np.where(lo == hi, hi, 0).astype(np.uint32)


def read_classes_text(node_ids, parent_of, leaves, direct, node_hits, kmers):
    """The text of read_classes.tsv.  node_ids: ascending, node v of the arrays (1-based) is node_ids[v - 1]; parent_of: {id: parent
    id, None for a root}; leaves: the ids that are clusters; direct / node_hits / kmers: [n + 1], entry 0 the unclassified reads,
    the hits of k-mers without a node, and 0."""
    n = len(node_ids)
    num = {nid: v for v, nid in enumerate(node_ids, 1)}
    clade = [int(x) for x in direct]
    for v, nid in enumerate(node_ids, 1):
        p, seen = parent_of.get(nid), 0
        while p is not None and seen <= n:
            clade[num[p]] += int(direct[v])
            p, seen = parent_of.get(p), seen + 1
    out = ["node\tparent\tcluster\tkmers\thits\treads_direct\treads_clade\n",
           "unclassified\t-\t-\t0\t%d\t%d\t%d\n" % (int(node_hits[0]), int(direct[0]), int(direct[0]))]
    for v, nid in enumerate(node_ids, 1):
        p = parent_of.get(nid)
        out.append("%s\t%s\t%s\t%d\t%d\t%d\t%d\n" % (nid, "-" if p is None else p, "C%s" % nid if nid in leaves else "-", int(kmers[v]),
                                                     int(node_hits[v]), int(direct[v]), clade[v]))
    return "".join(out)


def collect_read_classes(img, paths):
    """read_classes.tsv's numbers: the resident reads of `paths` against the tree's table (ReadSet.classify), summed over the
    ranks.  A no-op unless --classify_reads is on; a scope that has its numbers keeps them.  Every rank calls this at the same
    point (it holds a collective).  With --extract_class the same device call (ReadSet.select_class) also gives the sets of the
    listed classes, which are written here; a classification that was skipped takes --extract_class with it."""
    _collect_read_classes(img, paths)
    if EXTRACT_CLASS["items"] and CLASSIFY_READS["skipped"] is not None:
        _extract_class_skip("--classify_reads was skipped (%s)" % CLASSIFY_READS["skipped"])
    if TAG_BAM["on"] and CLASSIFY_READS["skipped"] is not None:
        _tag_bam_skip("--classify_reads was skipped (%s)" % CLASSIFY_READS["skipped"])
    if READ_CALLS["on"] and CLASSIFY_READS["skipped"] is not None:
        _read_calls_skip("--classify_reads was skipped (%s)" % CLASSIFY_READS["skipped"])


def _collect_read_classes(img, paths):
    m = CLASSIFY_READS["m"]
    if not m or CLASSIFY_READS["skipped"] is not None:
        return
    from .tree import read_tree_structure
    with _CLASSIFY_READS_LOCK:
        if SCOPE["label"] in CLASSIFY_READS["rows"]:
            return
        if img.is_external:
            return _classify_reads_skip("needs the tree's table scanned by this process (its counts came from elsewhere)")
        kdb = img.kdb
        if kdb.k < 17:
            return _classify_reads_skip(NEEDS_PAGE_INDEX % kdb.k)
        tree, _ = read_tree_structure(img.db_dir)
        if len(tree) < 2:
            return _classify_reads_skip("needs a cluster search tree (this database has a single cluster)")
        node_ids = sorted(set(img.node_ids) | {nd.identifier for nd in tree.all_nodes()})
        if len(node_ids) > _lib.CLASS_NODES_MAX:
            return _classify_reads_skip("takes trees of up to %d nodes (this one has %d)" % (_lib.CLASS_NODES_MAX, len(node_ids)))
        rs = _report_reads(paths)
        if rs is None:
            return _classify_reads_skip(NEEDS_RESIDENT)
        num = {nid: v for v, nid in enumerate(node_ids, 1)}
        parent_of = {nid: (tree.parent(nid).identifier if tree.get_node(nid) is not None and tree.parent(nid) is not None else None)
                     for nid in node_ids}
        parent = np.zeros(len(node_ids) + 1, np.uint32)
        for nid, p in parent_of.items():
            parent[num[nid]] = num[p] if p is not None else 0
        row_node = tree_row_nodes(node_ids, img.node_rows, kdb.n_rows)
        leaves = {nd.identifier for nd in tree.leaves()}
        wanted = _extract_class_wanted(paths, num, leaves)      # (None: --extract_class is off, or cannot run here)
        if not wanted:                                          # (nothing to select, or only `called`, which comes after the walk)
            res = _select_or_skip(lambda: rs.classify(kdb, row_node, parent, m), _classify_reads_skip, "classify")
        else:
            res = _select_or_skip(lambda: _select_classes(rs, kdb, row_node, parent, m, wanted, paths, True), _classify_reads_skip, "classify")
        if res is None:
            return
        if wanted is not None:
            EXTRACT_CLASS["tree"][SCOPE["label"]] = dict(row_node=row_node, parent=parent, num=num, leaves=leaves, m=m)
        v = np.concatenate([res["direct"].astype(np.int64), res["node_hits"].astype(np.int64), [res["ties"]]])
        if dist.is_distributed():
            v = dist.allreduce_int64(v)
        n1 = len(node_ids) + 1
        direct, node_hits = v[:n1], v[n1:2 * n1]
        CLASSIFY_READS["rows"][SCOPE["label"]] = dict(node_ids=node_ids, parent_of=parent_of, leaves=leaves,
                                                      direct=direct, node_hits=node_hits, kmers=res["kmers"], ties=int(v[-1]), m=m)
        if dist.rank_world()[0] == 0:
            records = int(direct.sum())
            print("classify_reads: M=%d\trecords %d\tclassified %d\tfrom a tie %d" % (m, records, records - int(direct[0]), int(v[-1])),
                  file=sys.stderr)
            sys.stderr.flush()
        _write_tagged_bams(kdb, row_node, parent, m, node_ids, paths)
        _write_read_calls(kdb, row_node, parent, m, node_ids, paths)


def write_read_classes(out_dir, scope=None):
    """out_dir/read_classes.tsv from the numbers collected under `scope`; nothing without the flag, without numbers, or after a skip."""
    r = CLASSIFY_READS["rows"].get(scope)
    if not CLASSIFY_READS["m"] or CLASSIFY_READS["skipped"] is not None or not r:
        return None
    return _write(out_dir, READ_CLASSES_FILE, read_classes_text(r["node_ids"], r["parent_of"], r["leaves"], r["direct"], r["node_hits"], r["kmers"]))


# --tag_bam (StrainScan.apply_tag_bam turns it on; it needs --classify_reads M and BAM input): which read went where.  A resident
# set keeps no map back to file order, a BAM needs none: _lib.bam_tag_file inflates input file i once more, classifies its records
# (with --pairs: its fragments) against the same table with the same row_node, parent and M, and writes `dir`/classified_<i>.bam --
# every record of the input in file order, each kept one with sn:i:<node id of read_classes.tsv, -1 for unclassified> and
# sc:i:<score> behind its last tag (tests/bam_tag_model.py restates it).  Written behind read_classes.tsv's numbers, once per scope;
# "dir" is the output directory where database_scope names none.  Whatever keeps a file from being written says one line and takes
# the files of this run with it; the exit status and every other file stay as they are.
TAG_BAM = {"on": False, "dir": None, "skipped": None, "files": []}
TAG_BAM_TAGS = b"snsc"


def tag_bam_reset(on=False, out_dir=None):
    TAG_BAM.update(on=bool(on), dir=out_dir, skipped=None, files=[])


def _tag_bam_skip(why):
    for f in TAG_BAM["files"]:
        with contextlib.suppress(OSError):
            os.remove(f)
    TAG_BAM["files"] = []
    _skip(TAG_BAM, "tag_bam", "and no tagged BAM was written", True, why)


def _write_tagged_bams(kdb, row_node, parent, m, node_ids, paths):
    """classified_<i>.bam for input file i of `paths`, and one line per file on stderr whose numbers are read_classes.tsv's: tagged -
    classified = the unclassified row's reads_direct, the histogram of sn its reads_direct column (summed over the files)."""
    if not TAG_BAM["on"] or TAG_BAM["skipped"] is not None:
        return
    if dist.is_distributed():
        return _tag_bam_skip("runs on one rank only (this run has several)")
    ps = [p for p in paths if p]
    if any(_lib.input_kind(p) != "bam" for p in ps):
        return _tag_bam_skip("takes BAM inputs (per-read classes of FASTA/FASTQ reads are not written)")
    if any(int(nid) != nid or not -(1 << 31) <= int(nid) < (1 << 31) for nid in node_ids):
        return _tag_bam_skip("needs node ids that fit a 32-bit integer tag (this tree has one outside)")
    node_value = np.array([-1] + [int(nid) for nid in node_ids], np.int32)
    out_dir = TAG_BAM["dir"] or EXTRACT_READS["dir"] or "."
    for i, p in enumerate(ps, 1):
        out = os.path.join(out_dir, "classified_%d.bam" % i)
        try:
            c = _lib.bam_tag_file(p, kdb, row_node, parent, m, node_value, out, pairs=PAIRS["on"], tags=TAG_BAM_TAGS)
        except _lib.BamTagError as e:
            if e.code != _lib.SS_EIO:
                raise
            n = e.counters["already_tagged"]
            if n:
                return _tag_bam_skip("%d records of %s already bear an sn or sc tag (remove them first: samtools view -x sn -x sc)" % (n, p))
            return _tag_bam_skip("%s: %s" % (p, "a read name is not one first and one second mate, or a record's tags are damaged,"
                                             if PAIRS["on"] else "a record's tags are damaged,"))
        TAG_BAM["files"].append(out)
        print("tag_bam: %s\tM=%d\trecords %d\ttagged %d\tclassified %d\tfragments %d\tfrom a tie %d" %
              (out, m, c["records"], c["tagged"], c["classified"], c["fragments"], c["ties"]), file=sys.stderr)
        sys.stderr.flush()


# --read_calls (StrainScan.apply_read_calls turns it on; it needs --classify_reads M and FASTA/FASTQ input): the per-read line of a
# k-mer read classifier -- name, node, score, length and the hit list -- as `dir`/read_calls_<i>.tsv for input file i.  The resident
# set keeps no map back to file order, so the table does not come from it: each file is loaded once more as one slab in FILE ORDER
# (db.ordered_reads: ReadSet.load_ordered per file; with --pairs the two files joined in line order), classified again with
# the row_node, parent and M of read_classes.tsv (ReadSet.calls: classes, scores and the hit lists per record), and the writer walks
# the file a second time and puts the names beside the numbers by position (_lib.read_calls_write; tests/read_calls_model.py restates
# it).  Without --pairs the mates are classified independently, each file on its own.  The ordered sets are cached beside the
# resident reads, so strainscan-multi loads them once for all databases.  Written behind read_classes.tsv's numbers, once per scope;
# whatever keeps a file from being written says one line and takes the files of this run with it; the exit status and every other
# file stay as they are.
READ_CALLS = {"on": False, "dir": None, "skipped": None, "files": []}
READ_CALLS_FILE = "read_calls_%d.tsv"


def read_calls_reset(on=False, out_dir=None):
    READ_CALLS.update(on=bool(on), dir=out_dir, skipped=None, files=[])


def _read_calls_skip(why):
    for f in READ_CALLS["files"]:
        with contextlib.suppress(OSError):
            os.remove(f)
    READ_CALLS["files"] = []
    _skip(READ_CALLS, "read_calls", "and no per-read table was written", True, why)


def _write_read_calls(kdb, row_node, parent, m, node_ids, paths):
    """read_calls_<i>.tsv for input file i of `paths`, and one line per file on stderr: the file, M, its records, those with a
    class, and its records without a sequence."""
    if not READ_CALLS["on"] or READ_CALLS["skipped"] is not None:
        return
    if dist.is_distributed():
        return _read_calls_skip("runs on one rank only (this run has several)")
    ps = [p for p in paths if p]
    if any(_lib.input_kind(p) != "fastx" for p in ps):
        return _read_calls_skip("takes FASTA/FASTQ inputs (a BAM sample's per-read classes are --tag_bam's)")
    if any(int(nid) != nid for nid in node_ids):
        return _read_calls_skip("needs integer node ids (this tree has another)")
    sets, why = db.ordered_reads(paths, PAIRS["on"])
    if sets is None:
        return _read_calls_skip(why)
    node_value = np.array([-1] + [int(nid) for nid in node_ids], np.int64)
    out_dir = READ_CALLS["dir"] or EXTRACT_READS["dir"] or "."
    outs = [os.path.join(out_dir, READ_CALLS_FILE % i) for i in range(1, len(ps) + 1)]
    groups = [(ps, outs, sets[0])] if PAIRS["on"] else [([p], [o], rs) for p, o, rs in zip(ps, outs, sets)]
    for ins, to, rs in groups:
        calls = _select_or_skip(lambda: rs.calls(kdb, row_node, parent, m), _read_calls_skip, "list")
        if calls is None:
            return
        try:
            c = _lib.read_calls_write(ins, to, calls, node_value)
        except _lib.SSError as e:
            if e.code != _lib.SS_EIO:
                raise
            return _read_calls_skip("%s: the records of the file are not those that were loaded (it changed, or it cannot be read or "
                                    "written)" % ins[0])
        READ_CALLS["files"].extend(to)
        per = len(ins)
        for o in to:
            print("read_calls: %s\tM=%d\trecords %d\tclassified %d\tempty %d" %
                  (o, m, c["read"] // per, c["classified"] // per, c["empty"]), file=sys.stderr)      # (--pairs: the empty mates of both files)
        sys.stderr.flush()


# --extract_class LIST (StrainScan.apply_extract_class turns it on; it needs --classify_reads M): the reads of chosen classes of
# read_classes.tsv, written as `dir`/extracted/class_<item>_1.<ext> (and _2 with a second mate) through -x's writer with -x's rules
# -- by content, original text, file order, a pair when either mate is in the class.  An item is `unclassified`, `C<id>` (a leaf
# under its cluster name), `<id>` (any node: its whole clade) or `called` (the clusters the tree walk identifies, each as C<id>).
# The device classifies the sample once and selects every listed clade from the classes it keeps (ReadSet.select_class): the
# call that gives read_classes.tsv its numbers also gives the sets of the listed items (collect_read_classes); `called` is known
# only after the walk and takes a second call (collect_called_classes).  "tree": per scope, what that second call needs; "done":
# the items written under each scope; "files": what this run has written so far (a skip takes them away again).  The output
# directory is EXTRACT_READS["dir"], which database_scope moves per database.
EXTRACT_CLASS = {"items": [], "tree": {}, "done": {}, "skipped": None, "files": []}
EXTRACT_CLASS_UNCLASSIFIED = "unclassified"
EXTRACT_CLASS_CALLED = "called"
_EXTRACT_CLASS_LOCK = threading.Lock()


def extract_class_reset(items=None):
    EXTRACT_CLASS.update(items=list(items or []), tree={}, done={}, skipped=None, files=[])


def parse_class_list(text):
    """--extract_class' value -> its items in order; ValueError for an empty item, an item that is none of `unclassified`,
    `called`, `C<id>` and `<id>` (id: decimal digits without a leading zero), an item listed twice, or more items than one device
    call takes (_lib.CLASS_CLADES_MAX)."""
    import re
    items = str(text).split(",")
    for it in items:
        if not it:
            raise ValueError("an empty item in %r" % (text,))
        if it not in (EXTRACT_CLASS_UNCLASSIFIED, EXTRACT_CLASS_CALLED) and not re.fullmatch(r"C?(0|[1-9][0-9]*)", it):
            raise ValueError("%r is none of unclassified, called, C<id>, <id>" % (it,))
        if items.count(it) > 1:
            raise ValueError("%r is listed twice" % (it,))
    if len(items) > _lib.CLASS_CLADES_MAX:
        raise ValueError("%d items, at most %d are taken" % (len(items), _lib.CLASS_CLADES_MAX))
    return items


def _extract_class_skip(why):
    for f in EXTRACT_CLASS["files"]:
        with contextlib.suppress(OSError):
            os.remove(f)
            os.rmdir(os.path.dirname(f))      # (once it is empty)
    EXTRACT_CLASS["files"] = []
    _skip(EXTRACT_CLASS, "extract_class", "and nothing was extracted", True, why)


def _class_clade(item, num, leaves):
    """The clade (0 = unclassified, v = node v's) that `item` names in a tree with the nodes num = {id: v} and the leaf ids
    `leaves`; None when it names none."""
    if item == EXTRACT_CLASS_UNCLASSIFIED:
        return 0
    nid = int(item[1:] if item.startswith("C") else item)
    if nid not in num or (item.startswith("C") and nid not in leaves):
        return None
    return num[nid]


def _extract_class_wanted(paths, num, leaves):
    """[(item, clade)] for the listed items that name a class of this tree (`called` apart), each other one said on stderr; None
    when --extract_class is off, was skipped, or cannot run on this sample (said once)."""
    if not EXTRACT_CLASS["items"] or EXTRACT_CLASS["skipped"] is not None:
        return None
    if dist.is_distributed():
        return _extract_class_skip("runs on one rank only (this run has several)")
    if any(_lib.input_kind(p) == "bam" for p in paths if p):
        return _extract_class_skip("takes FASTA/FASTQ inputs (BAM subsets per class are not built)")
    done = EXTRACT_CLASS["done"].setdefault(SCOPE["label"], set())
    wanted = []
    for item in EXTRACT_CLASS["items"]:
        if item == EXTRACT_CLASS_CALLED or item in done:
            continue
        clade = _class_clade(item, num, leaves)
        if clade is None:
            print("extract_class: %s names no %s of this database's tree and was not written" %
                  (item, "cluster" if item.startswith("C") else "node"), file=sys.stderr)
            sys.stderr.flush()
        else:
            wanted.append((item, clade))
    return wanted


def _select_classes(rs, kdb, row_node, parent, m, wanted, paths, want_counts=False):
    """One ReadSet.select_class for the clades of `wanted` = [(item, clade)], each set written as extracted/class_<item>_*;
    -> classify()'s numbers of the same call with want_counts."""
    res = rs.select_class(kdb, row_node, parent, m, [c for _, c in wanted], want_counts)
    sets, counts = res if want_counts else (res, None)
    try:
        with _EXTRACT_CLASS_LOCK:
            done = EXTRACT_CLASS["done"].setdefault(SCOPE["label"], set())
            for (item, _), sub in zip(wanted, sets):
                _write_class(item, sub, [p for p in paths if p], m)
                done.add(item)
    finally:
        for sub in sets:
            sub.close()
    return counts


def _write_class(item, sub, ps, m):
    """The set `sub` read back, digested, found in the files `ps` again and written as extracted/class_<item>_<mate>.<ext>
    (-x's writer: _write_selected)."""
    selected = sub.info()["n_records"]
    flat = sub.read_back()
    sub.close()
    keys = _lib.flat_record_keys(flat)
    del flat
    out_dir = os.path.join(EXTRACT_READS["dir"] or ".", EXTRACT_READS_DIR)
    os.makedirs(out_dir, exist_ok=True)
    outs = [os.path.join(out_dir, "class_%s_%d.%s" % (item, i + 1, fastx_record_type(p))) for i, p in enumerate(ps)]
    c = _extract_write(ps, keys, outs)
    EXTRACT_CLASS["files"].extend(outs)
    print("extract_class: %s\tM=%d\tselected on the device %d\twritten %d" % (item, m, selected, c["written"]), file=sys.stderr)
    sys.stderr.flush()


def collect_called_classes(cluster_ids, tree_db_dir, upper_keys, paths):
    """--extract_class called, once the tree walk has identified the clusters `cluster_ids`: extracted/class_C<id>_* for each
    that is not written yet under the current scope, from a second ReadSet.select_class against the cached tree image.  A no-op
    unless `called` is listed and the scope's reads were classified."""
    if EXTRACT_CLASS_CALLED not in EXTRACT_CLASS["items"] or EXTRACT_CLASS["skipped"] is not None or not _pairs_gate(paths):
        return
    t = EXTRACT_CLASS["tree"].get(SCOPE["label"])
    if t is None:
        return
    done = EXTRACT_CLASS["done"].setdefault(SCOPE["label"], set())
    wanted = []
    for cid in sorted(cluster_ids):
        item = "C%s" % cid
        clade = _class_clade(item, t["num"], t["leaves"])
        if clade is not None and item not in done:
            wanted.append((item, clade))
    if not cluster_ids:
        print("extract_class: called: no cluster was called and none was written", file=sys.stderr)
        sys.stderr.flush()
    if not wanted:
        return
    rs = _report_reads(paths)
    if rs is None:
        return _extract_class_skip(NEEDS_RESIDENT)
    kdb = db.tree_image(tree_db_dir, upper_keys).kdb
    for i in range(0, len(wanted), _lib.CLASS_CLADES_MAX):      # (more called clusters than a call takes: several calls)
        part = wanted[i:i + _lib.CLASS_CLADES_MAX]
        if _select_or_skip(lambda: _select_classes(rs, kdb, t["row_node"], t["parent"], t["m"], part, paths) or True,
                           _extract_class_skip, "extract") is None:
            return
