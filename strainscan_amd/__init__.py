"""strainscan_amd -- MI355X-native identification path of StrainScan.

The compute lives in hand-written gfx950 HIP kernels behind a C ABI
(include/strainscan_hip.h, strainscan_amd/lib/libstrainscan_hip.so); this package is the
host-side mirror of the reference's Python interface for that path:

    strainscan_amd.identify.identify_cluster                  (library/identify.py:402)
    strainscan_amd.identify_low_mem.identify_cluster          (library/identify_low_mem.py)
    strainscan_amd.identify_low_depth.identify_ranks          (library/identify_low_depth.py:104)
    strainscan_amd.Vote_Strain_L2_Lasso_new_sp.vote_strain_L2_batch   (library/Vote_...:247)
    strainscan_amd.identify_strains_L2_Enet_Pscan_new_sp.detect_strains  (library/identify_strains...:177)
    strainscan_amd.seqpy.revcomp                              (library/seqpy.c:24)
    strainscan_amd.StrainScan.main                            (StrainScan.py:113, the `strainscan` CLI)

    strainscan_amd.set_min_base_qual / get_min_base_qual      (the base-quality mask of `strainscan -q`; process-wide, off by default)
    strainscan_amd.set_read_support                           (`strainscan --read_support`: rows of reads per table, read_reports.READ_SUPPORT)
    strainscan_amd.set_extract_reads                          (`strainscan -x N`: the reads behind each table, read_reports.EXTRACT_READS)
    strainscan_amd.set_by_strain                              (`strainscan --by_strain`: both of the above per called strain, read_reports.BY_STRAIN)
    strainscan_amd.set_bootstrap                              (`strainscan --bootstrap B`: strain depth intervals from resampled reads, read_reports.BOOTSTRAP)
    strainscan_amd.set_bootstrap_clusters                     (`strainscan --bootstrap_clusters B`: the tree walk on resampled reads, read_reports.CLUSTER_BOOTSTRAP)
    strainscan_amd.set_classify_reads                         (`strainscan --classify_reads M`: reads per node of the cluster tree, read_reports.CLASSIFY_READS)
    strainscan_amd.set_extract_class                          (`strainscan --extract_class LIST`: the reads of chosen classes, read_reports.EXTRACT_CLASS)
    strainscan_amd.set_tag_bam                                (`strainscan --tag_bam`: a BAM sample written back with each read's class as tags, read_reports.TAG_BAM)
    strainscan_amd.set_read_calls                             (`strainscan --read_calls`: a line per read with its name, class, score and hit list, read_reports.READ_CALLS)
    strainscan_amd.set_classify_strains                       (`strainscan --classify_strains M`: every read assigned to its best called strains, read_reports.CLASSIFY_STRAINS)
    strainscan_amd.set_extract_strains                        (`strainscan --extract_strains unique|compatible`: the reads of each called strain, read_reports.EXTRACT_STRAINS)
    strainscan_amd.set_em_strains                             (`strainscan --em_strains B`: the called strains' read-based abundances by EM, read_reports.EM_STRAINS)
    strainscan_amd.set_divergence                             (`strainscan --divergence M`: k-mer gaps per read against the called strains, read_reports.DIVERGENCE)
    strainscan_amd.set_pairs                                  (`strainscan --pairs`: those reports on read pairs as fragments, read_reports.PAIRS)

There is no CPU fallback: every entry point raises if the HIP library or a GPU is missing.
"""
__version__ = "0.1.0"


def set_min_base_qual(q):
    """Every later load of reads in this process turns a base whose Phred quality is below `q` into N before any k-mer is
    formed (FASTQ: as `jellyfish count -Q chr(33 + q)`; BAM: qual[i] < q, records without qualities untouched; FASTA
    untouched).  An integer in 0..93; 0 = off, the default.  The reference signatures (identify_cluster(fq_path, db_dir,
    cutoff), ...) stay as they are: this is the one setting they read."""
    from . import _lib
    _lib.set_min_base_qual(q)


def set_read_support(on):
    """`strainscan --read_support` for callers of the functions above: from here on the tree scan of identify_cluster and the
    cluster scans of vote_strain_L2_batch each leave a row in strainscan_amd.read_reports.READ_SUPPORT["rows"][None] -- (table, distinct
    k-mers, reads, hits, 65-bin histogram of hits per read) -- and read_reports.write_read_support(out_dir) writes them as
    read_support.tsv.  set_read_support(False) turns it off and drops the rows.  Off by default; nothing runs while it is off."""
    from . import read_reports
    read_reports.read_support_reset(bool(on))


def set_extract_reads(n, out_dir=None):
    """`strainscan -x N` for callers of the functions above: from here on the tree scan of identify_cluster and the cluster
    scans of vote_strain_L2_batch each write the reads with at least `n` k-mer hits against their table to
    out_dir/extracted/<table>_1.<ext> (and _2 for a pair, written when either mate has them); out_dir defaults to the current
    directory.  n is an integer of at least 1; 0 (or None) turns it off.  Off by default; nothing runs while it is off."""
    if n and (isinstance(n, bool) or not isinstance(n, int) or n < 1):
        raise ValueError("extract_reads must be an integer >= 1 (or 0 for off), not %r" % (n,))
    from . import read_reports
    read_reports.extract_reads_reset(n or 0, out_dir)


def set_by_strain(on):
    """`strainscan --by_strain` for callers of the functions above: from here on vote_strain_L2_batch, after a multi-strain
    cluster has written its StrainVote.report, attributes reads to the called strains -- with set_read_support on, rows for
    read_reports.write_strain_support(out_dir) (strain_support.tsv); with set_extract_reads on, extracted/C<id>.<n>_1.<ext>.  A k-mer
    counts for a called strain when no other called strain of the cluster has it.  Off by default; nothing runs while it is
    off, or while both of the other two are off."""
    from . import read_reports
    read_reports.by_strain_reset(bool(on))


def set_bootstrap(b, seed=1):
    """`strainscan --bootstrap B --bootstrap_seed S` for callers of the functions above: from here on vote_strain_L2_batch, after
    a multi-strain cluster has written its StrainVote.report, solves the cluster `b` more times, each on the reads resampled with
    replacement on the device (ReadSet.resample(seed, replicate)), with the called strains and the penalty of the main solve held
    fixed.  read_reports.bootstrap_replicates() returns the replicate coefficients, read_reports.write_bootstrap(out_dir) writes
    strain_bootstrap.tsv.
    b is an integer in 2..1000 (0 or None turns it off), seed an integer in 0..2^63-1.  Off by default; nothing runs while it is
    off."""
    if b and (isinstance(b, bool) or not isinstance(b, int) or not 2 <= b <= 1000):
        raise ValueError("bootstrap must be an integer in 2..1000 (or 0 for off), not %r" % (b,))
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed <= (1 << 63) - 1:
        raise ValueError("bootstrap seed must be an integer in 0..2^63-1, not %r" % (seed,))
    from . import read_reports
    read_reports.bootstrap_reset(b or 0, seed)


def set_bootstrap_clusters(b, seed=1):
    """`strainscan --bootstrap_clusters B --bootstrap_seed S` for callers of the functions above: from here on
    StrainScan.identify_layer1, once the tree walk has returned, takes the counts of the tree's table under `b` replicates of the
    resident reads (ReadSet.scan_resampled: one pass per 16 replicates, nothing is materialised) and walks each with the run's
    cutoff ladder.  read_reports.cluster_bootstrap_replicates() returns the replicates' {leaf id: (cls_ab, cls_cov)},
    read_reports.write_cluster_bootstrap(out_dir) writes cluster_bootstrap.tsv.
    b is an integer in 2..1000 (0 or None turns it off), seed an integer in 0..2^63-1.  Off by default; nothing runs while it is
    off."""
    if b and (isinstance(b, bool) or not isinstance(b, int) or not 2 <= b <= 1000):
        raise ValueError("bootstrap_clusters must be an integer in 2..1000 (or 0 for off), not %r" % (b,))
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed <= (1 << 63) - 1:
        raise ValueError("bootstrap seed must be an integer in 0..2^63-1, not %r" % (seed,))
    from . import read_reports
    read_reports.cluster_bootstrap_reset(b or 0, seed)


def set_classify_reads(m):
    """`strainscan --classify_reads M` for callers of the functions above: from here on identify_cluster, behind its scan of the
    tree's table, assigns every read of the sample to a node of the cluster search tree (ReadSet.classify: the node whose path from
    the root collects the most of the read's k-mer hits, the lowest common ancestor on a tie, nobody below m hits) and keeps the
    numbers with read_reports.CLASSIFY_READS; read_reports.write_read_classes(out_dir) writes read_classes.tsv.
    m is an integer >= 1 (0 or None turns it off).  Off by default; nothing runs while it is off."""
    if m and (isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= 0xFFFFFFFF):
        raise ValueError("classify_reads must be an integer >= 1 (or 0 for off), not %r" % (m,))
    from . import read_reports
    read_reports.classify_reads_reset(m or 0)


def set_extract_class(names, out_dir=None):
    """`strainscan --extract_class LIST` for callers of the functions above, with set_classify_reads on: from here on
    identify_cluster, where it classifies the reads, also writes the reads of the listed classes to
    out_dir/extracted/class_<item>_1.<ext> (and _2 for a pair, written when either mate is in the class); out_dir defaults to the
    directory of set_extract_reads, then to the current one.  names: a list (or the command's comma-separated text) of
    `unclassified`, `C<id>`, `<id>` and `called`; `called` is written by StrainScan.identify_layer1, which knows the called
    clusters.  None or an empty list turns it off.  Off by default; nothing runs while it is off."""
    from . import read_reports
    items = read_reports.parse_class_list(names if isinstance(names, str) else ",".join(str(n) for n in names)) if names else []
    read_reports.extract_class_reset(items)
    if out_dir is not None:
        read_reports.EXTRACT_READS["dir"] = out_dir


def set_tag_bam(on, out_dir=None):
    """`strainscan --tag_bam` for callers of the functions above, with set_classify_reads on and a sample of BAM files: from here on
    identify_cluster, where it classifies the reads, also writes input file i back as out_dir/classified_<i>.bam -- every record in
    file order, each one the loader keeps with sn:i:<node id of read_classes.tsv, -1 for unclassified> and sc:i:<hits on the best
    path> appended (_lib.bam_tag_file; with set_pairs both mates carry the fragment's class); out_dir defaults to the directory of
    set_extract_reads, then to the current one.  Where no file can be written (FASTA/FASTQ input, several ranks, a record that
    already bears sn or sc) one line on stderr says why.  Off by default; nothing runs while it is off."""
    from . import read_reports
    read_reports.tag_bam_reset(bool(on), out_dir)


def set_read_calls(on, out_dir=None):
    """`strainscan --read_calls` for callers of the functions above, with set_classify_reads on and a sample of FASTA/FASTQ files:
    from here on identify_cluster, where it classifies the reads, also writes out_dir/read_calls_<i>.tsv for input file i -- one line
    per read in file order: name, node (the id read_classes.tsv gives the read's class, -1 for unclassified), score (the hits on
    the best path), length, and the hit list `id:hits ...` of every node whose k-mers the read carries.  Each file is loaded once
    more in file order (ReadSet.load_ordered) and classified again (ReadSet.calls); with set_pairs the two files are joined in line
    order and both mates carry the fragment's numbers.  out_dir defaults to the directory of set_extract_reads, then to the current
    one.  Where no file can be written (BAM input, several ranks, no room on the device, a file that changed) one line on stderr
    says why.  Off by default; nothing runs while it is off."""
    from . import read_reports
    read_reports.read_calls_reset(bool(on), out_dir)


def set_classify_strains(m):
    """`strainscan --classify_strains M` for callers of the functions above: from here on vote_strain_L2_batch, after a multi-strain
    cluster has written its StrainVote.report, assigns every read of the sample to the set of the cluster's called strains with the
    most of the read's k-mer hits (ReadSet.classify_strains: one strain is a unique assignment, several a tie, none below m hits)
    and keeps the numbers with read_reports.CLASSIFY_STRAINS; read_reports.write_strain_classes(out_dir) writes strain_classes.tsv
    and strain_sets.tsv.  A cluster with more than 16 called strains is passed over with one line on stderr.
    m is an integer >= 1 (0 or None turns it off).  Off by default; nothing runs while it is off."""
    if m and (isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= 0xFFFFFFFF):
        raise ValueError("classify_strains must be an integer >= 1 (or 0 for off), not %r" % (m,))
    from . import read_reports
    read_reports.classify_strains_reset(m or 0)


def set_extract_strains(mode, out_dir=None):
    """`strainscan --extract_strains unique|compatible` for callers of the functions above, with set_classify_strains on: every
    cluster that assigns its reads also writes out_dir/extracted/strain_C<id>.<n>_1.<ext> (and _2 for a pair) per called strain --
    "unique": the reads assigned to the strain alone, "compatible": those whose set holds it; out_dir defaults to the directory of
    set_extract_reads, then to the current one.  None turns it off.  Off by default; nothing runs while it is off."""
    from . import read_reports
    if mode is not None and mode not in read_reports.EXTRACT_STRAINS_MODES:
        raise ValueError("extract_strains must be one of %s (or None for off), not %r" % (", ".join(read_reports.EXTRACT_STRAINS_MODES), mode))
    read_reports.extract_strains_reset(mode)
    if out_dir is not None:
        read_reports.EXTRACT_READS["dir"] = out_dir


def set_em_strains(b, seed=1):
    """`strainscan --em_strains B --bootstrap_seed S` for callers of the functions above, with set_classify_strains on: every
    cluster that assigns its reads also shares the reads of its sets out among the called strains by EM (_lib.em_strain_sets; the
    rule is in strainscan_hip.h), on the sample's set counts and on those of b resampled replicates
    (ReadSet.strain_sets_resampled), and keeps the numbers with read_reports.EM_STRAINS; read_reports.write_em_strains(out_dir)
    writes strain_em.tsv, read_reports.em_replicates() hands the matrices over.  b: 0 (the estimate alone) or an integer in
    2..1000; None turns it off.  seed: an integer in 0..2^63-1.  Off by default; nothing runs while it is off."""
    if b is not None and (isinstance(b, bool) or not isinstance(b, int) or not (b == 0 or 2 <= b <= 1000)):
        raise ValueError("em_strains must be 0 or an integer in 2..1000 (or None for off), not %r" % (b,))
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed <= (1 << 63) - 1:
        raise ValueError("seed must be an integer in 0..2^63-1, not %r" % (seed,))
    from . import read_reports
    read_reports.em_strains_reset(b, seed)


def set_divergence(m):
    """`strainscan --divergence M` for callers of the functions above: from here on vote_strain_L2_batch, after a multi-strain
    cluster has written its StrainVote.report, walks the k-mer hits of every read of the sample in order and counts the runs of
    missing k-mers between two k-mers of the cluster's called strains (ReadSet.gaps; the rule is in strainscan_hip.h), over the reads
    with at least m k-mers of the called strains, and keeps the totals with read_reports.DIVERGENCE;
    read_reports.write_divergence(out_dir) writes strain_divergence.tsv.  m is an integer >= 1 (0 or None turns it off).  Off by
    default; nothing runs while it is off."""
    if m and (isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= 0xFFFFFFFF):
        raise ValueError("divergence must be an integer >= 1 (or 0 for off), not %r" % (m,))
    from . import read_reports
    read_reports.divergence_reset(m or 0)


def set_pairs(on):
    """`strainscan --pairs` for callers of the functions above: from here on every per-read report that is on (read support,
    extracted reads, by strain, bootstrap, read classes, extracted classes) works on the sample's read PAIRS -- record i of the
    first file, an N, record i of the second, or the mates of one BAM linked by name and flag, joined on the device
    (db.resident_pairs) -- in the place of its reads; the scans of the identification keep the plain set.  Where the pairs cannot be
    joined (one file that is no BAM, two BAMs, several ranks, no room, unequal record counts, BAM names that are not one first and
    one second mate) one line on stderr says why and those reports write nothing.  Off by default; nothing runs while it is off."""
    from . import read_reports
    read_reports.pairs_reset(bool(on))


def get_min_base_qual():
    from . import _lib
    return _lib.get_min_base_qual()
