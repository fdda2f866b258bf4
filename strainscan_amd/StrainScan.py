"""`strainscan` command line -- drop-in for the identification CLI StrainScan.py:113-271.

Same flags (-i -j -d -o -k -l -b -p -r -e -s), same cutoff ladder, same output files
(final_report.txt, C<id>/StrainVote.report, strain_prob.txt).  Two flags of its own: -q Q masks bases of Phred quality below Q
(`jellyfish count -Q`; off by default); --read_support also writes read_support.tsv (reads that carry each table's k-mers).  Plasmid mode (-p 1/2) rebuilds a
database with the reference's offline builder (StrainScan.py:235) and is out of scope here.
"""
import argparse
import os
import re
import sys

if __name__ == "__main__" or os.path.basename(sys.argv[0] or "") in ("strainscan", "StrainScan.py"):
    # the command itself: the library is loaded and the HIP runtime started on a worker thread (0.15-0.2 s) while this
    # thread imports numpy and the modules below and reads the arguments
    import threading

    def _early():
        from . import _lib
        # (plain-text reads in a single process: the parse threads' pinned buffers too; .gz inputs never use them, they have
        #  upload buffers of their own)
        n_gz = sum(a.endswith(".gz") or _lib.input_kind(a) == "bam" for a in sys.argv[1:])
        _lib.warm_up(ingest=int(os.environ.get("WORLD_SIZE", "1")) <= 1 and not n_gz, gz=min(n_gz, 2))

    threading.Thread(target=_early, name="ss-gpu-warm-up", daemon=True).start()

from . import identify, identify_low_mem, identify_low_depth, Vote_Strain_L2_Lasso_new_sp

usage = "StrainScan - A kmer-based strain-level identification tool (MI355X-native identification path)."


def generate_prob_report(prob_dict, out_dir, db_dir):
    """StrainScan.py:98-111."""
    d = {}
    with open(db_dir + "/hclsMap_95_recls.txt", "r") as f:
        while True:
            line = f.readline().strip()
            if not line:
                break
            ele = line.split("\t")
            d[int(ele[0])] = ele[-1]
    with open(out_dir + "/strain_prob.txt", "w+") as op:
        op.write("Cluster_ID\tProbability\tNumber_of_strains\tStrains_in_the_cluster\n")
        for p in prob_dict:
            st = re.split(",", d[p[0]])
            op.write("C" + str(p[0]) + "\t" + str(p[1]) + "\t" + str(len(st)) + "\t" + d[p[0]] + "\n")


def _l1(mdb, in_fq, tdb, cutoff):
    mod = identify_low_mem if mdb == 1 else identify
    return mod.identify_cluster(in_fq, tdb, cutoff)


# the cutoff ladder of -l (StrainScan.py:192-217): [cov, weighted cov, abundance] per rung; -l 0 takes its second rung when the
# first calls nothing (read_reports.collect_cluster_bootstrap walks the same rungs on resampled counts)
LADDER_CUTOFFS = {0: ([0.1, 0.4, 1], [0.05, 0.05, 1]), 1: ([0.01, 0.05, 1],), 2: ([0.005, 0.01, 1],)}


def identify_with_ladder(in_fq, tdb, ldep, mdb):
    """StrainScan.py:192-217 -> (cls_dict, l2)."""
    if ldep not in LADDER_CUTOFFS:
        raise ValueError("-l must be 0, 1 or 2")
    rungs = LADDER_CUTOFFS[ldep]
    cls_dict = _l1(mdb, in_fq, tdb, list(rungs[0]))
    l2 = 0 if ldep == 0 else 1
    if ldep == 0:
        if len(cls_dict) == 0:
            cls_dict = _l1(mdb, in_fq, tdb, list(rungs[1]))
            l2 = 1
        if len(cls_dict) == 0:
            print("Warning: No clusters can be detected!")
            raise SystemExit
    return cls_dict, l2


def _clock(what):
    """SS_CLI_TRACE=1: seconds since the interpreter started, at the CLI's milestones."""
    from ._lib import cli_clock
    cli_clock(what)


def add_arguments(ap, multi=False):
    """The flags of StrainScan.py:113-148 (multi: -d may be given several times, as `DIR` or `LABEL=DIR`)."""
    ap.add_argument("-i", "--input_fastq", dest="input_fq", type=str, required=True,
                    help="The dir of input fastq data --- Required")
    ap.add_argument("-j", "--input_fastq_2", dest="input_fq2", type=str,
                    help="The dir of input fastq data (for pair-end data).")
    if multi:
        ap.add_argument("-d", "--database_dir", dest="db_dir", type=str, action="append", required=True,
                        help="A database dir, or LABEL=dir; give -d once per database --- Required")
    else:
        ap.add_argument("-d", "--database_dir", dest="db_dir", type=str, required=True,
                        help="The dir of your database --- Required")
    ap.add_argument("-o", "--output_dir", dest="out_dir", type=str,
                    help="Output dir (default: current dir/StrainScan_Result)")
    ap.add_argument("-k", "--kmer_size", dest="ksize", type=str,
                    help="The size of kmer, should be odd number. (default: k=31)")
    ap.add_argument("-l", "--low_dep", dest="ldep", type=str,
                    help='"1" for low depth (< 10x), "2" for super low depth (< 1x) (default: -l 0)')
    ap.add_argument("-b", "--strain_prob", dest="sprob", type=str,
                    help="1: also output the probability of detecting a strain (or cluster) in low-depth samples")
    ap.add_argument("-p", "--plasmid_mode", dest="pmode", type=str,
                    help="plasmid / reference-genome search modes of the reference (not supported here)")
    ap.add_argument("-r", "--ref_genome", dest="rgenome", type=str, help="reference genomes for -p")
    ap.add_argument("-e", "--extraRegion_mode", dest="emode", type=str,
                    help="1: also return strains with extra regions covered (default: -e 0)")
    ap.add_argument("-s", "--minimum_snv_num", dest="msn", type=str,
                    help="The minimum number of SNV at Layer-2 identification. (default: 40)")
    ap.add_argument("-q", "--min_base_qual", dest="min_base_qual", type=min_base_qual_arg, default=0, metavar="Q",
                    help="Mask low-quality bases: a base whose Phred quality is below Q (FASTQ: quality character below "
                         "chr(33+Q), as `jellyfish count -Q`; BAM: qual < Q, records without qualities are left alone) "
                         "becomes N before k-mers are counted; FASTA input is untouched.  An integer in 0..93 "
                         "(default: 0, no masking)")
    ap.add_argument("--read_support", dest="read_support", action="store_true",
                    help="Also write read_support.tsv: for the tree's table and for every cluster table scanned at layer 2, how "
                         "many reads of the sample carry at least 1, 2, 4, ... 64 of its k-mers (needs the sample resident on "
                         "the device and k >= 17)")
    ap.add_argument("-x", "--extract_reads", dest="extract_reads", type=extract_reads_arg, default=0, metavar="N",
                    help="Also write the reads that carry at least N k-mers of a table to OUT/extracted/<table>_1.<ext> (and _2 "
                         "with -j; a pair when either mate does), for the tree's table and every cluster table scanned at "
                         "layer 2.  An integer >= 1; read_support.tsv's geN columns say how many reads a given N keeps.  Needs "
                         "the sample resident on the device, k >= 17 and one rank.  BAM input (every input a BAM; the sample "
                         "need not be resident) gives OUT/extracted/<table>_<i>.bam per input file: a BGZF BAM (zlib level 1) "
                         "with the input's header and, byte for byte and in file order, every record of a template (read name) "
                         "of which one record has N hits -- mates wherever they lie; secondary (0x100) and supplementary "
                         "(0x800) records and records without bases are never written (default: off)")


    ap.add_argument("--by_strain", dest="by_strain", action="store_true",
                    help="With --read_support and/or -x N: attribute reads to the strains called in each multi-strain cluster.  "
                         "A k-mer counts for a called strain when no other called strain of the cluster has it.  Writes "
                         "strain_support.tsv (rows C<id>.<n>, n = the strain's number in C<id>/StrainVote.report) and "
                         "OUT/extracted/C<id>.<n>_1.<ext>; reads that only carry k-mers shared between called strains are in "
                         "C<id>'s files and in no strain's (default: off)")
    ap.add_argument("--bootstrap", dest="bootstrap", type=bootstrap_arg, default=0, metavar="B",
                    help="Also write strain_bootstrap.tsv: for every strain called in a multi-strain cluster, the 2.5 %% and 97.5 %% "
                         "points of its depth and of its share of the cluster over B replicates, and in how many of them it is "
                         "present.  A replicate resamples the reads with replacement on the device (a Poisson bootstrap over reads), "
                         "re-counts the cluster's k-mers and solves again with the called strains and the penalty held fixed: the "
                         "intervals are conditional on both and on the cluster's abundance, mates are resampled independently (as "
                         "one fragment with --pairs) and identical reads together -- a lower bound on the real uncertainty.  An "
                         "integer in 2..1000; needs the "
                         "sample resident on the device and k >= 17 (default: off)")
    ap.add_argument("--bootstrap_seed", dest="bootstrap_seed", type=bootstrap_seed_arg, default=1, metavar="S",
                    help="The seed of --bootstrap's and --bootstrap_clusters' replicates: the same S gives the same files.  An integer in 0..2^63-1 (default: 1)")
    ap.add_argument("--bootstrap_clusters", dest="bootstrap_clusters", type=bootstrap_arg, default=0, metavar="B",
                    help="Also write cluster_bootstrap.tsv: would a second sequencing run have called the same clusters?  The "
                         "reads are resampled B times under the tree walk (a Poisson bootstrap over reads, the replicates of "
                         "--bootstrap_seed S); the counts of all replicates come from one pass per 16 over the resident reads, and "
                         "each is walked with this run's -l ladder.  One row per cluster that the run or any replicate called: in "
                         "how many replicates it is present, and the 2.5 %% and 97.5 %% points of its depth and coverage (0 where "
                         "absent).  Identical reads share a weight, mates are resampled independently (as one fragment with "
                         "--pairs); nothing is said about the strains inside a cluster, which is --bootstrap's job.  An integer in "
                         "2..1000; needs the sample resident on the device, one rank and a database with more than one cluster "
                         "(default: off)")
    ap.add_argument("--classify_reads", dest="classify_reads", type=classify_reads_arg, default=0, metavar="M",
                    help="Also write read_classes.tsv: every read assigned to a node of the cluster search tree.  A read's hits "
                         "against the tree's k-mers point at the nodes that list them; the read goes to the node whose path from the "
                         "root collects the most hits, to the lowest common ancestor where several nodes tie, and to nobody "
                         "(`unclassified`) below M hits on the best path.  One row per node: its k-mers, their hits, the reads "
                         "assigned to it (reads_direct) and to it or anything below it (reads_clade).  An integer >= 1 (1 or 2 "
                         "for the sampled node sets of a tree); needs the sample resident on the device and a database with "
                         "more than one cluster (default: off)")
    ap.add_argument("--extract_class", dest="extract_class", type=extract_class_arg, default=None, metavar="LIST",
                    help="With --classify_reads M: also write the reads of chosen classes of read_classes.tsv to "
                         "OUT/extracted/class_<item>_1.<ext> (and _2 with -j).  LIST is comma-separated, at most 64 items, each one "
                         "of `unclassified`, `C<id>` (a cluster, under the name read_classes.tsv gives it), `<id>` (any node of "
                         "read_classes.tsv: the reads of the node and of everything below it, its reads_clade) and `called` (the "
                         "clusters the tree walk identifies, each as class_C<id>_*).  Written with -x's rules: the original text in "
                         "file order, selected by content, a pair when either mate is in the class -- so a pair under "
                         "`unclassified` has at least one unclassified mate.  Needs FASTA/FASTQ input and one rank (default: off)")
    ap.add_argument("--classify_strains", dest="classify_strains", type=classify_strains_arg, default=0, metavar="M",
                    help="Also write strain_classes.tsv and strain_sets.tsv: every read assigned to the called strains of a "
                         "cluster that explain it best.  After a cluster's StrainVote.report is written, a read's hits against "
                         "the cluster's k-mers vote for every called strain that has the k-mer; the read's set is the strains "
                         "with the most votes -- one strain: a unique assignment, several: a tie -- and empty (`unassigned`) "
                         "below M votes.  strain_classes.tsv has a row per called strain: its k-mers, their hits, the reads "
                         "assigned to it alone (reads_unique), in a tie (reads_tied) and its share when a tied read is split "
                         "evenly (reads_share); strain_sets.tsv has a row per set with reads.  Identical reads share a set, "
                         "mates are assigned independently (as one fragment with --pairs), a strain that is not called gets "
                         "no reads.  An integer >= 1; needs the sample resident on the device, one rank and clusters with at "
                         "most 16 called strains (default: off)")
    ap.add_argument("--extract_strains", dest="extract_strains", choices=("unique", "compatible"), default=None,
                    help="With --classify_strains M: also write the reads of every called strain to "
                         "OUT/extracted/strain_C<id>.<n>_1.<ext> (and _2 with -j) -- `unique`: the reads assigned to the strain "
                         "alone; `compatible`: those whose set holds the strain.  Written with -x's rules: the original text "
                         "in file order, selected by content, a pair when either mate is selected (with --pairs: the "
                         "fragment).  Needs FASTA/FASTQ input (default: off)")
    ap.add_argument("--em_strains", dest="em_strains", type=em_strains_arg, default=None, metavar="B",
                    help="With --classify_strains M: also write strain_em.tsv, the called strains' abundances estimated from the "
                         "reads.  The reads of every set of called strains (strain_sets.tsv) are shared out among the set's strains "
                         "by an EM over these equivalence classes -- a tied read goes to its strains in proportion to their current "
                         "shares, iterated to a fixed point on the device -- which gives each strain its share of the assigned reads "
                         "(frac_reads) and, divided by the strain's k-mers, a depth-like abundance beside the elastic-net fraction "
                         "of StrainVote.report.  B = 0: the estimate alone; B in 2..1000: also its 2.5 %% and 97.5 %% bounds over B "
                         "replicates that resample the reads (a Poisson bootstrap over reads, the replicates of --bootstrap_seed S), "
                         "all replicates solved in one launch.  The bounds are conditional on the called strains, identical reads "
                         "share a weight, a strain that is not called gets no reads (default: off)")
    ap.add_argument("--divergence", dest="divergence", type=divergence_arg, default=0, metavar="M",
                    help="Also write strain_divergence.tsv: how far the sample's organism is from the nearest called strain of "
                         "each multi-strain cluster, from the ORDER of k-mer hits along every read.  After a cluster's "
                         "StrainVote.report is written, a read's windows are C (a k-mer of a called strain), T (a k-mer of the "
                         "cluster that no called strain has) or X (neither); a gap is a run of T/X windows between two C windows "
                         "with no N inside.  One differing base removes k consecutive k-mers (gap_k), a deleted base k - 1 "
                         "(gap_km1), an insertion or two close differences more (gap_k_2k); those are `sites` unless every "
                         "window of the gap is T (gaps_in_cluster: the read follows an uncalled strain).  per_kb = 1000 x sites / "
                         "detectable, detectable being the base positions at which a difference would have made such a gap.  It "
                         "is divergence PLUS the sequencing error rate, relative to the union of the called strains.  Only reads "
                         "with at least M k-mers of the called strains are assessed.  An integer >= 1; needs the sample resident "
                         "on the device, k >= 17 and one rank (default: off)")
    ap.add_argument("--tag_bam", dest="tag_bam", action="store_true",
                    help="With --classify_reads M and BAM input (every input a BAM): also write OUT/classified_<i>.bam per input "
                         "file, the input written back with the class of every read as two aux tags -- sn:i:<node of "
                         "read_classes.tsv, -1 for unclassified> and sc:i:<hits on the best path, reported below M too> behind the "
                         "last tag of every record the loader keeps; secondary (0x100) and supplementary (0x800) records and "
                         "records without bases are copied as they are.  A BGZF BAM (zlib level 1) with the input's header, "
                         "every record in file order; `samtools view -d sn:<id>` gives the reads of one node.  With --pairs "
                         "both mates carry the fragment's class.  A record that already bears sn or sc stops the file (remove "
                         "them with `samtools view -x sn -x sc`).  Needs one rank (default: off)")
    ap.add_argument("--read_calls", dest="read_calls", action="store_true",
                    help="With --classify_reads M and FASTA/FASTQ input: also write OUT/read_calls_<i>.tsv per input file (1 for -i, "
                         "2 for -j), one line per read in file order: name (the header up to the first blank), node (the read's "
                         "class as read_classes.tsv names it, -1 for unclassified), score (the hits on the best path, reported "
                         "below M too), length, and hits (`node:hits` for every node whose k-mers the read carries, ascending by "
                         "node as classified, `-` for none).  A read without a sequence is `name -1 0 0 -`.  Mates are classified "
                         "independently; with --pairs both mates of a pair carry the fragment's node, score and hits.  The files "
                         "are read and classified a second time for this.  Needs one rank and room for another copy of the bases "
                         "on the device; BAM input has --tag_bam (default: off)")
    ap.add_argument("--pairs", dest="pairs", action="store_true",
                    help="With -j (or a paired BAM under -i alone) and at least one of --read_support, -x N, --bootstrap B, "
                         "--classify_reads M: those reports (and "
                         "--by_strain, --extract_class) treat a read PAIR as one fragment -- record i of -i, an N, record i of -j, "
                         "joined on the device into a second resident set.  In a BAM the mates are found by read name and flag "
                         "(0x1, 0x40, 0x80), wherever they lie; a record whose mate is missing, and an unpaired one, is a "
                         "fragment of its own; a name that is not one first and one second mate stops the join.  "
                         "No k-mer spans the joint, so every kmers and hits "
                         "column stays what it is without the flag; `reads` counts pairs, a fragment's hits are both mates' added "
                         "up, a pair is classified, extracted and resampled as a whole.  The files, headers and columns are "
                         "unchanged; stdout and the identification reports do not depend on the flag.  Needs two FASTA/FASTQ files "
                         "or one BAM (--extract_class: FASTA/FASTQ only), "
                         "one rank and room for a second copy of the bases on the device; where the pairs cannot be joined, one "
                         "line says why and no per-read report is written (default: off)")


def refuse_pairs_alone(ap, args):
    """--pairs without -j has no pairs -- unless -i is a BAM, which holds both mates -- and without a per-read report nothing to
    apply them to: the parser's error (exit status 2; only the first bytes of -i are looked at)."""
    from . import _lib
    if args.pairs and not args.input_fq2 and _lib.input_kind(args.input_fq) != "bam":
        ap.error("--pairs needs -j (the second file of the pairs)")
    if args.pairs and not (args.read_support or args.extract_reads or args.bootstrap or args.classify_reads or args.bootstrap_clusters
                           or args.classify_strains or args.divergence):
        ap.error("--pairs needs at least one of --read_support, -x N, --bootstrap B, --classify_reads M, --bootstrap_clusters B")


def refuse_extract_class_alone(ap, args):
    """--extract_class without --classify_reads has no classes to take reads from: the parser's error (exit status 2, before any
    input is opened)."""
    if args.extract_class and not args.classify_reads:
        ap.error("--extract_class needs --classify_reads M")


def refuse_extract_strains_alone(ap, args):
    """--extract_strains without --classify_strains has no sets to take reads from: the parser's error (exit status 2, before any
    input is opened)."""
    if args.extract_strains and not args.classify_strains:
        ap.error("--extract_strains needs --classify_strains M")


def refuse_em_strains_alone(ap, args):
    """--em_strains without --classify_strains has no equivalence classes to start from: the parser's error (exit status 2, before
    any input is opened)."""
    if args.em_strains is not None and not args.classify_strains:
        ap.error("--em_strains needs --classify_strains M")


def refuse_tag_bam_alone(ap, args):
    """--tag_bam without --classify_reads has no classes to write, and tags go into BAM records only: the parser's error (exit
    status 2; only the first bytes of the inputs are looked at, no read is touched)."""
    if not args.tag_bam:
        return
    from . import _lib
    if not args.classify_reads:
        ap.error("--tag_bam needs --classify_reads M")
    for p in (args.input_fq, args.input_fq2):
        if p and _lib.input_kind(p) != "bam":
            ap.error("--tag_bam needs BAM input, %s is not a BAM (per-read classes of FASTA/FASTQ reads are not written)" % p)


def refuse_read_calls_alone(ap, args):
    """--read_calls without --classify_reads has no classes to write, and a BAM sample's per-read classes are --tag_bam's: the
    parser's error (exit status 2; only the first bytes of the inputs are looked at, and only once --classify_reads is there)."""
    if not args.read_calls:
        return
    if not args.classify_reads:
        ap.error("--read_calls needs --classify_reads M")
    from . import _lib
    for p in (args.input_fq, args.input_fq2):
        if p and _lib.input_kind(p) in ("bam", "cram"):
            ap.error("--read_calls takes FASTA/FASTQ input, %s is a BAM or CRAM (--tag_bam writes a BAM sample's per-read classes)" % p)


def refuse_by_strain_alone(ap, args):
    """--by_strain without --read_support or -x has nothing to write: the parser's error (exit status 2, before any input is
    opened)."""
    if args.by_strain and not (args.read_support or args.extract_reads):
        ap.error("--by_strain needs --read_support and/or -x N")


def min_base_qual_arg(text):
    """-q's value: an integer in 0..93, or the parser's error (exit status 2, before any input is opened)."""
    try:
        q = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not an integer in 0..93" % text)
    if not 0 <= q <= 93:
        raise argparse.ArgumentTypeError("%d is outside 0..93" % q)
    return q


def extract_reads_arg(text):
    """-x's value: an integer of at least 1, or the parser's error (exit status 2, before any input is opened)."""
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not an integer >= 1" % text)
    if n < 1 or n > 0xFFFFFFFF:
        raise argparse.ArgumentTypeError("%d is outside 1..%d" % (n, 0xFFFFFFFF))
    return n


def classify_reads_arg(text):
    """--classify_reads' value: an integer of at least 1, or the parser's error (exit status 2, before any input is opened)."""
    try:
        m = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not an integer >= 1" % text)
    if m < 1 or m > 0xFFFFFFFF:
        raise argparse.ArgumentTypeError("%d is outside 1..%d" % (m, 0xFFFFFFFF))
    return m


def classify_strains_arg(text):
    """--classify_strains' value: an integer of at least 1, or the parser's error (exit status 2, before any input is opened)."""
    return classify_reads_arg(text)


def divergence_arg(text):
    """--divergence's value: an integer of at least 1, or the parser's error (exit status 2, before any input is opened)."""
    return classify_reads_arg(text)


def extract_class_arg(text):
    """--extract_class' value: the items of the list (read_reports.parse_class_list), or the parser's error (exit status 2, before
    any input is opened)."""
    from . import read_reports
    try:
        return read_reports.parse_class_list(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def bootstrap_arg(text):
    """--bootstrap's value: an integer in 2..1000, or the parser's error (exit status 2, before any input is opened)."""
    try:
        b = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not an integer in 2..1000" % text)
    if not 2 <= b <= 1000:
        raise argparse.ArgumentTypeError("%d is outside 2..1000" % b)
    return b


def em_strains_arg(text):
    """--em_strains' value: 0 (the estimate alone) or an integer in 2..1000 (replicates), or the parser's error (exit status 2,
    before any input is opened)."""
    try:
        b = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not 0 or an integer in 2..1000" % text)
    if b != 0 and not 2 <= b <= 1000:
        raise argparse.ArgumentTypeError("%d is neither 0 nor in 2..1000" % b)
    return b


def bootstrap_seed_arg(text):
    """--bootstrap_seed's value: an integer in 0..2^63-1, or the parser's error (exit status 2, before any input is opened)."""
    try:
        s = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not an integer in 0..2^63-1" % text)
    if not 0 <= s <= (1 << 63) - 1:
        raise argparse.ArgumentTypeError("%d is outside 0..2^63-1" % s)
    return s


def apply_min_base_qual(q):
    """-q Q: the process-wide threshold (strainscan_amd.set_min_base_qual); the load of the sample then writes ONE line to stderr
    (db.resident_reads: the threshold, bases masked / bases read and, if any, the BAM records that carried no qualities).
    stdout and the report files are untouched."""
    from . import _lib, db
    _lib.set_min_base_qual(q)               # (0 as well: the command line states the setting of its run)
    db.MASK_REPORT.update(on=bool(q), done=False)


def apply_read_support(on):
    """--read_support (strainscan_amd.set_read_support): the tables scanned from here on leave a row each with read_reports.READ_SUPPORT;
    the command writes them to read_support.tsv when it ends.  stdout and the other report files are untouched."""
    from . import read_reports
    read_reports.read_support_reset(on)


def apply_extract_reads(n, out_dir=None):
    """-x N (strainscan_amd.set_extract_reads): the tables scanned from here on leave their reads in out_dir/extracted/
    (read_reports.collect_extract_reads).  stdout and the report files are untouched; 0 turns it off."""
    from . import read_reports
    read_reports.extract_reads_reset(n, out_dir)


def apply_by_strain(on):
    """--by_strain (strainscan_amd.set_by_strain): the multi-strain clusters solved from here on attribute their reads to the called
    strains (read_reports.collect_by_strain).  stdout, the reports, read_support.tsv and extracted/C<id>_* are untouched."""
    from . import read_reports
    read_reports.by_strain_reset(on)


def apply_bootstrap(b, seed=1):
    """--bootstrap B --bootstrap_seed S (strainscan_amd.set_bootstrap): the multi-strain clusters solved from here on are solved
    B more times on resampled reads (read_reports.collect_bootstrap); the command writes strain_bootstrap.tsv when it ends.  stdout and
    the other files are untouched; 0 turns it off."""
    from . import read_reports
    read_reports.bootstrap_reset(b, seed)


def apply_bootstrap_clusters(b, seed=1):
    """--bootstrap_clusters B --bootstrap_seed S (strainscan_amd.set_bootstrap_clusters): the tree walks from here on are run B
    more times on the counts of resampled reads (read_reports.collect_cluster_bootstrap); the command writes
    cluster_bootstrap.tsv when it ends.  stdout and the other files are untouched; 0 turns it off."""
    from . import read_reports
    read_reports.cluster_bootstrap_reset(b, seed)


def apply_classify_reads(m):
    """--classify_reads M (strainscan_amd.set_classify_reads): the tree scans from here on assign every read to a node of the tree
    (read_reports.collect_read_classes); the command writes read_classes.tsv when it ends.  stdout and the other files are
    untouched; 0 turns it off."""
    from . import read_reports
    read_reports.classify_reads_reset(m)


def apply_extract_class(items):
    """--extract_class LIST (strainscan_amd.set_extract_class): the tree scans from here on, which classify the reads, also write
    the reads of the listed classes beside -x's files (read_reports.collect_read_classes, collect_called_classes).  stdout and the
    other files are untouched; nothing turns it off."""
    from . import read_reports
    read_reports.extract_class_reset(items)


def apply_classify_strains(m):
    """--classify_strains M (strainscan_amd.set_classify_strains): the multi-strain clusters solved from here on assign every read
    to its best called strains (read_reports.collect_strain_classes); the command writes strain_classes.tsv and strain_sets.tsv
    when it ends.  stdout and the other files are untouched; 0 turns it off."""
    from . import read_reports
    read_reports.classify_strains_reset(m)


def apply_extract_strains(mode):
    """--extract_strains unique|compatible (strainscan_amd.set_extract_strains): the clusters that assign their reads also write
    each called strain's reads beside -x's files (read_reports.collect_strain_classes).  stdout and the other files are untouched;
    None turns it off."""
    from . import read_reports
    read_reports.extract_strains_reset(mode)


def apply_em_strains(b, seed=1):
    """--em_strains B --bootstrap_seed S (strainscan_amd.set_em_strains): the clusters that assign their reads (--classify_strains)
    also estimate their called strains' abundances by EM over the sets, with B resampled replicates (read_reports.collect_em_strains);
    the command writes strain_em.tsv when it ends.  stdout and the other files are untouched; None turns it off."""
    from . import read_reports
    read_reports.em_strains_reset(b, seed)


def apply_divergence(m):
    """--divergence M (strainscan_amd.set_divergence): the multi-strain clusters solved from here on walk every read's k-mer hits
    for gaps against the called strains (read_reports.collect_divergence); the command writes strain_divergence.tsv when it ends.
    stdout and the other files are untouched; 0 turns it off."""
    from . import read_reports
    read_reports.divergence_reset(m)


def apply_tag_bam(on, out_dir=None):
    """--tag_bam (strainscan_amd.set_tag_bam): the tree scans from here on, which classify the reads, also write every BAM input
    back as out_dir/classified_<i>.bam with each read's class as tags (read_reports.collect_read_classes).  stdout and the other
    files are untouched."""
    from . import read_reports
    read_reports.tag_bam_reset(on, out_dir)


def apply_read_calls(on, out_dir=None):
    """--read_calls (strainscan_amd.set_read_calls): the tree scans from here on, which classify the reads, also write
    out_dir/read_calls_<i>.tsv for every FASTA/FASTQ input: a line per read with its name, class, score, length and hit list
    (read_reports.collect_read_classes).  stdout and the other files are untouched."""
    from . import read_reports
    read_reports.read_calls_reset(on, out_dir)


def apply_pairs(on):
    """--pairs (strainscan_amd.set_pairs): the per-read reports collected from here on work on the set of joined pairs
    (db.resident_pairs) in the place of the resident reads; the scans do not.  stdout and the identification reports are
    untouched."""
    from . import read_reports
    read_reports.pairs_reset(on)


def settings(args):
    """The parsed flags as StrainScan.py:150-160 reads them: dict(ksize, ldep, sprob, pmode, emode, msn)."""
    return dict(ksize=args.ksize if args.ksize else 31, ldep=int(args.ldep) if args.ldep else 0,
                sprob=int(args.sprob) if args.sprob else 0, pmode=int(args.pmode) if args.pmode else 0,
                emode=int(args.emode) if args.emode else 0, msn=int(args.msn) if args.msn else 40)


def refuse_plasmid_mode(pmode):
    if pmode in (1, 2):
        print("Warning: plasmid / reference-genome mode (-p) needs the reference's database builder "
              "(StrainScan.py:235) and is not part of this identification path.")
        raise SystemExit(2)


def refuse_cram(*paths):
    """A CRAM sample is refused (it is not decoded, and never parsed as text): the message, then exit status 2."""
    from . import _lib
    try:
        _lib.refuse_cram(paths)
    except ValueError as e:
        print("Error: %s" % e, file=sys.stderr)
        raise SystemExit(2)


def output_dir(out_dir, pwd):
    """-o as StrainScan.py:162-165 reads it."""
    out_dir = out_dir if out_dir else pwd + "/StrainScan_Result"
    if not re.search("/", out_dir):
        out_dir = pwd + "/" + out_dir
    return out_dir


def identify_database(fq_dir, fq2, db_dir, out_dir, ksize, ldep, sprob, pmode, emode, msn):
    """One database's work once the flags are read (StrainScan.py:186-271): -b, the cutoff ladder, layer 2.  Ends in
    SystemExit where the reference exits (no cluster detected; one single-strain cluster)."""
    cls_dict, l2 = identify_layer1(fq_dir, fq2, db_dir, out_dir, ldep, sprob)
    Vote_Strain_L2_Lasso_new_sp.vote_strain_L2_batch(fq_dir, fq2, db_dir, out_dir, ksize, dict(cls_dict), l2, msn,
                                                     pmode, emode)


def identify_layer1(fq_dir, fq2, db_dir, out_dir, ldep, sprob):
    """-b and the cutoff ladder (StrainScan.py:186-227) -> (cls_dict, l2); SystemExit when no cluster is detected."""
    in_fq = (fq_dir, fq2)
    tdb = db_dir + "/Tree_database"
    if sprob == 1:
        prob = identify_low_depth.identify_ranks(in_fq, tdb)
        generate_prob_report(prob, out_dir, tdb)
    mdb = 1 if os.path.exists(db_dir + "/Memory_DB") else 0
    _clock("arguments read")
    cls_dict, l2 = identify_with_ladder(in_fq, tdb, ldep, mdb)
    _clock("clusters identified")
    print(cls_dict)
    from . import read_reports
    read_reports.collect_called_classes(list(cls_dict), tdb, (identify_low_mem if mdb else identify)._UPPER_KEYS,
                                        [p for p in in_fq if p])      # (--extract_class called)
    read_reports.collect_cluster_bootstrap(cls_dict, tdb, ldep, mdb, [p for p in in_fq if p])      # (--bootstrap_clusters: the main result is final)
    if len(cls_dict) == 0:
        print("Warning: No clusters can be detected!")
        raise SystemExit
    return cls_dict, l2


def rank_output_dir(out_dir, rank):
    """Every rank computes; rank 0 owns the output directory, the others write their reports to scratch."""
    if rank == 0:
        return out_dir
    import atexit
    import shutil
    import tempfile
    out_dir = tempfile.mkdtemp(prefix="strainscan_rank%d_" % rank)
    atexit.register(shutil.rmtree, out_dir, True)      # the other ranks' reports are scratch
    return out_dir


def main(argv=None):
    _clock("main() entered")
    pwd = os.getcwd()
    ap = argparse.ArgumentParser(prog="StrainScan.py", description=usage)
    add_arguments(ap)
    args = ap.parse_args(argv)
    refuse_by_strain_alone(ap, args)
    refuse_extract_class_alone(ap, args)
    refuse_extract_strains_alone(ap, args)
    refuse_em_strains_alone(ap, args)
    refuse_pairs_alone(ap, args)
    refuse_tag_bam_alone(ap, args)
    refuse_read_calls_alone(ap, args)

    fq_dir = args.input_fq
    fq2 = args.input_fq2 or ""
    db_dir = args.db_dir
    opts = settings(args)
    refuse_plasmid_mode(opts["pmode"])
    refuse_cram(fq_dir, fq2)
    apply_min_base_qual(args.min_base_qual)
    out_dir = output_dir(args.out_dir, pwd)
    os.makedirs(out_dir, exist_ok=True)     # (exist_ok: under torchrun every rank arrives here with the same -o at the same moment)

    from . import dist
    rank, world = dist.init_from_env()      # torchrun: one process per GPU, reads shard across ranks
    out_dir = rank_output_dir(out_dir, rank)
    apply_read_support(args.read_support)
    apply_extract_reads(args.extract_reads, out_dir)
    apply_by_strain(args.by_strain)
    apply_bootstrap(args.bootstrap, args.bootstrap_seed)
    apply_bootstrap_clusters(args.bootstrap_clusters, args.bootstrap_seed)
    apply_classify_reads(args.classify_reads)
    apply_extract_class(args.extract_class)
    apply_classify_strains(args.classify_strains)
    apply_extract_strains(args.extract_strains)
    apply_em_strains(args.em_strains, args.bootstrap_seed)
    apply_divergence(args.divergence)
    apply_tag_bam(args.tag_bam, out_dir)
    apply_read_calls(args.read_calls, out_dir)
    apply_pairs(args.pairs)
    try:
        identify_database(fq_dir, fq2, db_dir, out_dir, **opts)
    finally:
        from . import read_reports
        read_reports.write_all(out_dir)     # (in a finally: the reference's own early exit()s come through here as SystemExit)
        read_reports.reset_all()


def cli(main_fn=None):
    """Entry of the `strainscan` command (pyproject.toml, bin/strainscan, python -m): main(), then the process ENDS -- pending
    cache images are written, the streams flushed, and nothing is torn down piece by piece (unpinning the parse buffers,
    freeing GBs of device memory and joining the thread pools cost a fresh process 0.1 s of its 0.65 s; the driver reclaims
    everything at once).  (main_fn: another command's main, strainscan-multi's)"""
    try:
        rc = (main_fn or main)()
    except SystemExit as e:
        rc = e.code
    _clock("reports written")
    try:
        from . import db
        db.report_mask()                    # (-q and reads that were never resident: the line comes here, over all passes)
    except Exception:                       # noqa: B902
        pass
    try:
        from . import db
        db.wait_cache_writes()
    except Exception:                       # noqa: B902
        pass
    if rc is not None and not isinstance(rc, int):      # sys.exit("message"): the message goes to stderr, the code is 1
        print(rc, file=sys.stderr)
        rc = 1
    sys.stdout.flush()
    sys.stderr.flush()
    # several ranks: the ordinary way out (process group, RCCL); SS_FAST_EXIT=0: the ordinary way out for one rank as well
    # (atexit handlers, logging shutdown, temporary files of the caller's own)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("SS_FAST_EXIT", "1") == "0":
        sys.exit(rc)
    import logging
    logging.shutdown()
    os._exit(rc or 0)


if __name__ == "__main__":
    cli()
