"""`strainscan-multi` -- one sample against several databases in one run.

    strainscan-multi -i R1 [-j R2] -d DB1 -d DB2 [-d LABEL=DB3 ...] -o OUT [-k -l -b -e -s -q --read_support -x N --by_strain --bootstrap B --bootstrap_clusters B --classify_reads M --extract_class LIST --tag_bam --read_calls --classify_strains M --extract_strains unique|compatible --em_strains B --divergence M --pairs]

For every database OUT/<label>/ receives the files `strainscan -i R1 [-j R2] -d DBn -o OUT/<label> [flags]` writes, and
OUT/databases.tsv one line per database (command-line order): label, path, status -- `reports`, `no_clusters` (the "No
clusters can be detected" exit), `single_cluster` (layer 2's exit for one single-strain cluster) or `error:<ExceptionType>`.
<label> is the basename of the database directory, or the LABEL= given.

What is shared: the sample is parsed and copied to the device ONCE (db.resident_reads); the tree images of all databases are
resident together (db.pinned_images) and counted in ONE pass over the reads (db.scan_images: ss_scan_reads_multi, every tree
table behind its own Bloom filter); layer 2's cluster tables scan the same resident reads.  Each database then runs the steps
of StrainScan.main unchanged (-b, the cutoff ladder, layer 2), in command-line order.

Exit status: 0 when every database ended the way a single-database run ends, 1 when any raised an error (its traceback is
printed with its label; the databases after it still run), 2 for a command line refused before any read is touched.
"""
import argparse
import os
import sys
import traceback

if __name__ == "__main__" or os.path.basename(sys.argv[0] or "") == "strainscan-multi":
    # (as `strainscan`: the HIP runtime starts on a worker thread while the modules below are imported)
    import threading

    def _early():
        from . import _lib
        n_gz = sum(a.endswith(".gz") or _lib.input_kind(a) == "bam" for a in sys.argv[1:])
        _lib.warm_up(ingest=int(os.environ.get("WORLD_SIZE", "1")) <= 1 and not n_gz, gz=min(n_gz, 2))

    threading.Thread(target=_early, name="ss-gpu-warm-up", daemon=True).start()

from . import StrainScan, Vote_Strain_L2_Lasso_new_sp

usage = "strainscan-multi - one sample against several StrainScan databases in one run (one ingest, one fused tree scan)."
TSV = "databases.tsv"


class Refused(ValueError):
    """A command line refused before any read is touched (exit status 2)."""


def parse_database(arg):
    """`DIR` or `LABEL=DIR` -> (label, dir).  An existing directory is taken as it is even when its name holds '='."""
    if "=" in arg and not os.path.isdir(arg):
        label, path = arg.split("=", 1)
        if not label or "/" in label or label in (".", ".."):
            raise Refused("-d %s: a label is a non-empty name without '/'" % arg)
        if not path:
            raise Refused("-d %s: no database directory after the label" % arg)
        return label, path
    return os.path.basename(os.path.normpath(arg)), arg


def check_databases(dbs):
    """[(label, dir)] -> the same list, or Refused: a database without Tree_database/, two -d of one directory, two equal labels."""
    seen_dir, seen_label = {}, set()
    for label, path in dbs:
        if not os.path.isdir(os.path.join(path, "Tree_database")):
            raise Refused("-d %s: no Tree_database/ in that directory" % path)
        real = os.path.realpath(path)
        if real in seen_dir:
            raise Refused("-d %s and -d %s are the same database directory" % (seen_dir[real], path))
        seen_dir[real] = path
        if label in seen_label:
            raise Refused("two databases are labelled %r (give one of them LABEL=DIR)" % label)
        seen_label.add(label)
    return dbs


def parse_args(argv=None):
    """-> (args, [(label, dir)], settings dict).  Refusals end in SystemExit(2) with a message, before any file is opened."""
    ap = argparse.ArgumentParser(prog="strainscan-multi", description=usage)
    StrainScan.add_arguments(ap, multi=True)
    args = ap.parse_args(argv)
    StrainScan.refuse_by_strain_alone(ap, args)
    StrainScan.refuse_extract_class_alone(ap, args)
    StrainScan.refuse_extract_strains_alone(ap, args)
    StrainScan.refuse_em_strains_alone(ap, args)
    StrainScan.refuse_pairs_alone(ap, args)
    StrainScan.refuse_tag_bam_alone(ap, args)
    StrainScan.refuse_read_calls_alone(ap, args)
    try:
        opts = StrainScan.settings(args)
    except ValueError as e:
        ap.error(str(e))
    if opts["pmode"] in (1, 2):
        ap.error("plasmid / reference-genome mode (-p) needs the reference's database builder and is not supported")
    try:
        dbs = check_databases([parse_database(a) for a in args.db_dir])
    except Refused as e:
        ap.error(str(e))
    return args, dbs, opts


def write_table(path, rows):
    """databases.tsv: label \\t path \\t status, one line per database."""
    with open(path, "w") as f:
        for label, db, status in rows:
            f.write("%s\t%s\t%s\n" % (label, os.path.abspath(db), status))


def read_table(path):
    with open(path) as f:
        return [tuple(line.rstrip("\n").split("\t")) for line in f if line.strip()]


def _image_spec(db_dir):
    """The tree image the walk of this database asks for: identify_low_mem's key convention when <DB>/Memory_DB exists
    (StrainScan.main picks it), identify's otherwise."""
    from . import identify, identify_low_mem
    mdb = os.path.exists(db_dir + "/Memory_DB")
    return db_dir + "/Tree_database", (identify_low_mem if mdb else identify)._UPPER_KEYS


def identify_databases(in_fq, db_dirs, out_dir, ksize=31, ldep=0, sprob=0, emode=0, msn=40, pmode=0, before_each=None, rank=0):
    """in_fq = (fq1, fq2 or ''); db_dirs: [dir or (label, dir)] -> [(label, dir, status)] in that order, also written to
    out_dir/databases.tsv (rank 0).  Database i's reports go to out_dir/<label>.  before_each(i) is called just before
    database i's work (tests seed numpy's RNG there: the walk's Poisson draw is unseeded, as in the reference)."""
    from . import db as dbm, read_reports
    fq1, fq2 = in_fq[0], in_fq[1] or ""
    dbs = [(d if isinstance(d, tuple) else parse_database(d)) for d in db_dirs]
    paths = [p for p in (fq1, fq2) if p]
    rows = []
    with dbm.pinned_images([_image_spec(d) for _, d in dbs], reads=paths) as imgs:
        if not dbm.scan_images([i for i in imgs if i is not None], paths):
            print("strainscan-multi: the reads do not fit the resident budget (SS_READS_RESIDENT_GB): every database scans "
                  "the files itself", file=sys.stderr)
        for i, (label, d) in enumerate(dbs):
            od = os.path.join(out_dir, label)
            os.makedirs(od, exist_ok=True)
            print("== database %s: %s" % (label, d))
            sys.stdout.flush()
            if before_each is not None:
                before_each(i)
            stage = "layer1"
            try:
                with read_reports.database_scope(label, od):      # (this database's rows; -x: OUT/<label>/extracted/)
                    cls_dict, l2 = StrainScan.identify_layer1(fq1, fq2, d, od, ldep, sprob)
                    stage = "layer2"
                    Vote_Strain_L2_Lasso_new_sp.vote_strain_L2_batch(fq1, fq2, d, od, ksize, dict(cls_dict), l2, msn, pmode, emode)
                status = "reports"
            except SystemExit as e:
                if e.code in (None, 0):
                    status = "no_clusters" if stage == "layer1" else "single_cluster"
                else:
                    print("strainscan-multi: database %s (%s) exited with %r" % (label, d, e.code), file=sys.stderr)
                    status = "error:SystemExit"
            except Exception as e:              # noqa: B902 -- recorded; the databases after it still run
                sys.stdout.flush()
                print("strainscan-multi: database %s (%s) failed:" % (label, d), file=sys.stderr)
                traceback.print_exc()
                sys.stderr.flush()
                status = "error:" + type(e).__name__
            finally:
                read_reports.write_all(od, label)       # (OUT/<label>/read_support.tsv, strain_support.tsv, strain_bootstrap.tsv, cluster_bootstrap.tsv, read_classes.tsv, strain_classes.tsv, strain_sets.tsv, strain_em.tsv, strain_divergence.tsv)
            rows.append((label, d, status))
    if rank == 0:
        write_table(os.path.join(out_dir, TSV), rows)
    return rows


def main(argv=None):
    args, dbs, opts = parse_args(argv)
    StrainScan.refuse_cram(args.input_fq, args.input_fq2)         # (reads the sample's first bytes: after the checks above)
    StrainScan.apply_min_base_qual(args.min_base_qual)
    out_dir = StrainScan.output_dir(args.out_dir, os.getcwd())
    os.makedirs(out_dir, exist_ok=True)
    from . import dist, read_reports
    rank, _ = dist.init_from_env()
    out_dir = StrainScan.rank_output_dir(out_dir, rank)
    StrainScan.apply_read_support(args.read_support)
    StrainScan.apply_extract_reads(args.extract_reads)
    StrainScan.apply_by_strain(args.by_strain)
    StrainScan.apply_bootstrap(args.bootstrap, args.bootstrap_seed)
    StrainScan.apply_bootstrap_clusters(args.bootstrap_clusters, args.bootstrap_seed)
    StrainScan.apply_classify_reads(args.classify_reads)
    StrainScan.apply_extract_class(args.extract_class)
    StrainScan.apply_classify_strains(args.classify_strains)      # (OUT/<label>/strain_classes.tsv, strain_sets.tsv, extracted/strain_*)
    StrainScan.apply_extract_strains(args.extract_strains)
    StrainScan.apply_em_strains(args.em_strains, args.bootstrap_seed)      # (OUT/<label>/strain_em.tsv)
    StrainScan.apply_divergence(args.divergence)      # (OUT/<label>/strain_divergence.tsv)
    StrainScan.apply_tag_bam(args.tag_bam)      # (database_scope names each database's directory: OUT/<label>/classified_<i>.bam)
    StrainScan.apply_read_calls(args.read_calls)      # (OUT/<label>/read_calls_<i>.tsv; db.ordered_reads loads the ordered sets once)
    StrainScan.apply_pairs(args.pairs)         # (db.resident_pairs caches the joined set: joined once for all databases)
    try:
        rows = identify_databases((args.input_fq, args.input_fq2 or ""), dbs, out_dir, ksize=opts["ksize"], ldep=opts["ldep"],
                                  sprob=opts["sprob"], emode=opts["emode"], msn=opts["msn"], pmode=opts["pmode"], rank=rank)
    finally:
        read_reports.reset_all()
    return 1 if any(st.startswith("error:") for _, _, st in rows) else 0


def cli():
    StrainScan.cli(main)


if __name__ == "__main__":
    cli()
