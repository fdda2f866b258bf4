"""`strainscan --pairs` / `strainscan-multi --pairs`: with the flag every per-read report is what its model gives on the JOINED records
(record i of -i, an N, record i of -j: tests/pairs_model.py) -- read_support.tsv, strain_support.tsv, the -x and --by_strain files,
read_classes.tsv, the class_* files, strain_bootstrap.tsv -- while stdout and the identification's own reports are those of the
run without it.  The sample is M_mix dealt out as pairs plus CONSTRUCTED pairs that make the flag matter: mates that carry one tree
k-mer of the same leaf each (a class at M = 2 only as a fragment; for two leaves), mates that point at two sibling leaves (the
fragment goes to their parent), a mate of foreign sequence, an empty mate.  Flag off, nothing is joined; where the pairs cannot be joined one line
says why and no per-read report is written."""
import os
import pickle
import re

import numpy as np
import pytest

from tests import bamio, boot_model, label_model, pairs_model as pm, rs_model, select_class_model as scm
from tests import test_bootstrap_cli_gpu as bc
from tests.test_bam_select_gpu import HDR
from tests.test_classify_cli_gpu import model_text
from tests.test_extract_class_cli_gpu import classes_of, tree_model
from tests.test_extract_cli_gpu import DIR, _files, _ok, _result_lines, _run, _with_cache, pair      # noqa: F401
from tests.test_read_support_cli_gpu import _check_tsv

pytestmark = pytest.mark.gpu

M, N, B, SEED = 2, 2, 3, 5
PER_READ = ("read_support.tsv", "strain_support.tsv", "read_classes.tsv", "strain_bootstrap.tsv")


@pytest.fixture(scope="module")
def L():
    from strainscan_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def tm(mid_dbs):
    t = tree_model(mid_dbs["DB_M"]["db_dir"])
    with open(os.path.join(mid_dbs["DB_M"]["db_dir"], "Tree_database", "kmer.fa"), "rb") as f:
        t["kmers"] = [km.upper() for km in rs_model.kmers_of_fasta(f.read())]
    return t


def _rand(rs, n):
    return np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, size=n)].tobytes()


@pytest.fixture(scope="module")
def sample(pair, tm, tmp_path_factory):      # noqa: F811
    """-> dict(paths, recs=[(mate 1 records), (mate 2 records)] as (text, sequence), joined=[fragment], flat=the joined flat block,
    leaf_a, leaf_b, parent: the node ids of two sibling leaves with rows of their own and of their parent; kinds: {name: indices})"""
    rs = np.random.RandomState(41)
    rows_of = {}
    for r, v in enumerate(tm["row_node"].tolist()):
        if v:
            rows_of.setdefault(v, []).append(r)
    by_parent = {}
    for nid in sorted(tm["leaves"]):
        if len(rows_of.get(tm["num"][nid], ())) >= 4 and tm["parent_of"][nid] is not None:
            by_parent.setdefault(tm["parent_of"][nid], []).append(nid)
    par, (leaf_a, leaf_b) = next((p, ls[:2]) for p, ls in sorted(by_parent.items()) if len(ls) >= 2)
    ka, kb = ([tm["kmers"][r] for r in rows_of[tm["num"][nid]][:4]] for nid in (leaf_a, leaf_b))
    seqs = [[s for _, s in pair["recs"][m]] for m in range(2)]
    kinds = {}

    def add(name, m1, m2):
        kinds.setdefault(name, []).append(len(seqs[0]))
        seqs[0].append(m1)
        seqs[1].append(m2)

    def around(kmers, a):
        """the k-mers, an N between them, in random flanks (a bases in front) up to 150 bases: exactly len(kmers) hits -- a flank
        that happens to continue a k-mer into its neighbour in the genome is drawn again"""
        core = b"N".join(kmers)
        while True:
            s = _rand(rs, a) + core + _rand(rs, 150 - len(core) - a)
            if int(rs_model.hits_per_record(s + b"\n", tm["keys"], 31)[0]) == len(kmers):
                return s

    for i in range(30):
        a = 20 + i
        add("same_leaf", around([ka[i % 2]], a), around([ka[2 + i % 2]], 99 - a))
        add("siblings", around([ka[i % 2], ka[2 + i % 2]], a), around([kb[i % 2], kb[2 + i % 2]], a))
        if i < 10:
            add("same_leaf_b", around([kb[i % 2]], a), around([kb[2 + i % 2]], 99 - a))
        add("foreign", seqs[0][7 * i], _rand(rs, 150))
        add("empty_2" if i % 2 else "empty_1", *((seqs[0][11 * i], b"") if i % 2 else (b"", seqs[1][13 * i])))
    qa = np.frombuffer(b"5678ABCDEFGHIJ", np.uint8)
    recs = ([], [])
    for i in range(len(seqs[0])):
        for m in range(2):
            s = seqs[m][i]
            recs[m].append((b"@frag%d/%d\n%s\n+\n%s\n" % (i, m + 1, s, qa[rs.randint(0, qa.size, size=len(s))].tobytes()), s))
    root = tmp_path_factory.mktemp("pairs_sample")
    paths = []
    for m in range(2):
        p = root / ("frag_R%d.fastq" % (m + 1))
        p.write_bytes(b"".join(t for t, _ in recs[m]))
        paths.append(str(p))
    joined = pm.join_lines(seqs[0], seqs[1])
    return dict(paths=paths, recs=recs, joined=joined, flat=b"".join(r + b"\n" for r in joined), kinds=kinds,
                mates=[b"".join(s + b"\n" for s in seqs[m]) for m in range(2)], leaf_a=leaf_a, leaf_b=leaf_b, parent=par)


@pytest.fixture(scope="module")
def items(tm, sample):
    root = next(nid for nid in tm["node_ids"] if tm["parent_of"][nid] is None and nid not in tm["leaves"])
    return ["unclassified", str(root), "C%d" % sample["leaf_a"], "C%d" % sample["leaf_b"], str(sample["parent"])]


@pytest.fixture(scope="module")
def runs(L, mid_dbs, sample, items, tmp_path_factory):
    """`strainscan` with every per-read report on, without and with --pairs -> name: (err, stdout, stderr, out dir, joins made),
    and "spy": layer 2's arguments and the replicates of the run with the flag"""
    from strainscan_amd import StrainScan
    root = tmp_path_factory.mktemp("pairs_cli")
    flags = ["--read_support", "-x", str(N), "--by_strain", "--bootstrap", str(B), "--bootstrap_seed", str(SEED), "--classify_reads", str(M),
             "--extract_class", ",".join(items)]

    def go():
        out = {}
        for name, extra in (("off", []), ("on", ["--pairs"])):
            with bc._Spy() as spy:
                before = L.join_pairs_calls()
                od = str(root / name)
                err, _, text, errs = _run(StrainScan.main, ["-i", sample["paths"][0], "-j", sample["paths"][1], "-d", mid_dbs["DB_M"]["db_dir"],
                                                            "-o", od] + flags + extra)
                out[name] = (err, text, errs, od, L.join_pairs_calls() - before)
            out["spy_" + name] = spy
        return out
    return _with_cache(root, go)


def _tsv(od, name):
    return [ln.split("\t") for ln in open(os.path.join(od, name)).read().split("\n")[1:] if ln]


def test_the_constructed_pairs_make_the_flag_matter(tm, sample):
    """on the model alone: what each kind of pair is as two mates and as a fragment, at M = 2"""
    cls_f = classes_of(tm, sample["flat"], M)
    cls_m = [classes_of(tm, sample["mates"][m], M) for m in range(2)]
    # (the mates' blocks hold empty records, which the models skip: index the non-empty ones)
    at = [np.cumsum([bool(s) for _, s in sample["recs"][m]]) - 1 for m in range(2)]
    a, b, par = (tm["num"][sample[x]] for x in ("leaf_a", "leaf_b", "parent"))
    for i in sample["kinds"]["same_leaf"]:
        assert cls_f[i] == a and cls_m[0][at[0][i]] == 0 and cls_m[1][at[1][i]] == 0
    for i in sample["kinds"]["same_leaf_b"]:
        assert cls_f[i] == b and cls_m[0][at[0][i]] == 0 and cls_m[1][at[1][i]] == 0
    for i in sample["kinds"]["siblings"]:
        assert cls_f[i] == par and cls_m[0][at[0][i]] == a and cls_m[1][at[1][i]] == b
    for i in sample["kinds"]["foreign"]:
        assert cls_m[1][at[1][i]] == 0 and cls_f[i] == cls_m[0][at[0][i]]
    assert sum(1 for i in sample["kinds"]["foreign"] if cls_f[i]) >= 10
    for i in sample["kinds"]["empty_1"]:
        assert not sample["recs"][0][i][1] and sample["joined"][i].startswith(b"N") and cls_f[i] == cls_m[1][at[1][i]]
    for i in sample["kinds"]["empty_2"]:
        assert not sample["recs"][1][i][1] and sample["joined"][i].endswith(b"N") and cls_f[i] == cls_m[0][at[0][i]]
    assert len(cls_f) == len(sample["joined"]) >= 1000


def test_runs_end_alike_and_the_other_files_do_not_depend_on_the_flag(runs):
    e0, t0, errs0, d0, joins0 = runs["off"]
    e1, t1, errs1, d1, joins1 = runs["on"]
    assert _ok(e0) and _ok(e1) and type(e0) is type(e1)
    assert joins0 == 0 and joins1 == 1 and "pairs:" not in errs0
    assert t0 == t1 or _result_lines(t0) == _result_lines(t1)
    assert _result_lines(t0)
    mine = lambda k: os.path.basename(k) in PER_READ or DIR in k.split(os.sep)      # noqa: E731
    a, b = ({k: v for k, v in _files(d).items() if not mine(k)} for d in (d0, d1))
    assert any(k.endswith("StrainVote.report") for k in a) and "final_report.txt" in a
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    # the files, headers and columns are those of the run without the flag
    for name in PER_READ:
        assert open(os.path.join(d0, name)).readline() == open(os.path.join(d1, name)).readline(), name
    assert sorted(os.listdir(os.path.join(d0, DIR))) == sorted(os.listdir(os.path.join(d1, DIR)))
    line = [ln for ln in errs1.split("\n") if ln.startswith("pairs: ")]
    assert len(line) == 1 and re.fullmatch(r"pairs: (\d+) pairs joined\t(\d+) bytes on the device", line[0]), line


def test_read_support_is_the_models_on_fragments(runs, mid_dbs, sample):
    od = runs["on"][3]
    rows = _check_tsv(os.path.join(od, "read_support.tsv"), mid_dbs["DB_M"]["db_dir"], od, sample["flat"])
    off = {r[0]: r for r in _tsv(runs["off"][3], "read_support.tsv")}
    for r in rows:
        assert r[1] == off[r[0]][1] and r[3] == off[r[0]][3]                            # kmers and hits: those of the flag-off file
        assert int(r[2]) == len(sample["joined"]) < int(off[r[0]][2])                   # reads: the pairs
    assert any(r[4:] != off[r[0]][4:] for r in rows)


def test_extracted_files_are_the_models_on_fragments(runs, mid_dbs, sample):
    err, _, errs, od, _ = runs["on"]
    db_dir, ex, ex_off = mid_dbs["DB_M"]["db_dir"], os.path.join(od, DIR), os.path.join(runs["off"][3], DIR)
    tables = ["tree"] + sorted(d for d in os.listdir(od) if d.startswith("C") and os.path.isdir(os.path.join(od, d)))
    lines = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in
             (re.match(r"extract_reads: (\S+)\tN=%d\tselected on the device (\d+)\twritten (\d+)$" % N, ln) for ln in errs.split("\n")) if m}
    grew = 0
    for t in tables:
        fa = os.path.join(db_dir, "Tree_database", "kmer.fa") if t == "tree" else os.path.join(db_dir, "Kmer_Sets_L2", "Kmer_Sets", t, "all_kmer.fasta")
        with open(fa, "rb") as f:
            keys = rs_model.encode_kmers(list(dict.fromkeys(km.upper() for km in rs_model.kmers_of_fasta(f.read()))), 31)
        per = rs_model.hits_per_record(sample["flat"], keys, 31)
        keep = np.nonzero(per >= N)[0]
        for m in range(2):
            got = open(os.path.join(ex, "%s_%d.fastq" % (t, m + 1)), "rb").read()
            assert got == b"".join(sample["recs"][m][i][0] for i in keep), (t, m + 1)
        assert lines[t] == (keep.size, 2 * keep.size), (t, lines[t])                    # written = 2 x selected on the device
        # a superset of the either-mate rule at the same N
        on = set(re.findall(rb"^@frag(\d+)/1$", open(os.path.join(ex, "%s_1.fastq" % t), "rb").read(), re.M))
        off = set(re.findall(rb"^@frag(\d+)/1$", open(os.path.join(ex_off, "%s_1.fastq" % t), "rb").read(), re.M))
        assert off <= on and len(on) == keep.size
        grew += len(on - off)
        print(t, "pairs", keep.size, "either mate", len(off))
    assert grew > 0                      # (one hit in each mate: a fragment of two, no mate of two)


def test_read_classes_and_class_files_are_the_models_on_fragments(runs, mid_dbs, tm, sample, items):
    err, _, errs, od, _ = runs["on"]
    text, direct = model_text(mid_dbs["DB_M"]["db_dir"], sample["flat"], M)
    assert open(os.path.join(od, "read_classes.tsv")).read() == text
    rows = {r[0]: r for r in _tsv(od, "read_classes.tsv")}
    off = {r[0]: r for r in _tsv(runs["off"][3], "read_classes.tsv")}
    assert sum(int(r[5]) for r in rows.values()) == len(sample["joined"]) == int(direct.sum())      # reads_direct sums to the pairs
    assert all(rows[k][3:5] == off[k][3:5] for k in rows) and sorted(rows) == sorted(off)            # kmers and hits of every node
    assert int(rows[str(sample["parent"])][5]) >= 30 > int(off[str(sample["parent"])][5])            # the siblings' fragments
    cls = classes_of(tm, sample["flat"], M)
    lines = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in
             (re.match(r"extract_class: (\S+)\tM=%d\tselected on the device (\d+)\twritten (\d+)$" % M, ln) for ln in errs.split("\n")) if m}
    names = {}
    for it in items:
        c = 0 if it == "unclassified" else tm["num"][int(it.lstrip("C"))]
        keep = [i for i in range(len(cls)) if scm.in_clade(tm["parent"], int(cls[i]), c)]
        for m in range(2):
            got = open(os.path.join(od, DIR, "class_%s_%d.fastq" % (it, m + 1)), "rb").read()
            assert got == b"".join(sample["recs"][m][i][0] for i in keep), (it, m + 1)
        assert lines[it] == (len(keep), 2 * len(keep)) and len(keep) == int(rows[it.lstrip("C")][6]), it      # written = 2 x reads_clade
        names[it] = set(keep)
    # a pair is in exactly one class: the files of classes that are not nested are disjoint
    assert not names["unclassified"] & names[items[1]] and len(names["unclassified"]) + len(names[items[1]]) == len(cls)
    assert not names[items[2]] & names[items[3]] and names[items[2]] and names[items[3]]
    assert names[items[2]] | names[items[3]] <= names[items[4]] <= names[items[1]]
    assert set(sample["kinds"]["same_leaf"]) <= names[items[2]] and set(sample["kinds"]["siblings"]) <= names[items[4]] - names[items[2]] - names[items[3]]
    # flag off, the same pair stands under two classes
    off_names = [set(re.findall(rb"^@frag(\d+)/1$", open(os.path.join(runs["off"][3], DIR, "class_%s_1.fastq" % it), "rb").read(), re.M))
                 for it in ("unclassified", items[1])]
    assert off_names[0] & off_names[1]


def test_strain_support_and_strain_files_are_the_models_on_fragments(runs, mid_dbs, sample):
    import scipy.sparse as sp
    from strainscan_amd import read_reports
    od, db_dir = runs["on"][3], mid_dbs["DB_M"]["db_dir"]
    order = [r[0] for r in _tsv(od, "read_support.tsv") if r[0] != "tree"]
    rows, two = [], 0
    for cls in order:
        report = os.path.join(od, cls, "StrainVote.report")
        if not os.path.exists(report):
            continue
        called = [(int(r[0]), r[1]) for r in (ln.split("\t") for ln in open(report).read().split("\n")[1:] if ln.strip())]
        cdir = os.path.join(db_dir, "Kmer_Sets_L2", "Kmer_Sets", cls)
        with open(os.path.join(cdir, "id2strain_re.pkl"), "rb") as f:
            sid = pickle.load(f)
        col_of = {name: c for c, name in (sid.items() if isinstance(sid, dict) else enumerate(sid))}
        dense = np.asarray(sp.load_npz(os.path.join(cdir, "all_strains_re.npz")).todense())
        lab = label_model.row_labels(dense, [col_of[name] for _, name in called])
        with open(os.path.join(cdir, "all_kmer.fasta"), "rb") as f:
            keys = rs_model.encode_kmers([km.upper() for km in rs_model.kmers_of_fasta(f.read())], 31)
        per = label_model.labeled_hits_per_record(sample["flat"], keys, lab, len(called), 31)
        _, ul = label_model.kmer_labels(keys, lab)
        two += len(called) >= 2
        for j, (n, name) in enumerate(called, 1):
            rows.append(("%s.%d" % (cls, n), name, int((ul == j).sum()), len(sample["joined"]), int(per[j].sum()), rs_model.histogram(per[j], 65)))
            keep = np.nonzero(per[j] >= N)[0]
            for m in range(2):
                got = open(os.path.join(od, DIR, "%s.%d_%d.fastq" % (cls, n, m + 1)), "rb").read()
                assert got == b"".join(sample["recs"][m][i][0] for i in keep), (cls, n, m + 1)
    assert rows and two >= 1
    assert open(os.path.join(od, "strain_support.tsv")).read() == read_reports.strain_support_text(rows)
    off = {r[0]: r for r in _tsv(runs["off"][3], "strain_support.tsv")}
    assert all(r[2] == off[r[0]][2] and r[4] == off[r[0]][4] for r in _tsv(od, "strain_support.tsv"))      # kmers and hits


def _bootstrap_model(L, db_dir, solve_args, recs, b, seed):
    """{cluster: (strain names in pre-scan order, float64[b, p])} from the files of the database and the records' bytes alone, as
    tests/test_bootstrap_cli_gpu.py works it out for reads: recs = [(text, flat form)] are the units that draw a weight (here a
    pair: both mates' text, the joined sequence), solve_args what layer 1 handed to layer 2 per cluster"""
    import scipy.sparse as sp
    from oracle import oracle as orc
    keys = L.flat_record_keys(b"".join(s + b"\n" for _, s in recs))
    assert keys.shape == (len(recs), 2)
    fq_b = []
    for rep in range(b):
        w = boot_model.weights_of_keys(keys[:, 1], seed, rep)
        fq_b.append(b"".join(t * int(n) for (t, _), n in zip(recs, w.tolist())))
    out = {}
    for cls, a in sorted(solve_args.items()):
        cd = os.path.join(db_dir, "Kmer_Sets_L2", "Kmer_Sets", cls)
        kfa = open(os.path.join(cd, "all_kmer.fasta"), "rb").read()
        X = sp.load_npz(os.path.join(cd, "all_strains_re.npz")).toarray().astype(np.int64)
        om = sp.load_npz(os.path.join(cd, "overlap_matrix.npz")).toarray().astype(np.int64)[:, [int(c - 1) for c in a["all_cls"]]]
        sid = pickle.load(open(os.path.join(cd, "id2strain_re.pkl"), "rb"))
        ln = om.sum(axis=1)
        ln[ln > 1] = 0
        y = a["y"].astype(np.int64)
        cols, names, _, _, _, _ = orc.prescan(X, y, y * ln, sid, a["msn"] * a["ksize"], a["l2"], a["pmode"], a["emode"])
        alpha = None
        if len(cols) > 1:
            keep = ~((y < a["npp25"]) | (y > a["npp75"]) | (y > a["npp_out"]))
            alphas, mse = orc.enet_cv(X[keep][:, cols], y[keep])
            alpha, _, _ = orc.lasso_mpm(alphas, mse)
        coefs = np.zeros((b, len(cols)))
        for rep in range(b):
            counts, _ = orc.jellyfish_count(kfa, [fq_b[rep]], k=a["ksize"], upper=False)
            yb = np.asarray(counts, np.int64).copy()
            yb[yb == 1] = 0
            if len(cols) == 1:
                yu = yb * ln
                yy = yu if yu.sum() > 0 else yb
                coefs[rep, 0] = orc.get_avg_depth(cols[0], X, yy) if np.count_nonzero(X[:, cols[0]] * yy) else 0.0
            else:
                keep = ~((yb < a["npp25"]) | (yb > a["npp75"]) | (yb > a["npp_out"]))
                if keep.any():
                    coefs[rep] = orc.enet_fit(X[keep][:, cols], yb[keep], alpha)
        out[cls] = ([str(n) for n in names], coefs)
    return out


def test_a_fragment_draws_one_weight(L, runs, mid_dbs, sample):
    """strain_bootstrap.tsv: the replicates are the model's with the pairs as the records that draw a weight, and differ from those
    of the run that resamples mates"""
    from strainscan_amd import read_reports
    od = runs["on"][3]
    got = runs["spy_on"].replicates[None]
    frags = [(sample["recs"][0][i][0] + sample["recs"][1][i][0], r) for i, r in enumerate(sample["joined"])]
    want = _bootstrap_model(L, mid_dbs["DB_M"]["db_dir"], runs["spy_on"].args, frags, B, SEED)
    reports = sorted(c for c in runs["spy_on"].args if os.path.exists(os.path.join(od, c, "StrainVote.report")))
    assert sorted(got) == reports and reports
    for c in reports:
        names, coefs = got[c]
        assert names == want[c][0] and coefs.shape == want[c][1].shape == (B, len(names))
        assert (np.abs(coefs - want[c][1]) <= bc.TOL * np.maximum(1.0, np.abs(want[c][1]))).all(), (c, np.abs(coefs - want[c][1]).max())
    mates = runs["spy_off"].replicates[None]
    assert sorted(mates) == reports and any(not np.array_equal(mates[c][1], got[c][1]) for c in reports)
    rows = []
    text = open(os.path.join(od, "strain_bootstrap.tsv")).read()
    for c in dict.fromkeys(ln.split("\t")[0].split(".")[0] for ln in text.split("\n")[1:-1]):
        for ln in open(os.path.join(od, c, "StrainVote.report")).read().split("\n")[1:]:
            f = ln.split("\t")
            if len(f) > 5:
                rows.append(("%s.%s" % (c, f[0]), f[1], f[4], f[3], got[c][0].index(f[1]), got[c][1]))
    assert text == read_reports.bootstrap_text(rows)


def test_a_paired_bam_says_one_line_and_writes_no_per_read_report(L, mid_dbs, sample, tmp_path, monkeypatch):
    from strainscan_amd import StrainScan
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    for m in range(2):
        reads = [("frag%d" % i, s.decode().upper()) for i, (_, s) in enumerate(sample["recs"][m][:3000]) if s]
        (tmp_path / ("S%d.bam" % (m + 1))).write_bytes(bamio.bgzf(HDR, bamio.sample_records(21 + m, reads, aligned=True, decoys=0.0, extras=False),
                                                                  level=1))
    base = ["-i", str(tmp_path / "S1.bam"), "-j", str(tmp_path / "S2.bam"), "-d", mid_dbs["DB_M"]["db_dir"]]
    outs = {}
    for name, extra in (("plain", []), ("pairs", ["--read_support", "-x", "2", "--classify_reads", "1", "--extract_class", "unclassified", "--pairs"])):
        before = L.join_pairs_calls()
        od = str(tmp_path / name)
        err, _, text, errs = _run(StrainScan.main, base + ["-o", od] + extra)
        assert _ok(err), err
        outs[name] = (type(err), _result_lines(text), errs, _files(od))
        assert L.join_pairs_calls() == before
    errs = outs["pairs"][2]
    lines = [ln for ln in errs.split("\n") if ln.startswith(("pairs:", "read_support:", "extract_reads:", "classify_reads:", "extract_class:"))]
    assert len(lines) == 1 and lines[0].startswith("pairs: ") and "BAM" in lines[0] and lines[0].endswith(" and no per-read report was written"), lines
    assert outs["pairs"][0] is outs["plain"][0] and outs["pairs"][1] == outs["plain"][1] and outs["pairs"][3] == outs["plain"][3]


def test_multi_db_joins_once(L, runs, mid_dbs, sample, tmp_path, monkeypatch):
    from strainscan_amd import multi_db
    monkeypatch.setenv("SS_IMAGE_CACHE", str(tmp_path / "cache"))
    dbm, dbmem = mid_dbs["DB_M"]["db_dir"], mid_dbs["DB_Mmem"]["db_dir"]
    before = L.join_pairs_calls()
    err, rc, _, errs = _run(multi_db.main, ["-i", sample["paths"][0], "-j", sample["paths"][1], "-d", dbm, "-d", "mem=" + dbmem, "-o", str(tmp_path / "out"),
                                            "--read_support", "--classify_reads", str(M), "--pairs"])
    assert err is None and rc == 0
    assert L.join_pairs_calls() == before + 1
    assert len([ln for ln in errs.split("\n") if ln.startswith("pairs: ")]) == 1
    # the two databases hold the same genomes and the same tree: each label's files are the single run's
    for label in (os.path.basename(os.path.normpath(dbm)), "mem"):
        for name in ("read_support.tsv", "read_classes.tsv"):
            assert open(os.path.join(str(tmp_path / "out"), label, name)).read() == open(os.path.join(runs["on"][3], name)).read(), (label, name)
