"""The model of `--read_calls` that the read-call tests hold the device, the writer and the command to.

Per record (class_model's record, hit, h[v], score and class): the record's HIT LIST is every node v >= 1 with h[v] > 0, in
ascending v, with h[v]; hits of k-mers without a node (node 0) are not listed.  The lists of all records stand behind each other,
first[i] .. first[i + 1] - 1 being record i's.  The score is the largest score(v), reported below m too.

The table: the input file walked record by record -- a FASTQ record is a header line `@...`, sequence lines up to a line that
begins with `+`, then quality lines until they hold as many characters as the sequence lines; a FASTA record a header line `>...`
and the lines up to the next `>`; other lines between records are skipped.  One line per record, name TAB node TAB score TAB
length TAB hits: name = the header behind its marker up to the first space, tab, CR or LF; a record whose sequence lines hold
nothing is `name -1 0 0 -` and takes no entry of the arrays, every other record takes the next one; length counts the sequence
lines' characters but CR; hits = `id:h` items separated by a space, `-` for none.  Two files of a joined set: record j of both
files takes entry j, each with its own length.

Everything is plain Python: it is the statement, not a fast one.
"""
import numpy as np

from tests import class_model as cm

HEADER = b"name\tnode\tscore\tlength\thits\n"


def record_lists(per):
    """[{node: hits}] per record (class_model.record_hits) -> [[(v, h[v])] ascending in v, v >= 1]"""
    return [sorted((int(v), int(c)) for v, c in h.items() if v and c) for h in per]


def calls_model(text, keys, row_node, parent, k, m, per=None):
    """-> dict(classes u32[n], scores u32[n], first u64[n + 1], list_node u32, list_hits u32, ties, lists) for the records of the
    flat block `text`, in rs_model.record_ids' numbering"""
    if per is None:
        per, _ = cm.record_hits(text, keys, row_node, k)
    det = cm.classes_detail(text, keys, row_node, parent, k, m, per)
    lists = record_lists(per)
    first = np.zeros(len(lists) + 1, np.uint64)
    first[1:] = np.cumsum([len(x) for x in lists])
    flat = [e for x in lists for e in x]
    return dict(classes=np.array([d[0] for d in det], np.uint32), scores=np.array([d[1] for d in det], np.uint32), first=first,
                list_node=np.array([v for v, _ in flat], np.uint32), list_hits=np.array([c for _, c in flat], np.uint32),
                ties=sum(1 for d in det if d[2]), lists=lists)


def walk_records(text):
    """[(name, flat form, length)] of a FASTA / FASTQ text (bytes): the flat form is the sequence lines concatenated (a CR at a
    line's end stays in it, as in the loader's), length its characters other than CR"""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    out, i = [], 0

    def name_of(header):
        n = header[1:]
        for stop in (b" ", b"\t", b"\r"):
            n = n.split(stop)[0]
        return n

    while i < len(lines):
        ln = lines[i]
        if ln.startswith(b">"):
            i += 1
            seq = []
            while i < len(lines) and not lines[i].startswith(b">"):
                seq.append(lines[i])
                i += 1
        elif ln.startswith(b"@"):
            i += 1
            seq = []
            while i < len(lines) and not lines[i].startswith(b"+"):
                seq.append(lines[i])
                i += 1
            i += 1                                   # the '+' line
            want, got = sum(len(s) for s in seq), 0
            while i < len(lines) and got < want:
                got += len(lines[i])
                i += 1
        else:
            i += 1
            continue
        flat = b"".join(seq)
        out.append((name_of(ln), flat, len(flat) - flat.count(b"\r")))
    return out


def _line(name, node, score, length, items):
    return b"%s\t%d\t%d\t%d\t%s\n" % (name, node, score, length, b" ".join(b"%d:%d" % it for it in items) or b"-")


def table_text(texts, calls, node_value):
    """The files of `--read_calls` for the input texts (one, or the two of a joined set) -> [bytes]; calls: dict(classes=, scores=,
    first=, list_node=, list_hits=) of the set; node_value[v]: what stands for class or node v.  ValueError where the records of
    the texts are not those of `calls`."""
    recs = [walk_records(t) for t in texts]
    n = len(calls["classes"])
    first = [int(x) for x in calls["first"]]

    def entry(i, name, length):
        if i >= n:
            raise ValueError("more records than entries")
        items = [(int(node_value[calls["list_node"][e]]), int(calls["list_hits"][e])) for e in range(first[i], first[i + 1])]
        return _line(name, int(node_value[calls["classes"][i]]), int(calls["scores"][i]), length, items)

    out = []
    if len(texts) == 2:
        if len(recs[0]) != len(recs[1]) or len(recs[0]) != n:
            raise ValueError("the files and the set differ in records")
        for rs in recs:
            out.append(HEADER + b"".join(entry(j, name, length) for j, (name, _, length) in enumerate(rs)))
        return out
    i, rows = 0, []
    for name, flat, length in recs[0]:
        if not flat:
            rows.append(_line(name, -1, 0, 0, []))
        else:
            rows.append(entry(i, name, length))
            i += 1
    if i != n:
        raise ValueError("the file and the set differ in records")
    return [HEADER + b"".join(rows)]
