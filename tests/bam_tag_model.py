"""The model of `--tag_bam` (ss_bam_tag_stream, ss_bam_tag_file), restating the rule of include/strainscan_hip.h, "Tagged BAM".

KEPT is the loader's rule: neither 0x100 nor 0x800, l_seq != 0.  flat(r) is the loader's form of kept record r (walk / read_of of
tests/test_bam_select_gpu.py; under `pairs` the fragments of tests/bam_pairs_model.py).  Class and score of a record are
class_model.classify_hits on the hits of flat(r): the class (0 below m) and the best score, which is reported whatever m is.

The body is EVERY record of the stream in file order: a record that is not kept as it is; a kept record with its block_size raised
by 14 and  t0 t1 'i' <int32 LE node_value[class]>  t2 t3 'i' <int32 LE score>  behind its last aux field.  With `pairs` both records
of a pair carry the class and score of the fragment  flat(m1) N flat(m2).

The aux fields of a kept record are walked by field: tag[2], type[1], the value (A c C: 1 byte, s S: 2, i I f: 4, Z H: up to and
with a NUL, B: subtype[1] count[4] count x size).  A field named t0t1 or t2t3: the record BEARS a tag.  An unknown type, or a field
that runs past the record's end: DAMAGED (which wins).  Either stops the call: no body.
"""
import struct

from tests import bam_pairs_model, class_model
from tests.test_bam_select_gpu import HDR, read_of, walk

TAG_BYTES = 14
AUX_OK, AUX_TAGGED, AUX_DAMAGED = 0, 1, 2
SIZES = {ord("A"): 1, ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}
COUNTERS = ("records", "tagged", "classified", "already_tagged", "fragments", "ties")


def aux_fields(aux):
    """[(tag, type, value bytes)] of a record's aux bytes; ValueError for an unknown type or a field that runs past the end"""
    p, n, out = 0, len(aux), []
    while p < n:
        if n - p < 3:
            raise ValueError("a field of %d bytes" % (n - p))
        tag, ty = aux[p:p + 2], aux[p + 2]
        p += 3
        if ty in SIZES:
            q = p + SIZES[ty]
        elif ty in b"ZH":
            z = aux.find(b"\0", p)
            if z < 0:
                raise ValueError("no NUL")
            q = z + 1
        elif ty == ord("B"):
            if n - p < 5:
                raise ValueError("a B field without its count")
            sub, count = aux[p], struct.unpack_from("<I", aux, p + 1)[0]
            if sub not in SIZES or sub == ord("A"):
                raise ValueError("B subtype %r" % chr(sub))
            q = p + 5 + count * SIZES[sub]
        else:
            raise ValueError("type %r" % ty)
        if q > n:
            raise ValueError("a field runs past the end")
        out.append((tag, ty, aux[p:q]))
        p = q
    return out


def aux_walk(aux, tags):
    try:
        fields = aux_fields(aux)
    except ValueError:
        return AUX_DAMAGED
    return AUX_TAGGED if any(t in (tags[:2], tags[2:4]) for t, _, _ in fields) else AUX_OK


def aux_of(stream, at, size):
    """the aux bytes of the record at stream[at:at + size]"""
    lrn = stream[at + 12]
    ncig, _, lseq = struct.unpack_from("<HHI", stream, at + 16)
    return stream[at + 36 + lrn + 4 * ncig + (lseq + 1) // 2 + lseq:at + size]


def rebase(stream):
    """the records of `stream` behind the header that walk() expects (the body never holds the header)"""
    return HDR + stream[bam_pairs_model.header_end(stream):]


def tag_bytes(tags, value, score):
    return tags[:2] + b"i" + struct.pack("<i", value) + tags[2:4] + b"i" + struct.pack("<i", score)


def model(stream, keys, row_node, parent, n_nodes, k, m, node_value, tags=b"snsc", pairs=False, min_qual=0):
    """-> (body bytes, counters[6], direct, node_hits, kmers); body None (and the counters as far as they are defined: records,
    tagged, already_tagged) when a name group is no pair, a kept record bears a tag or its aux fields are damaged"""
    stream = rebase(stream)
    recs = walk(stream)
    kept = [i for i, r in enumerate(recs) if not r[2] & 0x900 and r[3]]
    counters = [len(recs), len(kept), 0, 0, len(kept), 0]
    if pairs:
        frags, _, _, who = bam_pairs_model.fragments(stream, min_qual)
        if frags is None:
            return None, counters, None, None, None
        text = b"".join(f + b"\n" for f in frags)
        of = {}                                            # record -> its fragment
        for g, (a, b) in enumerate(who):
            of[a] = g
            if b is not None:
                of[b] = g
        counters[4] = len(frags)
    else:
        text = "".join(read_of(recs[i][2], recs[i][3], recs[i][5], recs[i][6], min_qual) + "\n" for i in kept).encode()
        of = {i: g for g, i in enumerate(kept)}
    per, n_text = class_model.record_hits(text, keys, row_node, k)
    assert n_text == counters[4]
    detail = class_model.classes_detail(text, keys, row_node, parent, k, m, per)
    direct, node_hits, kmers = class_model.classify_model(text, keys, row_node, parent, n_nodes, k, m, per)
    counters[5] = sum(1 for d in detail if d[2])
    counters[2] = sum(1 for i in kept if detail[of[i]][0])
    walks = [aux_walk(aux_of(stream, recs[i][0], recs[i][1]), tags) for i in kept]
    if AUX_DAMAGED in walks:
        return None, counters, direct, node_hits, kmers
    counters[3] = walks.count(AUX_TAGGED)
    if counters[3]:
        return None, counters, direct, node_hits, kmers
    out = []
    for i, r in enumerate(recs):
        raw = stream[r[0]:r[0] + r[1]]
        if i in of:
            cls, score = detail[of[i]][0], detail[of[i]][1]
            raw = struct.pack("<i", r[1] - 4 + TAG_BYTES) + raw[4:] + tag_bytes(tags, int(node_value[cls]), score)
        out.append(raw)
    return b"".join(out), counters, direct, node_hits, kmers


def offsets(stream):
    """[(D, E, kept)] of every record in the body the model writes: where it begins and ends there"""
    recs = walk(rebase(stream))
    out, d = [], 0
    for r in recs:
        k = not r[2] & 0x900 and r[3] != 0
        e = d + r[1] + (TAG_BYTES if k else 0)
        out.append((d, e, bool(k)))
        d = e
    return out


def read_tags(body, tags=b"snsc"):
    """[(flag, name, value or None, score or None)] of the records of a body (no header): the two tags read back through the field
    walk, None where a record has none"""
    p, out = 0, []
    while p < len(body):
        size = 4 + struct.unpack_from("<i", body, p)[0]
        lrn = body[p + 12]
        flag = struct.unpack_from("<H", body, p + 18)[0]
        got = {t: struct.unpack("<i", v)[0] for t, ty, v in aux_fields(aux_of(body, p, size)) if ty == ord("i")}
        out.append((flag, body[p + 36:p + 36 + lrn].split(b"\0")[0], got.get(tags[:2]), got.get(tags[2:4])))
        p += size
    assert p == len(body)
    return out
