"""The base-quality mask (`strainscan -q Q`, ss_set_min_base_qual) stated in Python, and inputs with a realistic quality profile.

mask_fastx(blob, q) is the whole definition for FASTA/FASTQ text: over the record grammar jellyfish 2.3.0 accepts, the i-th
sequence character of a FASTQ record becomes N when the i-th quality character consumed for the record has a byte value below
33 + q; FASTA records are untouched.  tests/golden/qual_mask.json pins it to the real `jellyfish count -Q`.  The product run with
the threshold on X must equal the product run without it on mask(X)."""
import numpy as np

from tests import bamio


def mask_fastx(blob, q, count=None):
    """blob with the mask applied.  count: a one-element list that receives the number of sequence characters whose quality
    was below the threshold (what ss_mask_counters counts: an N among them too)."""
    if q <= 0:
        if count is not None:
            count[0] = 0
        return blob
    thr = 33 + q
    out = bytearray(blob)
    n = len(blob)
    pos = 0
    masked = 0

    def line(p):
        e = blob.find(b"\n", p)
        return (p, n, n) if e < 0 else (p, e, e + 1)

    while pos < n:
        s, e, nx = line(pos)
        if e == s:                                  # a blank line between records
            pos = nx
            continue
        c = blob[s]
        if c == ord(">"):
            pos = nx
            while pos < n and blob[pos] != ord(">"):
                pos = line(pos)[2]
            continue
        pos = nx
        if c != ord("@"):                           # a stray line
            continue
        seq_idx = []
        while pos < n and blob[pos] != ord("+"):
            s, e, pos = line(pos)
            seq_idx.extend(range(s, e))
        if pos < n:
            pos = line(pos)[2]                      # the '+' line
        got = 0
        while got < len(seq_idx) and pos < n:      # whole quality lines until there are as many characters as bases
            s, e, pos = line(pos)
            for j in range(s, e):
                if got < len(seq_idx) and blob[j] < thr:
                    out[seq_idx[got]] = ord("N")
                    masked += 1
                got += 1
    if count is not None:
        count[0] = masked
    return bytes(out)


def realistic_quals(rs, n):
    """Phred values of one read: each base 2..12 with probability 1-2 %, else 30..40; one read in five has a tail that decays
    from the high band towards Phred 2."""
    q = rs.randint(30, 41, size=n)
    low = rs.random_sample(n) < rs.uniform(0.01, 0.02)
    q[low] = rs.randint(2, 13, size=int(low.sum()))
    if n > 20 and rs.random_sample() < 0.2:
        t = int(rs.randint(5, max(6, n // 3)))
        q[n - t:] = np.maximum(2, q[n - t:] - (np.arange(t) * 36 // t + rs.randint(0, 4, size=t)))
    return q.astype(np.uint8)


def fastq_with_quals(rs, reads, names=None):
    """[letters (bytes)] -> (four-line FASTQ text, [Phred arrays])."""
    out, quals = [], []
    for i, r in enumerate(reads):
        q = realistic_quals(rs, len(r))
        quals.append(q)
        out.append(b"@" + (names[i] if names else b"r%d" % i) + b"\n" + r + b"\n+\n" + (q + 33).astype(np.uint8).tobytes() + b"\n")
    return b"".join(out), quals


def mask_read(read, quals, q):
    """One read (bytes, as sequenced) under Phred values in the same order -> (masked read, bases masked)."""
    a = np.frombuffer(read, np.uint8).copy()
    low = np.asarray(quals) < q
    a[low] = ord("N")
    return a.tobytes(), int(low.sum())


def qual_known_deviation(kinds):
    """Inputs on which `jellyfish count -Q` is no reference for the mask: whatever scenarios_fuzz.fmt_known_deviation names, and
    * a FASTQ file with a blank line (`fq_blank_tail`): with -Q, jellyfish 2.3.0 drops the reads of such a file (a two-record
      file with one blank line at the end or between the records counts 0 with -Q and 2 without) -- a defect of the binary in
      the family of its "no final newline" loss; the product follows the definition and does not imitate it."""
    from tests import scenarios_fuzz as sf
    why = sf.fmt_known_deviation(kinds)
    if why:
        return why
    if any(k.split("+")[0] == "fq_blank_tail" for k in kinds):
        return "FASTQ with a blank line under -Q"
    return None


def real_case(seed, root_dir):
    """The database of scenarios_fuzz.fmt_case(seed) and a four-line FASTQ sample with the realistic quality profile (gzip for
    odd seeds) -> (info, [path], [bytes as written, uncompressed], [kind])"""
    import gzip
    import os
    from tests import scenarios_fuzz as sf
    from tests import synth
    info, _, _, _ = sf.fmt_case(seed, root_dir)
    rs = np.random.RandomState(7700000 + seed)
    leaf = int(rs.permutation(info["tree"].leaves)[0])
    fq = synth.simulate_reads([(info["leaf_genome"][leaf], 5.0), (synth.rand_seq(rs, 2000), 2.0)], 7800000 + seed, read_len=150)
    lines = fq.split(b"\n")
    blob, _ = fastq_with_quals(rs, lines[1::4][:len(lines) // 4], names=[ln[1:] for ln in lines[0::4][:len(lines) // 4]])
    gz = bool(seed % 2)
    p = os.path.join(root_dir, "real%d.fq%s" % (seed, ".gz" if gz else ""))
    if gz:
        with open(p, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", compresslevel=6, mtime=0) as z:
            z.write(blob)
    else:
        with open(p, "wb") as f:
            f.write(blob)
    return info, [p], [blob], ["real" + ("+gz" if gz else "")]


class FastqSample:
    """Reads with realistic qualities as four-line FASTQ: text(q) is mask(X, q) built from the arrays (q = 0: X itself),
    flat(q) the flat block the product must hold, masked(q) what ss_mask_counters must move by."""

    def __init__(self, seed, reads, names=None):
        rs = np.random.RandomState(seed)
        self.reads = [bytes(r) for r in reads]
        self.names = names or [b"r%d" % i for i in range(len(reads))]
        self.quals = [realistic_quals(rs, len(r)) for r in self.reads]
        self.qtext = [(q + 33).astype(np.uint8).tobytes() for q in self.quals]

    def masked_reads(self, q):
        return [mask_read(r, ql, q)[0] for r, ql in zip(self.reads, self.quals)] if q else list(self.reads)

    def masked(self, q):
        return int(sum(int((ql < q).sum()) for ql in self.quals)) if q else 0

    def text(self, q=0, lo=0, hi=None):
        rd = self.masked_reads(q)[lo:hi]
        return b"".join(b"@" + n + b"\n" + r + b"\n+\n" + t + b"\n" for n, r, t in zip(self.names[lo:hi], rd, self.qtext[lo:hi]))

    def flat(self, q=0):
        return b"".join(r + b"\n" for r in self.masked_reads(q))


def requal_fastq(seed, blob):
    """A four-line FASTQ text (constant qualities, as tests/synth.py writes it) -> FastqSample of the same reads and names."""
    lines = blob.split(b"\n")
    n = len(lines) // 4
    return FastqSample(seed, lines[1:4 * n:4], [ln[1:] for ln in lines[0:4 * n:4]])


class BamSample:
    """The reads of a FastqSample as BAM records: a share stored reverse-complemented (0x10, qualities reversed with the
    bases), a share without qualities (0xFF in every place: never masked), optionally secondary / supplementary decoys and aux
    fields.  records(q) is mask(X, q) -- the same records with N stored at the masked places -- so that a load of records(q)
    without a threshold is what a load of records(0) under threshold q must give."""

    def __init__(self, seed, fq, reverse_share=0.5, no_qual_share=0.05, decoys=0.0, extras=False):
        rs = np.random.RandomState(seed)
        self.fq = fq
        self.spec = []
        for i in range(len(fq.reads)):
            self.spec.append(dict(rev=bool(rs.random_sample() < reverse_share), noq=bool(rs.random_sample() < no_qual_share),
                                  pos=int(rs.randint(0, 99999)), decoy=bool(rs.random_sample() < decoys),
                                  aux=(b"RGZgrp1\0NMC" + bytes([int(rs.randint(0, 9))])) if extras else b""))
        self.decoy_seq = "".join("ACGT"[c] for c in rs.randint(0, 4, size=90))

    def kept_reads(self, q):
        """The reads the product must hold under threshold q, in record order."""
        return [r if s["noq"] else mask_read(r, ql, q)[0] for r, ql, s in zip(self.fq.reads, self.fq.quals, self.spec)] if q else list(self.fq.reads)

    def masked(self, q):
        return int(sum(int((ql < q).sum()) for ql, s in zip(self.fq.quals, self.spec) if not s["noq"])) if q else 0

    def no_qual(self):
        return sum(1 for s in self.spec if s["noq"])

    def records(self, q=0):
        out = []
        for name, r, ql, s in zip(self.fq.names, self.kept_reads(q), self.fq.quals, self.spec):
            seq, quals = r.decode(), (bytes([0xFF] * len(r)) if s["noq"] else ql.tobytes())
            if s["rev"]:
                out.append(bamio.record(name.decode(), bamio.revcomp(seq), flag=0x10, ref=0, pos=s["pos"], cigar=((len(seq) << 4) | 0,),
                                        qual=quals[::-1], aux=s["aux"], mapq=60))
            else:
                out.append(bamio.record(name.decode(), seq, flag=4, qual=quals, aux=s["aux"]))
            if s["decoy"]:                        # low qualities on a skipped record must not be counted
                out.append(bamio.record(name.decode(), self.decoy_seq, flag=0x100, ref=0, pos=5, cigar=((90 << 4),), qual=bytes([3] * 90)))
        return out
