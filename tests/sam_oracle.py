"""CPU statement of the SAM record of include/biogpu.h (bg_sam_header, bg_sam_emit_batch[_dev]), for the tests.

Pure Python over the numpy outputs of the existing host calls: FASTQ records (`fastq.Parsed` or anything with text / recs / seq /
qual), hits, strand and operations of a seed-and-extend call, optionally its multi or pair records.  Field 6 is
`oracle_py.cigar`, field 10 `dna.revcomp`; everything else is restated here from the header's words."""
import bisect

import numpy as np

import oracle_py as orc
from rust_bio_amd.alphabets import dna

MIN_SCORE = -858993459
HIT_REVERSE, HIT_NONE = 1, 255
PAIRED, SECONDARY, TAG_NM, TAG_MD = 1, 2, 4, 8
MATCH, SUBST, DEL, INS = 0, 1, 2, 3


def header(contigs):
    """contigs: [(name: bytes, start, len)]"""
    sq = b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (name, ln) for name, _, ln in contigs)
    return b"@HD\tVN:1.6\tSO:unsorted\n" + sq + b"@PG\tID:biogpu\tPN:biogpu\n"


def md_of(ops, ref_start, text):
    """the MD string: walk the operations from ref_start with a counter"""
    out, c, t, prev = [], 0, ref_start, None
    for op in ops:
        if op == MATCH:
            c += 1
            t += 1
        elif op == SUBST:
            out.append(b"%d%c" % (c, text[t]))
            c = 0
            t += 1
        elif op == DEL:
            if prev != DEL:  # a run of consecutive DEL opens with the counter and '^'
                out.append(b"%d^" % c)
                c = 0
            out.append(bytes([text[t]]))
            t += 1
        prev = op
    out.append(b"%d" % c)
    return b"".join(out)


class Slot:
    """one hit slot seen through the placement rule"""

    def __init__(self, hit, strand, starts, contigs):
        self.hit, self.strand = hit, int(strand)
        self.ref_start, self.ref_end = int(hit["ref_start"]), int(hit["ref_end"])
        self.contig = None
        if int(hit["aln"]["score"]) != MIN_SCORE and self.strand != HIT_NONE:
            c = bisect.bisect_right(starts, self.ref_start) - 1
            if c >= 0:
                end = contigs[c][1] + contigs[c][2]
                if self.ref_start < end and self.ref_start <= self.ref_end <= end:
                    self.contig = c
        self.placed = self.contig is not None
        self.pos = self.ref_start - contigs[self.contig][1] + 1 if self.placed else 0
        self.reverse = self.placed and self.strand == HIT_REVERSE


def lines(contigs, fq, hits, strand, ops, flags=0, K=1, multi=None, pairs=None, text=None):
    """The lines of every slot, in slot order: a list of n_reads * K bytes objects (b"" for a slot that writes no line).
    contigs: [(name: bytes, start, len)]; fq: text / recs / seq / qual; hits, strand: n_reads * K entries (any shape); ops: the
    buffer aln.ops_off points into; text: the indexed text (for MD)."""
    hits, strand = np.asarray(hits).reshape(-1), np.asarray(strand).reshape(-1)
    starts = [c[1] for c in contigs]
    n = len(fq.recs)
    assert len(hits) == len(strand) == n * K
    slots = [Slot(hits[s], strand[s], starts, contigs) for s in range(n * K)]
    fq_text, seqs, quals = bytes(fq.text), bytes(fq.seq), bytes(fq.qual)
    paired = bool(flags & PAIRED)
    assert not paired or (K == 1 and n % 2 == 0 and pairs is not None)
    out = []
    for s, me in enumerate(slots):
        r, k = divmod(s, K)
        if k > 0 and not (flags & SECONDARY and me.placed and slots[r * K].placed):
            out.append(b"")
            continue
        rec, hit = fq.recs[r], me.hit
        qname = fq_text[int(rec["id_off"]):int(rec["id_off"]) + int(rec["id_len"])]
        flag = (0 if me.placed else 0x4) | (0x10 if me.reverse else 0) | (0x100 if k else 0)
        rname, pos = (contigs[me.contig][0], me.pos) if me.placed else (b"*", 0)
        rnext, pnext, tlen = b"*", 0, 0
        if paired:
            mate, first = slots[s ^ 1], r % 2 == 0
            if len(qname) > 2 and qname.endswith(b"/1" if first else b"/2"):
                qname = qname[:-2]
            flag |= 0x1 | (0x40 if first else 0x80) | (0 if mate.placed else 0x8) | (0x20 if mate.reverse else 0)
            both = me.placed and mate.placed and me.contig == mate.contig
            if both and pairs["proper"][r // 2]:
                flag |= 0x2
            if not me.placed and mate.placed:  # SAM 1.4: an unplaced mate sits with its partner
                rname, pos = contigs[mate.contig][0], mate.pos
            if me.placed or mate.placed:
                mate_rname, pnext = (contigs[mate.contig][0], mate.pos) if mate.placed else (rname, pos)
                rnext = b"=" if mate_rname == rname else mate_rname
            if both:
                span = max(me.ref_end, mate.ref_end) - min(me.ref_start, mate.ref_start)
                leftmost = me.ref_start < mate.ref_start or (me.ref_start == mate.ref_start and first)
                tlen = span if leftmost else -span
        mapq = 0 if (not me.placed or k) else (int(multi["mapq"][r]) if multi is not None else 255)
        n_ops, ops_off = int(hit["aln"]["n_ops"]), int(hit["aln"]["ops_off"])
        my_ops = np.asarray(ops[ops_off:ops_off + n_ops]) if me.placed else np.zeros(0, np.uint8)
        cigar = b"*"
        if me.placed and n_ops:
            aln = {f: int(hit["aln"][f]) for f in ("xstart", "xend", "xlen", "mode")}
            cigar = orc.cigar(aln, my_ops.astype(np.uint64), False).encode()
        seq = seqs[int(rec["seq_off"]):int(rec["seq_off"]) + int(rec["seq_len"])]
        qual = quals[int(rec["qual_off"]):int(rec["qual_off"]) + int(rec["qual_len"])]
        if me.reverse:
            seq, qual = dna.revcomp(seq), qual[::-1]
        if k or not seq:
            seq = b"*"
        if k or not qual or int(rec["qual_len"]) != int(rec["seq_len"]):
            qual = b"*"
        fields = [qname or b"*", b"%d" % flag, rname, b"%d" % pos, b"%d" % mapq, cigar, rnext, b"%d" % pnext, b"%d" % tlen, seq, qual]
        if me.placed:
            fields.append(b"AS:i:%d" % int(hit["aln"]["score"]))
            if multi is not None and k == 0 and int(multi["sub_score"][r]) != MIN_SCORE:
                fields.append(b"XS:i:%d" % int(multi["sub_score"][r]))
            if flags & TAG_NM:
                fields.append(b"NM:i:%d" % int(np.isin(my_ops, (SUBST, INS, DEL)).sum()))
            if flags & TAG_MD:
                fields.append(b"MD:Z:" + md_of(my_ops.tolist(), me.ref_start, text))
        out.append(b"\t".join(fields) + b"\n")
    return out


class Fastq:
    """FASTQ records of a list of (id, seq, qual) bytes triples in the layout of fastq.Parsed: text / recs / seq / qual"""

    def __init__(self, reads, rec_dtype):
        self.recs = np.zeros(len(reads), dtype=rec_dtype)
        text, seq, qual = b"", b"", b""
        for r, (id_, s, q) in enumerate(reads):
            self.recs[r] = (len(text) + 1, 0, len(seq), len(qual), len(id_), 0, len(s), len(q), 0, 0)
            text += b"@" + id_ + b"\n" + s + b"\n+\n" + q + b"\n"
            seq += s
            qual += q
        self.text, self.seq, self.qual = (np.frombuffer(b, dtype=np.uint8) for b in (text, seq, qual))


def kat_arrays(kat, hit_dtype, multi_dtype, pair_dtype, rec_dtype):
    """one record case of tests/golden/sam_kats.json as the arrays the calls take:
    (flags, K, Fastq, hits, strand, ops, multi or None, pairs or None)"""
    flags = sum({"PAIRED": PAIRED, "SECONDARY": SECONDARY, "NM": TAG_NM, "MD": TAG_MD}[f] for f in kat["flags"])
    fq = Fastq([(r["id"].encode(), r["seq"].encode(), r["qual"].encode()) for r in kat["reads"]], rec_dtype)
    hits = np.zeros(len(kat["hits"]), dtype=hit_dtype)
    strand = np.full(len(hits), HIT_NONE, dtype=np.uint8)
    ops = []
    for s, h in enumerate(kat["hits"]):
        if h is None:
            hits[s]["aln"]["score"] = MIN_SCORE
            hits[s]["window_start"] = hits[s]["ref_start"] = hits[s]["ref_end"] = 2**64 - 1
            continue
        a = hits[s]["aln"]
        a["score"], a["xstart"], a["xend"], a["xlen"], a["mode"] = h["score"], h["xstart"], h["xend"], h["xlen"], 2
        a["n_ops"], a["ops_off"] = len(h["ops"]), len(ops)
        hits[s]["ref_start"], hits[s]["ref_end"], strand[s] = h["ref_start"], h["ref_end"], h["strand"]
        ops += ["=XDI".index(c) for c in h["ops"]]
    multi = pairs = None
    if kat.get("multi"):
        multi = np.zeros(len(kat["multi"]), dtype=multi_dtype)
        for r, m in enumerate(kat["multi"]):
            multi[r]["mapq"], multi[r]["sub_score"] = m["mapq"], MIN_SCORE if m["sub_score"] is None else m["sub_score"]
    if kat.get("pairs"):
        pairs = np.zeros(len(kat["pairs"]), dtype=pair_dtype)
        for p, m in enumerate(kat["pairs"]):
            pairs[p]["proper"], pairs[p]["span"] = m["proper"], m["span"]
    return flags, kat["K"], fq, hits, strand, np.array(ops, dtype=np.uint8), multi, pairs


def offsets(ls):
    off = np.zeros(len(ls) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in ls])
    return off
