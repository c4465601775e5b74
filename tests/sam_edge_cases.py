"""Hand-made hit records for the SAM writer, the sort keys, the permuted copy and the duplicate marker at the places where
their kernels change behaviour: the decimal width of every numeric field, the staging limit of the write pass, the slots per
group / block / scan tile, the lengths around the switch between the two copy kernels and around a chunk of the long one, and
the 16 lanes of the score kernel.  No seeding, no alignment, no genome: records in the style of `sam_oracle.kat_arrays` and
tests/sam_sort_cases.py.  Every generator returns its inputs together with `covers`, a line on what it claims to hold;
tests/test_sam_edge_cases.py (no GPU) derives from the oracles alone that the claim is true, and the GPU tests import the same
generators."""
import functools
import random
import re

import numpy as np

import sam_oracle as so
import sam_sort_oracle as sso
from rust_bio_amd import _lib
from sam_sort_cases import BIG_CONTIGS, CONTIGS, PHRED, arrays, make_hit, random_batch, read_of

DTYPES = (_lib.SEED_HIT_DTYPE, _lib.MULTI_HIT_DTYPE, _lib.PAIR_HIT_DTYPE, _lib.FQREC_DTYPE)
TOP = 2**64 - 1
STAGE = 1040          # sam_emit.hip: a line is staged in LDS when (offset mod 16) + length <= 1040
LONG_LINE = 16384     # sam_rule.h: SAM_LONG_LINE
CHUNK = 4096          # sam_rule.h: SAM_CHUNK_VECS * 16

# ---- the texts and contig tables ---------------------------------------------------------------------------------------
# the indexed text of the cases that ask for MD: four contigs, the second long enough for an MD counter of 10 000
MD_CONTIGS = [(b"m0", 0, 1500), (b"m1", 1501, 11000), (b"m2", 12502, 2000), (b"m3", 14503, 1500)]
# coordinates far beyond any text (no MD): ref_start needs more than 32 bits while POS does not
FAR = 2**40 + 77
WIDE_CONTIGS = [(b"lo", 5, 3000), (b"far", FAR, 3_000_000_000)]
NAME_CONTIGS = [(b"c", 0, 1000), ((b"L" + b"0123456789" * 20)[:200], 1000, 1000), (b"mid", 2000, 1000)]


@functools.lru_cache(maxsize=None)
def md_text():
    """the text under MD_CONTIGS: random bases, a '$' behind every contig"""
    rng = np.random.default_rng(101)
    end = MD_CONTIGS[-1][1] + MD_CONTIGS[-1][2]
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=end + 1)
    for _, start, ln in MD_CONTIGS:
        text[start + ln] = ord("$")
    return text


POS_VALUES = sorted({1, 2_147_483_647, 2_999_999_999} | {10**k for k in range(1, 10)} | {10**k - 1 for k in range(1, 10)})
SPANS = [0] + POS_VALUES
SCORES = [0, 9, -9, 10, -10, 99_999, -99_999, 2_147_483_647, so.MIN_SCORE + 1]
MAPQS = [0, 9, 10, 99, 100, 254]
NMS = [0, 9, 10, 99, 100, 1000]
RUNS = [1, 9, 10, 99, 100, 999, 1000, 9999, 10_000]
DUPS = [0, 1, 0x7e, 255]
GRID_SLOTS = [1, 15, 16, 17, 255, 256, 257, 2047, 2048, 2049]
GRID_READS_K8 = [1, 2, 3, 31, 32, 33, 255, 256, 257]  # K = 8: n_slots is a multiple of 8 (see grid())


# ---- building blocks -----------------------------------------------------------------------------------------------------
def bases(n, salt=0):
    j = np.arange(n, dtype=np.int64)
    return np.frombuffer(b"ACGTN", np.uint8)[(j * 7 + (j >> 3) + salt) % 5].tobytes()


def quals(n, salt=0):
    j = np.arange(n, dtype=np.int64)
    return (33 + (j * 11 + (j >> 6) + salt) % 90).astype(np.uint8).tobytes()


def read(id_, n, salt=0):
    return {"id": id_, "seq": bases(n, salt), "qual": quals(n, salt)}


def hit(at, ops, strand=0, score=30, xstart=0, tail=0, ref_end=None):
    """a hit at text coordinate `at` with the operations `ops` (a string over =XDI) and soft clips of xstart and tail"""
    q = sum(ops.count(c) for c in "=XI")
    r = sum(ops.count(c) for c in "=XD")
    return {"score": score, "strand": strand, "ref_start": at, "ref_end": at + r if ref_end is None else ref_end, "xstart": xstart,
            "xend": xstart + q, "xlen": xstart + q + tail, "ops": ops}


def kat_arrays(kat):
    """sam_oracle.kat_arrays for reads whose id / seq / qual are bytes"""
    fq = so.Fastq([(r["id"], r["seq"], r["qual"]) for r in kat["reads"]], DTYPES[3])
    k2 = dict(kat, reads=[])
    flags, K, _, hits, strand, ops, multi, pairs = so.kat_arrays(k2, *DTYPES)
    return flags, K, fq, hits, strand, ops, multi, pairs


class EmitCase:
    """the arrays of one writer call, the oracle's lines, and what the case claims to cover"""

    def __init__(self, name, covers, contigs, kat, text=None, dup=None):
        self.name, self.covers, self.contigs, self.text = name, covers, contigs, text
        self.flags, self.K, self.fq, self.hits, self.strand, self.ops, self.multi, self.pairs = kat_arrays(kat)
        self.dup = None if dup is None else np.asarray(dup, dtype=np.uint8)
        self.n = len(self.fq.recs)
        assert len(self.hits) == self.n * self.K
        assert not self.flags & so.TAG_MD or text is not None
        self._want = None

    def want(self):
        """the oracle's lines of every slot"""
        if self._want is None:
            text = None if self.text is None else self.text.tobytes()
            ls = so.lines(self.contigs, self.fq, self.hits, self.strand, self.ops, self.flags, self.K, self.multi, self.pairs, text)
            self._want = ls if self.dup is None else sso.add_dup_flag(ls, self.dup, self.K)
        return self._want


def fields(line):
    return line[:-1].split(b"\t")


def tag(line, name):
    for t in fields(line)[11:]:
        if t.startswith(name):
            return t[5:]
    return None


def two_slots(name, covers, contigs, values, make, flags, multi=None, text=None, extra=()):
    """K = 2 with secondary lines.  For every value two reads: A with make(v, forward) in slot 0 and make(v, reverse) in slot 1
    (a secondary line), B with make(v, reverse) in slot 0 and nothing in slot 1; then an unplaced read; `extra`: more
    (read, slot 0, slot 1).  multi: v, i -> the multi record of the two reads."""
    reads, hits, ms = [], [], []
    for i, v in enumerate(values):
        f, r = make(v, 0), make(v, 1)
        reads += [read(b"A%d" % i, f["xlen"], i), read(b"B%d" % i, r["xlen"], i + 1)]
        hits += [f, r, r, None]
        ms += [multi(v, i, 0), multi(v, i, 1)] if multi else []
    reads.append(read(b"none", 7))
    hits += [None, hit(contigs[0][1] + 1, "=" * 7)]  # a placed slot 1 behind an unplaced slot 0 writes nothing
    ms += [{"mapq": 99, "sub_score": 5}] if multi else []
    for rd, h0, h1 in extra:
        reads.append(rd)
        hits += [h0, h1]
        ms += [{"mapq": 60, "sub_score": None}] if multi else []
    kat = {"flags": ["SECONDARY"] + flags, "K": 2, "reads": reads, "hits": hits, "multi": ms or None}
    return EmitCase(name, covers, contigs, kat, text)


# ---- the writer: field widths ----------------------------------------------------------------------------------------------
def pos_pnext():
    reads, hits, pairs = [], [], []
    n = len(POS_VALUES)
    for i, v in enumerate(POS_VALUES):
        w = POS_VALUES[(i + 1) % n]
        # mate 1 forward at POS v, mate 2 reverse at POS w; then mate 1 reverse at POS v with an unplaced mate 2 that borrows it
        for h1, h2 in ((hit(FAR + v - 1, "=", 0), hit(FAR + w - 1, "=", 1)), (hit(FAR + v - 1, "=", 1), None)):
            p = len(pairs)
            reads += [read(b"p%d/1" % p, 1, p), read(b"p%d/2" % p, 1, p + 1)]
            hits += [h1, h2]
            pairs.append({"proper": p % 2, "span": 0})
    kat = {"flags": ["PAIRED"], "K": 1, "reads": reads, "hits": hits, "pairs": pairs}
    return EmitCase("pos_pnext", "POS and PNEXT of 1 to 10 digits on forward, reverse and unplaced lines; ref_start above 2^40",
                    WIDE_CONTIGS, kat)


def tlen():
    reads, hits, pairs = [], [], []
    a = FAR  # the contig's first base: a span of 2 999 999 999 still ends inside it

    def pair(h1, h2):
        p = len(pairs)
        reads.extend([read(b"t%d/1" % p, max(h1["xlen"], 1) if h1 else 3, p), read(b"t%d/2" % p, max(h2["xlen"], 1) if h2 else 3, p + 1)])
        hits.extend([h1, h2])
        pairs.append({"proper": (p + 1) % 2, "span": 0})
    for v in SPANS:
        if v == 0:  # two empty alignments at one place: equal starts, a span of 0
            pair(hit(a, "", 0), hit(a, "", 1))
            pair(hit(a, "", 1), hit(a, "", 0))
            continue
        left, right = a, a + v - 1
        pair(hit(left, "=", 0), hit(right, "=", 1))    # mate 1 leftmost: forward +v, reverse -v (v = 1: equal starts)
        pair(hit(right, "=", 1), hit(left, "=", 0))    # mate 2 leftmost
        pair(hit(left, "=", 1), hit(right, "=", 0))    # reverse +v, forward -v
        pair(hit(left, "=", 0), hit(left, "=", 1, ref_end=left + v))  # equal starts: mate 1 positive, mate 2 negative
    pair(hit(a, "=", 0), None)                          # TLEN 0 on a placed and on an unplaced line
    pair(hit(a, "=", 1), hit(WIDE_CONTIGS[0][1] + 4, "=", 0))  # both placed, two contigs: 0
    kat = {"flags": ["PAIRED"], "K": 1, "reads": reads, "hits": hits, "pairs": pairs}
    return EmitCase("tlen", "TLEN +-span for every span of 0 to 10 digits on either strand; equal starts", WIDE_CONTIGS, kat)


def as_xs():
    n = len(SCORES)
    lo = WIDE_CONTIGS[0][1]
    extra = [(read(b"nx%d" % s, 5), hit(lo + 9, "=====", s, score=-9), None) for s in (0, 1)]  # XS absent while AS is negative
    return two_slots("as_xs", "AS and XS of every width and sign; XS absent beside a negative AS", WIDE_CONTIGS, SCORES,
                     lambda v, s: hit(lo + 20, "====", s, score=v), [],
                     multi=lambda v, i, b: {"mapq": 30, "sub_score": SCORES[(i + 1 + b) % n]}, extra=extra)


def mapq(with_multi=True):
    lo = WIDE_CONTIGS[0][1]
    return two_slots("mapq" if with_multi else "mapq_255", "MAPQ 0 ... 254 from multi records" if with_multi else "MAPQ 255 without multi records",
                     WIDE_CONTIGS, MAPQS, lambda v, s: hit(lo + 30 + v, "===", s), [],
                     multi=(lambda v, i, b: {"mapq": v, "sub_score": 3}) if with_multi else None)


def nm():
    lo = WIDE_CONTIGS[0][1]
    return two_slots("nm", "NM of 1 to 4 digits", WIDE_CONTIGS, NMS, lambda v, s: hit(lo + 10, "=" + "X" * v + "=", s), ["NM"])


def cigar():
    def make(r, s):
        return hit(FAR + 10**6 + r, "=" * r + "X" + "D" * r + "=" + "I" * r + "X" * r, s, score=-r, xstart=r, tail=r)
    long_read = (read(b"run65535", 65_535, 3), hit(FAR + 5, "=" * 65_535, 0, score=65_535), None)
    return two_slots("cigar", "CIGAR runs and soft clips of 1 to 5 digits at either end; one run of 65 535 (a line above 130 KB)", WIDE_CONTIGS,
                     RUNS, make, ["NM"], extra=[long_read])


MD_EXTRA = ["XX", "=D=", "=" + "D" * 100 + "=", "=XD=", "=DX="]


def md():
    at = MD_CONTIGS[1][1] + 3
    values = ["X" + "=" * r + "X" for r in RUNS] + MD_EXTRA
    return two_slots("md", "MD counters of 1 to 5 digits between two mismatches, 0 between adjacent ones, ^ runs of 1 and 100, a deletion "
                     "behind a mismatch and a mismatch behind a deletion", MD_CONTIGS, values, lambda v, s: hit(at, v, s), ["NM", "MD"],
                     text=md_text())


STATES = (None, 0, 1)  # unplaced, forward, reverse


def flag_paired():
    reads, hits, pairs, dup = [], [], [], []
    lo, far = WIDE_CONTIGS[0][1], FAR
    for s1 in STATES:
        for s2 in STATES:
            for proper in (0, 1):
                for apart in (False, True):  # both mates on one contig, or on two (0x2 must stay clear)
                    if apart and (s1 is None or s2 is None):
                        continue
                    for d1, d2 in zip(DUPS, DUPS[1:] + DUPS[:1]):
                        p = len(pairs)
                        reads += [read(b"f%d/1" % p, 4, p), read(b"f%d/2" % p, 4, p + 2)]
                        hits += [None if s1 is None else hit(lo + 40, "====", s1), None if s2 is None else hit((far if apart else lo) + 90, "====", s2)]
                        pairs.append({"proper": proper, "span": 54})
                        dup += [d1, d2]
    kat = {"flags": ["PAIRED"], "K": 1, "reads": reads, "hits": hits, "pairs": pairs}
    return EmitCase("flag_paired", "every FLAG of a paired line; 0x400 driven by dup bytes 0, 1, 0x7e, 255", WIDE_CONTIGS, kat, dup=dup)


def flag_secondary():
    reads, hits, dup = [], [], []
    lo = WIDE_CONTIGS[0][1]
    for s0 in STATES:
        for s1 in STATES:
            for d in DUPS:
                reads.append(read(b"s%d" % len(reads), 4, len(reads)))
                hits += [None if s0 is None else hit(lo + 40, "====", s0), None if s1 is None else hit(lo + 70, "====", s1)]
                dup.append(d)
    kat = {"flags": ["SECONDARY"], "K": 2, "reads": reads, "hits": hits}
    return EmitCase("flag_secondary", "every FLAG of an unpaired line, primary and secondary, with and without 0x400", WIDE_CONTIGS, kat, dup=dup)


def expected_flags(paired):
    """every FLAG the rule of include/biogpu.h can produce, with dup given"""
    out = set()
    if not paired:
        for k in (0, 1):
            for own in STATES:
                if k and own is None:
                    continue
                base = (0x100 if k else 0) | (0x4 if own is None else 0) | (0x10 if own == 1 else 0)
                out |= {base} | ({base | 0x400} if own is not None else set())
        return out
    for first in (0x40, 0x80):
        for own in STATES:
            for mate in STATES:
                base = 0x1 | first | (0x4 if own is None else 0) | (0x10 if own == 1 else 0) | (0x8 if mate is None else 0) | (0x20 if mate == 1 else 0)
                for proper in ((0, 0x2) if own is not None and mate is not None else (0,)):
                    out |= {base | proper} | ({base | proper | 0x400} if own is not None else set())
    return out


LONG_ID = b"q" * 253
IDS_SINGLE = [b"", b"x", b"/1", b"a/1", LONG_ID + b"/1", b"z" * 255]
IDS_MATE1 = [b"", b"x", b"/1", b"/2", b"a/1", b"a/2", LONG_ID + b"/1", LONG_ID + b"/2", b"z" * 255]
IDS_MATE2 = [b"", b"x", b"/2", b"/1", b"a/2", b"a/1", LONG_ID + b"/2", LONG_ID + b"/1", b"z" * 255]


def qname(paired):
    reads, hits = [], []
    lo = WIDE_CONTIGS[0][1]
    ids = list(zip(IDS_MATE1, IDS_MATE2)) if paired else [(i,) for i in IDS_SINGLE]
    for rot in range(3):  # every id on a forward, a reverse and an unplaced line
        for j, group in enumerate(ids):
            for m, id_ in enumerate(group):
                s = STATES[(rot + j + m) % 3]
                reads.append(read(id_, 5, j))
                hits.append(None if s is None else hit(lo + 10 + j, "=====", s))
    kat = {"flags": ["PAIRED"] if paired else [], "K": 1, "reads": reads, "hits": hits,
           "pairs": [{"proper": 1, "span": 0}] * (len(reads) // 2) if paired else None}
    return EmitCase("qname_paired" if paired else "qname_single", "ids of 0, 1, 2, 3 and 255 bytes" +
                    ("; /1 goes from mate 1 and /2 from mate 2 only, and only behind a longer id" if paired else "; /1 stays"), WIDE_CONTIGS, kat)


def rname():
    reads, hits, pairs = [], [], []
    starts = [c[1] for c in NAME_CONTIGS]
    places = [(c, s) for c in (0, 1, 2) for s in (0, 1)] + [None]
    for p1 in places:
        for p2 in places:
            p = len(pairs)
            reads += [read(b"n%d/1" % p, 3, p), read(b"n%d/2" % p, 3, p + 1)]
            hits += [None if pl is None else hit(starts[pl[0]] + 17 + 3 * m, "===", pl[1]) for m, pl in enumerate((p1, p2))]
            pairs.append({"proper": p % 2, "span": 0})
    kat = {"flags": ["PAIRED"], "K": 1, "reads": reads, "hits": hits, "pairs": pairs}
    return EmitCase("rname", "RNAME and RNEXT names of 1 and 200 bytes, own, borrowed from the mate, and =", NAME_CONTIGS, kat)


# ---- the writer: the staging limit ---------------------------------------------------------------------------------------
def _one_line(rd, h, flags, contigs, text):
    kat = {"flags": flags, "K": 1, "reads": [rd], "hits": [h]}
    f, K, fq, hits, strand, ops, _, _ = kat_arrays(kat)
    return so.lines(contigs, fq, hits, strand, ops, f, K, None, None, text)[0]


def _fit(length, placed, salt, text):
    """(read, hit) whose line under NM | MD on MD_CONTIGS has exactly `length` bytes: an unplaced line, or a placed
    reverse-strand one with all tags; the bases give two bytes each, the id the rest"""
    at = MD_CONTIGS[1][1] + 50 + salt
    for n in range((length - 18) // 2, 0, -1):
        h = hit(at, "=" * (n - 5) + "X" + "====", 1, score=-(100 + salt), xstart=0) if placed else None
        base = len(_one_line(read(b"i", n, salt), h, ["NM", "MD"], MD_CONTIGS, text))
        if base <= length:
            assert length - base <= 40
            return read(b"i" * (1 + length - base), n, salt), h
    raise AssertionError(length)


def _filler(id_len):
    return read(b"f" * id_len, 0), None  # "ff\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n": id_len + 22 bytes


def _at_residues(targets, name, covers):
    """targets: [(residue, length, placed)].  In front of every target a filler line whose id length puts the target at the
    residue, computed from the oracle's line lengths."""
    text = md_text().tobytes()
    reads, hits, at, where = [], [], 0, []
    for i, (res, length, placed) in enumerate(targets):
        rd, h = _filler(1)
        base = len(_one_line(rd, h, ["NM", "MD"], MD_CONTIGS, text))
        id_len = 1 + (res - (at + base)) % 16
        rd, h = _filler(id_len)
        reads.append(rd)
        hits.append(h)
        at += base + id_len - 1
        assert at % 16 == res
        rd, h = _fit(length, placed, i, text)
        reads.append(rd)
        hits.append(h)
        where.append(len(reads) - 1)
        at += length
    kat = {"flags": ["NM", "MD"], "K": 1, "reads": reads, "hits": hits}
    case = EmitCase(name, covers, MD_CONTIGS, kat, md_text())
    case.targets = where
    return case


def staging_limit():
    targets = [(res, total - res, placed) for res in range(16) for total in (STAGE, STAGE + 1) for placed in (False, True)]
    return _at_residues(targets, "staging_limit", "for every residue 0 ... 15 a line with residue + length == 1040 and one with == 1041, "
                        "each as an unplaced line and as a placed reverse-strand line with all tags")


def stage_1024():
    targets = [(0, length, placed) for length in (1023, 1024, 1025, 1026) for placed in (False, True)]
    return _at_residues(targets, "stage_1024", "lines of 1023 ... 1026 bytes at residue 0")


# ---- the writer: grid and group edges ------------------------------------------------------------------------------------
def grid(n_reads, K):
    """K = 1: n_reads slots, every third read unplaced.  K = 8 with secondary lines: slot 0 of a read always writes a line, so
    no block is empty; the reads alternate between all eight slots written, slot 0 unplaced (one line, seven placed slots
    that write nothing), slot 0 alone, and a ragged mix; read 32 j - 1 and the last read write one line only, so that the first slot of every
    256-slot block, and the end of the batch, follow empty slots; reads 64 ... 95 give three 256-slot blocks of which only
    every eighth slot writes."""
    at = MD_CONTIGS[2][1]
    reads, hits = [], []
    for r in range(n_reads):
        reads.append(read(b"g%d" % r, 6 + r % 5, r))
        n = len(reads[-1]["seq"])
        own = hit(at + 5 + r % 900, "=" * (n - 2) + "XD=" if r % 2 else "=" * n, r % 2, score=r)
        if K == 1:
            hits.append(None if r % 3 == 1 else own)
            continue
        sec = [hit(at + 7 + (r + k) % 900, "===X==", (r + k) % 2, score=k, xstart=n - 6) for k in range(1, K)]
        kind = 2 if (r % 32 == 31 or r == n_reads - 1 or 64 <= r < 96) else r % 4
        if kind == 0:
            hits += [own] + sec
        elif kind == 1:
            hits += [None] + sec
        elif kind == 2:
            hits += [own] + [None] * (K - 1)
        else:
            hits += [own] + [h if (r + k) % 3 else None for k, h in enumerate(sec)]
    kat = {"flags": ["NM", "MD"] + (["SECONDARY"] if K > 1 else []), "K": K, "reads": reads, "hits": hits}
    return EmitCase("grid_%d_K%d" % (n_reads, K), "%d slots" % (n_reads * K), MD_CONTIGS, kat, md_text())


def nothing_placed():
    reads = [read(b"u%d" % r, r % 7, r) for r in range(40)]
    kat = {"flags": ["NM", "MD", "SECONDARY"], "K": 2, "reads": reads, "hits": [None] * 80}
    return EmitCase("nothing_placed", "no read is placed", MD_CONTIGS, kat, md_text())


def one_empty_read():
    kat = {"flags": ["NM", "MD"], "K": 1, "reads": [read(b"e", 0)], "hits": [None]}
    return EmitCase("one_empty_read", "a single read of length 0", MD_CONTIGS, kat, md_text())


FIELD_CASES = {"pos_pnext": pos_pnext, "tlen": tlen, "as_xs": as_xs, "mapq": mapq, "mapq_255": lambda: mapq(False), "nm": nm, "cigar": cigar,
               "md": md, "flag_paired": flag_paired, "flag_secondary": flag_secondary, "qname_single": lambda: qname(False),
               "qname_paired": lambda: qname(True), "rname": rname}
STAGE_CASES = {"staging_limit": staging_limit, "stage_1024": stage_1024}
GRID_CASES = dict([("grid_%d_K1" % n, functools.partial(grid, n, 1)) for n in GRID_SLOTS] +
                  [("grid_%d_K8" % n, functools.partial(grid, n, 8)) for n in GRID_READS_K8] +
                  [("nothing_placed", nothing_placed), ("one_empty_read", one_empty_read)])
EMIT_CASES = {**FIELD_CASES, **STAGE_CASES, **GRID_CASES}


@functools.lru_cache(maxsize=None)
def emit_case(name):
    return EMIT_CASES[name]()


def staged_pairs(case):
    """{(residue, residue + length, placed)} of the case's target lines"""
    want = case.want()
    off = so.offsets(want)
    return {(int(off[s]) % 16, int(off[s]) % 16 + len(want[s]), not int(fields(want[s])[1]) & 0x4) for s in case.targets}


# ---- the keys ------------------------------------------------------------------------------------------------------------
class KeyBatch:
    def __init__(self, name, seed, n, K=1, paired=False, flags=0, contigs=CONTIGS, p_unmapped=0.1, p_cross=0.1):
        self.name, self.K, self.contigs, self.n = name, K, contigs, n
        self.flags = flags | (so.PAIRED if paired else 0)
        self.fq, self.hits, self.strand = random_batch(random.Random(seed), n, K=K, paired=paired, contigs=contigs, p_unmapped=p_unmapped,
                                                       p_cross=p_cross)

    def counts(self):
        """by direct count from the placement rule: keys borrowed from a placed mate, secondary slots with a key, secondary
        slots without one because slot 0 is unplaced, hits across a contig's end, keys of 2^64 - 1"""
        starts = [c[1] for c in self.contigs]
        slots = [so.Slot(self.hits[s], self.strand[s], starts, self.contigs) for s in range(len(self.hits))]
        c = {"borrowed": 0, "secondary with a key": 0, "secondary behind an unplaced slot 0": 0, "across a contig's end": 0}
        for s, me in enumerate(slots):
            r, k = divmod(s, self.K)
            if self.flags & so.PAIRED and not me.placed and slots[s ^ 1].placed:
                c["borrowed"] += 1
            if k and self.flags & so.SECONDARY and me.placed:
                c["secondary with a key" if slots[r * self.K].placed else "secondary behind an unplaced slot 0"] += 1
            if not me.placed and me.strand != so.HIT_NONE:
                ends = [st + ln for _, st, ln in self.contigs]
                c["across a contig's end"] += any(me.ref_start < e < me.ref_end for e in ends)
        return c


# (seeds 301 ... 314: the floors of tests/test_sam_edge_cases.py hold for them from the oracle alone)
def key_batches():
    S, NM, MD = so.SECONDARY, so.TAG_NM, so.TAG_MD
    return [KeyBatch("single_1", 301, 1), KeyBatch("single_255", 302, 255, p_unmapped=0.5), KeyBatch("single_257", 303, 257, flags=NM),
            KeyBatch("single_2800", 304, 2800, flags=MD), KeyBatch("single_256_unmapped", 305, 256, p_unmapped=1.0),
            KeyBatch("paired_256", 306, 256, paired=True, p_unmapped=0.5), KeyBatch("paired_2800", 307, 2800, paired=True, flags=NM | MD),
            KeyBatch("paired_big", 308, 2800, paired=True, contigs=BIG_CONTIGS, p_unmapped=0.5),
            KeyBatch("paired_2_unmapped", 309, 2, paired=True, p_unmapped=1.0),
            KeyBatch("k4_256", 310, 64, K=4), KeyBatch("k4_2800", 311, 700, K=4, p_unmapped=0.5),
            KeyBatch("k4_secondary_256", 312, 64, K=4, flags=S), KeyBatch("k4_secondary_2800", 313, 700, K=4, flags=S | NM, p_unmapped=0.5),
            KeyBatch("k4_secondary_unmapped", 314, 64, K=4, flags=S, p_unmapped=1.0)]


# ---- the sort ------------------------------------------------------------------------------------------------------------
def record(i, ln):
    """the bytes of sam_sort_cases.synthetic_lines for record i"""
    j = np.arange(ln, dtype=np.uint64)
    return ((i * 7 + j * 13 + (j >> 8) * 5 + (j >> 12)) & 0xFF).astype(np.uint8).tobytes()


class SortBatch:
    """records and keys (below 1990, or 2^64 - 1) in input order"""

    def __init__(self, name, covers, lens, keys):
        self.name, self.covers = name, covers
        self.recs = [record(i, ln) for i, ln in enumerate(lens)]
        self.key = np.array(keys, dtype=np.uint64)
        assert len(self.recs) == len(self.key) and all(k < 1990 or k == TOP for k in keys)

    def placed(self, min_len=LONG_LINE - 1):
        """(length, destination residue, source minus destination residue) of every record of at least min_len bytes"""
        off = so.offsets(self.recs)
        perm, out_off, _ = sso.sort(self.key, self.recs)
        return [(len(self.recs[int(i)]), int(out_off[j]) % 16, (int(off[int(i)]) - int(out_off[j])) % 16)
                for j, i in enumerate(perm) if len(self.recs[int(i)]) >= min_len]

    def hits(self):
        """the keys as hit records on sam_sort_cases.CONTIGS (K = 1, unpaired): sam_rule_key gives `key` back"""
        reads = [read_of(r, 4, 20) for r in range(len(self.key))]
        return arrays(reads, [None if k == TOP else make_hit(40, 0, int(k), int(k) + 1, 0, 4, 4) for k in self.key.tolist()])


def _laid_out(name, covers, longs, drift=5):
    """longs: [(length, destination residue)].  In the output every long record follows a short one that sets its residue;
    in the input a record of `drift` bytes with the top key stands in front of every such pair, so that the source runs
    ahead of the destination by drift, 2 drift, ... bytes."""
    lens, keys, at = [], [], 0
    for g, (length, res) in enumerate(longs):
        pad = (res - at) % 16 or 16
        lens += [drift, pad, length]
        keys += [TOP, 2 * g, 2 * g + 1]
        at += pad + length
    return SortBatch(name, covers, lens, keys)


SWITCH_LENGTHS = (16383, 16384, 16385, 16399, 16400, 16401)
RESIDUES = (0, 1, 8, 15)
CHUNK_DELTAS = (-17, -16, -1, 0, 1, 15, 16, 17)
CHUNK_BASES = (5 * CHUNK, 32 * CHUNK, 33 * CHUNK)


def sort_switch():
    return _laid_out("switch", "lengths around SAM_LONG_LINE at destination residues 0, 1, 8, 15",
                     [(ln, res) for ln in SWITCH_LENGTHS for res in RESIDUES])


def sort_chunk():
    longs = [(b + d, RESIDUES[(i + j) % 4]) for i, b in enumerate(CHUNK_BASES) for j, d in enumerate(CHUNK_DELTAS)]
    return _laid_out("chunk", "5, 32 and 33 chunks of 4096 bytes, 17 bytes either side: the last chunk empty, of one vector, or only a tail", longs,
                     drift=3)


def sort_rows(n_long, seed=9):
    """n_long long records of 16 385 ... 16 500 bytes among short and empty ones, random keys"""
    rng = random.Random(seed + n_long)
    lens = [rng.randint(LONG_LINE + 1, 16_500) for _ in range(n_long)] + [rng.choice((0, 0, 1, 15, 16, 17, 40, 77)) for _ in range(n_long // 2 + 20)]
    rng.shuffle(lens)
    keys = [rng.choice((rng.randrange(1990), rng.randrange(30), TOP)) for _ in lens]
    return SortBatch("rows_%d" % n_long, "%d long records: the row wrap of the long-line kernel's grid at 256" % n_long, lens, keys)


def sort_ends(which):
    lens = [40, 17, 20_000, 0, 33, 5]
    keys = [5, 6, 0 if which == "first" else TOP, 7, 7, 8]
    return SortBatch("long_" + which, "a long record that is the %s of the output" % which, lens, keys)


# ---- duplicate marking ---------------------------------------------------------------------------------------------------
QUAL_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 65_535)
MIN_QUALS = (0, 15)
# below the offset itself, at it, below / at / above offset + 15, far above
LEVELS = (PHRED - 3, PHRED, PHRED + 14, PHRED + 15, PHRED + 16, PHRED + 40)
LAST = (PHRED + 14, PHRED - 3, PHRED + 40)  # the members of a group differ in their last quality only: the third one wins


def qual_lengths():
    """For every length a group of three reads at one coordinate whose qualities are equal but for the last byte — below the
    floor of min_qual 15, below the offset, far above — so that the last member wins, and wins only if the last byte counts."""
    reads, hl = [], []
    for g, n in enumerate(QUAL_LENGTHS):
        body = bytes(LEVELS[(i * 5 + g) % 6] for i in range(n))
        for m in range(3):
            q = body[:-1] + bytes([LAST[m]]) if n else b""
            reads.append((b"q%d_%d" % (n, m), b"A" * n, q))
            hl.append(make_hit(40, g % 2, 100 + 40 * g, 124 + 40 * g, 0, 24, 24))
    return arrays(reads, hl)


def fragments_only(n_pairs=150, seed=21):
    """a paired batch in which every pair has exactly one end"""
    fq, hits, strand = random_batch(random.Random(seed), 2 * n_pairs, paired=True, p_unmapped=0.0, p_cross=0.0, n_coords=6)
    for p in range(n_pairs):
        r = 2 * p + (p * 7 // 3) % 2
        hits[r]["aln"]["score"] = so.MIN_SCORE
        hits[r]["window_start"] = hits[r]["ref_start"] = hits[r]["ref_end"] = TOP
        strand[r] = so.HIT_NONE
    return fq, hits, strand


def md_counter_values(md_string):
    return {int(x) for x in re.findall(rb"[0-9]+", md_string)}
