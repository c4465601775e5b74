"""Seed-and-extend on reads beyond 150 bases (include/biogpu.h, bg_seed_extend_*), for tests/test_gpu_seed_extend_long.py and its
CPU companion tests/test_oracle_seed_extend_long.py.

One random genome of 300 kbp with a two-copy repeat of 2400 bases whose copies differ every 97 bases.  A class is a longest read
length L and a pad (the candidate window is y = L + 2 pad) chosen so that plan_fill (sw_api.hip, restated by sw_fill of
tests/test_gpu_score_edges.py) takes one given road for the candidate alignments; CLASSES names the fill family of each and
`fill_of` derives it.  (The strip hand-over is two classes: F512, every read in one strip, and F513, reads of 513 and 512 bases
in a call of two strips.)  Every class holds the same kinds of reads, drawn from the genome with their edits planted:

  exact, subs       the read as it stands in the text; 5 .. 10 % substitutions
  del_*, ins_*      one deletion (min(24, pad) bases: a deletion longer than pad does not fit the window) or one insertion (24
                    bases) in the first, middle and last strip of the read.  The seeds on one side of the indel are broken (a
                    substitution every 15 bases), so that the read has one candidate: seeds on both sides would propose two
                    starts more than pad / 2 apart whose windows both hold the alignment, a tie by construction
  left0, left2      starts 0 and 2: the window is clipped at the text's first base
  right0, right3    the read ends at, and 3 before, the text's last base: the window is clipped at n_text
  over_right        the read's last 4 bases hang over the text's end (they are inserted)
  over_left         the read's first 3 bases hang over the text's start: every proposal is negative, dropped but counted
  rev, rev_subs     from the reverse strand
  rep_a, rep_b      inside the repeat: two candidates with distinct scores
  random            no hit
  short             (ragged class) shorter than a seed, a read of 1

Implied scores are under (gap_open, gap_extend, match, mismatch) = (go, -1, 1, -1): matches - substitutions + go - (indel length
- 1), the oracle's cost of a gap.  Under class W's gap_open of -9000 no alignment opens a gap it can avoid: its indel and
overhanging reads are placed (within the indel's length of the planted locus) without a stated score."""
import functools

import numpy as np

from rescue_cases import flat_of, other_base
from rust_bio_amd import synth
from rust_bio_amd.alphabets import dna
from rust_bio_amd.bwt import bwt, less
from rust_bio_amd.suffix_array import suffix_array
from test_gpu_score_edges import F, sw_fill

ALPHA = b"ACGTNacgtn$"
SC = (-5, -1, 1, -1)
SC_WIDE = (-9000, -1, 1, -1)
N_TEXT = 300_000
SEED_LEN = 20
MAX_OCC = 16
REP_A, REP_B, REP_LEN = 100_000, 200_000, 2400
REP_DIFF = np.arange(48, REP_LEN, 97)  # copy B differs from copy A here
INDEL = 24
MAX_SPAN = 1000
OP_M, OP_S, OP_D, OP_I = 0, 1, 2, 3

# class -> longest read, pad, the fill family of its candidate alignments
CLASSES = {
    "A": dict(L=192, pad=16, fill="K1P"),           # last length of K1p's 16-lane shape
    "B": dict(L=193, pad=16, fill="K1P"),           # first length of its 32-lane shape
    "C": dict(L=384, pad=11, fill="K1P"),           # y = 406: 5 * 408 = 2040, K1p exactly at its bound
    "D": dict(L=384, pad=12, fill="K1_NARROW"),     # y = 408: 5 * 410 = 2050, one step past
    "E": dict(L=385, pad=16, fill="K1_NARROW"),     # first length of K1's 64-lane kernel, one strip
    "F512": dict(L=512, pad=16, fill="K1_NARROW"),  # the last length of one strip (64 lanes x 8 rows)
    "F513": dict(L=513, pad=16, fill="K1_NARROW", lengths=(513, 512)),  # two strips, reads of 512 among them
    "G": dict(L=1500, pad=32, fill="K1_NARROW", ragged=True),
    "H": dict(L=2049, pad=32, fill="K1_NARROW", few=True),  # five strips
    "W": dict(L=1500, pad=32, fill="K1_WIDE", sc=SC_WIDE),  # 9000 * (1500 + 1564 + 8) >= 2^24
}
PAIR_CLASSES = ("B", "E", "F513")
G_LENGTHS = (10, 19, 1, 20, 21, 192, 193, 384, 385, 512, 513, 45, 100, 777, 1024, 1025, 1499)


def scoring_kw(sc):
    return dict(gap_open=sc[0], gap_extend=sc[1], match=sc[2], mismatch=sc[3])


def fill_of(sc, max_x, max_y):
    """the family plan_fill gives a semiglobal call of these longest lengths"""
    return sw_fill(scoring_kw(sc), "semiglobal", None, max_x, max_y)


def seed_params(L):
    """(seed_len, stride, max_occ): the smallest stride with at most 64 slots at L; slots * max_occ <= 1024"""
    stride = max(1, -(-(L - SEED_LEN) // 63))
    slots = (L - SEED_LEN) // stride + 1
    assert slots <= 64 and slots * MAX_OCC <= 1024
    return SEED_LEN, stride, MAX_OCC


for _name, _c in CLASSES.items():  # each class lands where the table says, one on each side of each switch
    assert fill_of(_c.get("sc", SC), _c["L"], _c["L"] + 2 * _c["pad"]) == F[_c["fill"]], _name
assert CLASSES["C"]["pad"] + 1 == CLASSES["D"]["pad"] and CLASSES["A"]["L"] + 1 == CLASSES["B"]["L"]
assert CLASSES["D"]["L"] + 1 == CLASSES["E"]["L"] and CLASSES["F512"]["L"] + 1 == CLASSES["F513"]["L"]


def revcomp(x):
    return np.frombuffer(dna.revcomp(np.ascontiguousarray(x).tobytes()), np.uint8)


@functools.lru_cache(maxsize=None)
def genome():
    g = synth.random_dna(N_TEXT, seed=2024).copy()
    g[REP_B:REP_B + REP_LEN] = g[REP_A:REP_A + REP_LEN]
    g[REP_B + REP_DIFF] = other_base(g[REP_B + REP_DIFF])
    g.setflags(write=False)
    text = np.append(g, np.uint8(ord("$")))
    text.setflags(write=False)
    return g, text


@functools.lru_cache(maxsize=None)
def index():
    """(suffix array, BWT, less) of the text, once"""
    _, text = genome()
    sa = suffix_array(text)
    b = bwt(text, sa)
    return sa, b, less(b, ALPHA)


class Read:
    """x: the bases; kind; s / e: where its alignment starts and ends in the text (None: no placement expected); strand: 0
    forward, 1 reverse; score: what its edits imply (None: not stated, and s / e hold to within INDEL bases); indel: (operation
    kind, length) planted"""

    def __init__(self, x, kind, s=None, e=None, strand=0, score=None, indel=None):
        self.x, self.kind, self.s, self.e, self.strand, self.score, self.indel = np.ascontiguousarray(x, np.uint8), kind, s, e, strand, score, indel


def break_seeds(x, lo, hi):
    """a substitution every 15 bases of x[lo .. hi): no 20-base window inside holds none.  Returns how many"""
    pos = np.arange(lo + 7, hi, 15)
    x[pos] = other_base(x[pos])
    return len(pos)


class Maker:
    def __init__(self, name, seed):
        c = CLASSES[name]
        self.name, self.L, self.pad, self.sc = name, c["L"], c["pad"], c.get("sc", SC)
        self.go = self.sc[0]
        self.stride = seed_params(self.L)[1]
        self.g, _ = genome()
        self.rng = np.random.default_rng(seed)
        self.n_random = 0

    def locus(self, span):
        """a start away from the repeat and the text's ends"""
        zones = ((3000, REP_A - 3000), (REP_A + 5000, REP_B - 3000), (REP_B + 5000, N_TEXT - 6000))
        lo, hi = zones[int(self.rng.integers(0, 3))]
        return int(self.rng.integers(lo, hi - span))

    def exact(self, L, s=None, kind="exact"):
        s = self.locus(L) if s is None else s
        return Read(self.g[s:s + L], kind, s, s + L, score=L)

    def subs(self, L, rate, kind="subs"):
        s = self.locus(L)
        x = self.g[s:s + L].copy()
        k = max(1, int(round(rate * L)))
        while True:  # drawn again until a seed slot of the class holds no substitution
            pos = self.rng.choice(np.arange(1, L - 1), size=k, replace=False)
            hit = np.zeros(L, bool)
            hit[pos] = True
            if any(not hit[o:o + SEED_LEN].any() for o in range(0, L - SEED_LEN + 1, self.stride)):
                break
        x[pos] = other_base(x[pos])
        return Read(x, kind, s, s + L, score=L - 2 * k)

    def places(self, L):
        """read offsets in the first, middle and last strip (512 rows) of a read, and the side whose seeds are broken"""
        if L <= 512:
            return (("first", 60, "left"), ("middle", L // 2, "right"), ("last", L - 60 - INDEL, "right"))
        return (("first", 150, "left"), ("middle", (L // 1024) * 512 + 200 if L >= 1024 else L // 2, "right"),
                ("last", L - 150, "right"))

    def dele(self, L, where, at, side):
        d = min(INDEL, self.pad)
        s = self.locus(L + d)
        ref = self.g[s:s + L + d]
        x = np.concatenate([ref[:at], ref[at + d:]])
        nb = break_seeds(x, 0, at) if side == "left" else break_seeds(x, at, L)
        score = L - 2 * nb + self.go - (d - 1) if self.sc == SC else None
        return Read(x, "del_" + where, s, s + L + d, score=score, indel=(OP_D, d))

    def ins(self, L, where, at, side):
        d = INDEL
        s = self.locus(L)
        ref = self.g[s:s + L - d]
        self.n_random += 1
        x = np.concatenate([ref[:at], synth.random_dna(d, seed=7000 + 100 * sum(map(ord, self.name)) + self.n_random), ref[at:]])
        nb = break_seeds(x, 0, at) if side == "left" else break_seeds(x, at + d, L)
        score = L - d - 2 * nb + self.go - (d - 1) if self.sc == SC else None
        return Read(x, "ins_" + where, s, s + L - d, score=score, indel=(OP_I, d))

    def random(self, L, kind="random"):
        self.n_random += 1
        return Read(synth.random_dna(L, seed=9000 + 100 * sum(map(ord, self.name)) + self.n_random), kind)

    def ends(self, L):
        g, n = self.g, N_TEXT
        tail = other_base(g[n - 4:n][::-1].copy())
        return [self.exact(L, 0, "left0"), self.exact(L, 2, "left2"), self.exact(L, n - L, "right0"), self.exact(L, n - L - 3, "right3"),
                Read(np.concatenate([g[n - L + 4:n], tail]), "over_right", n - L + 4, n,
                     score=L - 4 + self.go - 3 if self.sc == SC else None),
                Read(np.concatenate([other_base(g[:3][::-1].copy()), g[:L - 3]]), "over_left")]

    def rev(self, rd, kind):
        return Read(revcomp(rd.x), kind, rd.s, rd.e, strand=1, score=rd.score)

    def repeat(self, L, copy, kind):
        o = int(self.rng.integers(0, REP_LEN - L + 1))
        base = REP_A if copy == 0 else REP_B
        return Read(self.g[base + o:base + o + L], kind, base + o, base + o + L, score=L)


def single_reads(name):
    c = CLASSES[name]
    L = c["L"]
    mk = Maker(name, seed=1000 + sum(map(ord, name)))
    lens = c.get("lengths", (L,))
    k = [0]

    def nl():  # the class's lengths in turn
        k[0] += 1
        return lens[(k[0] - 1) % len(lens)]

    if c.get("few"):  # at most 8 reads
        pl = mk.places(L)
        return [mk.exact(L), mk.subs(L, 0.07), mk.dele(L, *pl[2]), mk.ins(L, *pl[0]), mk.rev(mk.subs(L, 0.05), "rev_subs"),
                mk.repeat(L, 0, "rep_a"), mk.exact(L, N_TEXT - L, "right0"), mk.random(L)]
    out = [mk.exact(L)] + [mk.exact(nl()) for _ in range(3)]
    out += [mk.subs(nl(), r) for r in (0.05, 0.06, 0.07, 0.08, 0.09, 0.10)]
    for fn in (mk.dele, mk.ins):
        for _ in range(len(lens)):
            for where, at, side in mk.places(lens[0]):
                out.append(fn(nl(), where, at, side))
    out += mk.ends(L)
    out += [mk.rev(mk.exact(nl()), "rev") for _ in range(3)] + [mk.rev(mk.subs(nl(), 0.07), "rev_subs") for _ in range(3)]
    out += [mk.repeat(nl(), 0, "rep_a"), mk.repeat(nl(), 1, "rep_b"), mk.repeat(L, 0, "rep_a"), mk.repeat(L, 1, "rep_b")]
    out += [mk.random(nl()) for _ in range(3)]
    if c["fill"] == "K1P":
        # K1p pairs its jobs by length once a sub-batch holds 64 of them: more repeat reads (two candidates each) and
        # reads shorter than L, so that the couples are ragged
        out += [mk.repeat(L, k % 2, "rep_a" if k % 2 == 0 else "rep_b") for k in range(16)]
        out += [mk.exact(n) for n in (L - 1, L - 37, 150, 97)] + [mk.subs(n, 0.06) for n in (L - 2, L - 64, 151, 120)]
    if c.get("ragged"):
        for n in G_LENGTHS:
            out.append(mk.exact(n, kind="exact" if n >= SEED_LEN else "short"))
            out[-1].score = n if n >= SEED_LEN else None
            if n < SEED_LEN:
                out[-1].s = out[-1].e = None
        out += [mk.subs(int(n), 0.06) for n in mk.rng.integers(600, L, size=6)]
        out += [mk.rev(mk.exact(int(n)), "rev") for n in (230, 640)]
        order = mk.rng.permutation(len(out))  # lengths from 1 to 1500 next to each other
        out = [out[i] for i in order]
    return out


class Case:
    """One class's batch: reads (flat, off), the Read objects, its parameters."""

    def __init__(self, name, rds):
        c = CLASSES[name]
        self.name, self.L, self.pad, self.sc = name, c["L"], c["pad"], c.get("sc", SC)
        self.seed_len, self.stride, self.max_occ = seed_params(self.L)
        self.items = rds
        self.reads, self.off = flat_of([r.x for r in rds])
        self.fill = F[c["fill"]]
        assert int(np.diff(self.off).max()) == self.L

    @property
    def seed_kw(self):
        return dict(seed_len=self.seed_len, stride=self.stride, max_occ=self.max_occ, pad=self.pad)

    def of_kind(self, *prefix):
        return [r for r, it in enumerate(self.items) if it.kind.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def case(name):
    c = Case(name, single_reads(name))
    n = len(c.items)
    assert (n <= 8) if CLASSES[name].get("few") else (30 <= n <= 60), (name, n)
    return c


# ------------------------------------------------------------------------------------------------------------------ pairs


def mate_subs(mk, x, k):
    x = x.copy()
    pos = mk.rng.choice(np.arange(25, len(x) - 25), size=k, replace=False)
    x[pos] = other_base(x[pos])
    return x


@functools.lru_cache(maxsize=None)
def pair_case(name):
    """Interleaved mates of class `name`: 2x250-style fragments (max_span 1000), fragments shorter than a mate (the mates overlap
    completely), a mate with broken seeds (rescue aligns it against a window of max_span), a random mate, a fragment at the text's
    end.  info[p] = (kind, fragment start, fragment length, the seed-broken or random read of the pair or None)"""
    c = CLASSES[name]
    L = c["L"]
    lens = c.get("lengths", (L,))
    mk = Maker(name, seed=5000 + sum(map(ord, name)))
    g = mk.g
    frag = min(MAX_SPAN, int(2.6 * L))
    reads, info = [], []

    def add(kind, a, f, l1, l2, swap, spoil=None):
        m1 = g[a:a + l1]
        ref2 = g[a + f - l2:a + f].copy()
        bad = None
        if spoil == "broken":
            break_seeds(ref2, 0, l2)
        elif spoil == "random":
            ref2 = mk.random(l2).x
        else:
            m1, ref2 = mate_subs(mk, m1, 2), mate_subs(mk, ref2, 3)
        pair = [m1, revcomp(ref2)]
        if spoil:
            bad = 0 if swap else 1
        reads.extend(pair[::-1] if swap else pair)
        info.append((kind, a, f, bad))

    for k in range(6):
        add("frag", mk.locus(frag), frag - 7 * k, L, lens[k % len(lens)], k % 2 == 1)
    for k, f in enumerate((L - 40, L - 1, L // 2)):
        add("overlap", mk.locus(L), f, f, f, k % 2 == 1)
    for k in range(4):
        add("broken", mk.locus(frag), frag - 11 * k, lens[k % len(lens)], L, k % 2 == 1, "broken")
    add("random", mk.locus(frag), frag, L, L, False, "random")
    add("end", N_TEXT - frag, frag, L, L, False)
    add("end_broken", N_TEXT - frag, frag, L, L, True, "broken")
    cs = Case(name, [Read(x, "mate") for x in reads])
    cs.info = info
    assert 30 <= len(reads) <= 60
    return cs


# ----------------------------------------------------------------------------------------------- the oracle's answers, once


def _orc():
    import oracle_py as orc
    return orc


@functools.lru_cache(maxsize=None)
def oracle_single(name):
    """orc.seed_extend_batch on the class's reads: (hits, ops, ops stride)"""
    orc = _orc()
    c, (g, text), (sa, b, ls) = case(name), genome(), index()
    return orc.seed_extend_batch(b, ls, orc.Occ(b, 64, ALPHA), sa, text, N_TEXT, orc.make_scoring(*c.sc), c.reads, c.off, threads=8,
                                 **c.seed_kw)


@functools.lru_cache(maxsize=None)
def oracle_both(name):
    """the joined oracle of both strands: (hits, strand, ops, ops stride)"""
    from test_gpu_seed_extend_strands import oracle_strands
    c, (g, text), (sa, b, ls) = case(name), genome(), index()
    return oracle_strands(b, ls, sa, text, N_TEXT, c.reads, c.off, scores=c.sc, **c.seed_kw)


@functools.lru_cache(maxsize=None)
def candidates(name, paired=False):
    """every candidate of every virtual read (read r: 2r forward, 2r + 1 its revcomp), and the voting hits (pair_oracle)"""
    import pair_oracle as po
    orc = _orc()
    c, (g, text), (sa, b, ls) = (pair_case if paired else case)(name), genome(), index()
    vr, voff = po.virtual_reads(c.reads, c.off)
    cands, nh = po.candidates(orc, b, ls, orc.Occ(b, 64, ALPHA), sa, text, N_TEXT, orc.make_scoring(*c.sc), vr, voff, **c.seed_kw)
    return cands, nh, vr, voff
