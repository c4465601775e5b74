"""SMEM-seeded seed-and-extend cases whose hit counts are set by construction (include/biogpu.h, bg_seed_extend_smem_batch), for
tests/test_gpu_seed_extend_smem_edges.py and its CPU companion tests/test_oracle_seed_extend_smem_edges.py.

A random genome T of a few hundred kbp.  An edge read is random DNA of its own: pieces of PIECE = min_seed_len + 1 bases with
one separator base between neighbours.  Copies of its pieces are planted in T; the bases next to a planted piece differ from
the read's separators there, so a planted piece is an SMEM of exactly PIECE bases and no SMEM spans two pieces.  A piece of the
read planted in T is a suffix-array row in the T half of T$R$; a piece of revcomp(read) planted in T is a row of the read in
the R half.  The records' interval sizes count both, and so does max_occ.

Plantings go through `Genome`, which hands out T from left to right and keeps a strand's proposed starts more than GAP > pad
apart unless a case asks for a cluster.  A whole copy (`Genome.copy`) holds every piece of the read with the separators
changed: all its pieces propose the same start.  The last bases of T stay as drawn: the ordinary reads and the reads at T's
ends are cut from them.

Three batches: "s64" (max_smems 64 x max_occ 16) and "s32" (32 x 32), each with the count cases (distinct, stacked, split
between the halves, truncated at the limit), the reads at the ends of T and ordinary reads, heavy reads in the middle and at
the very end; and "merge", the reads whose proposals lie pad / 2 and pad / 2 + 1 apart, for every pad of PADS.

`restate` derives every read's rows per half, dropped proposals and kept starts from smem_seed_oracle.records and the suffix
array alone, with the header's conditions written out again; `corpus()` builds everything once and asserts that every case
has exactly the record count, rows per half and kept starts it was built for (no retries: a miss is a bug of this file).

The read T[n_t - 40 .. n_t) $ R[0 .. 40): the oracle answers it without a panic (one record, one row at n_t - 40, across the
sentinel and so in neither half): it stays an ordinary case with no hit and no candidate."""
import functools

import numpy as np

import fmd_cases as fc
import oracle_py as orc
import smem_seed_oracle as sso
from rust_bio_amd.suffix_array import suffix_array

F, R = sso.HIT_FORWARD, sso.HIT_REVERSE
MIN_SEED_LEN = 19
PIECE = MIN_SEED_LEN + 1
STEP = PIECE + 1   # a piece and the separator after it
GAP = 27           # between a strand's proposed starts where a case wants them apart: more than the largest pad
PADS = (25, 24, 1, 0)
N_TEXT = 640_000
HEAD = 1_500       # no planting before it: every proposal p - a is a start >= 0
PLAIN = 12_000     # the last bases of T are never planted
NH_VALUES = (0, 1, 63, 64, 65, 127, 128, 129, 512, 513, 1023, 1024)
SHAPES = {"s64": dict(max_smems=64, max_occ=16), "s32": dict(max_smems=32, max_occ=32)}
SPLITS = ((700, 324), (1, 1023), (1023, 1))
CHUNK = 8          # the device flavour's pass size that puts a boundary before one heavy read and after another
END_L = 100        # length of the reads at the ends of T


def revcomp(x):
    return np.frombuffer(fc.revcomp(np.ascontiguousarray(x).tobytes()), np.uint8)


def other(b):
    return np.uint8(fc.other_base(int(b)))


class Read:
    """an edge read of P pieces; view[F] is the read, view[R] its reverse complement (piece k of the read is piece P - 1 - k of it)"""

    def __init__(self, x, P):
        self.x, self.P = x, P
        self.view = {F: x, R: revcomp(x)}
        self.last = {F: None, R: None}  # the strand's last start handed out by Genome.next_start


class Genome:
    def __init__(self, n=N_TEXT, seed=211):
        self.n = n
        self.g = np.frombuffer(fc.random_dna(n, seed), np.uint8).copy()
        self.core = np.zeros(n, bool)    # bases of planted pieces
        self.flank = np.zeros(n, bool)   # bases set to differ from a separator
        self.cur = HEAD                  # everything before it is taken
        self.read_seed = seed * 1000

    def new_read(self, P):
        self.read_seed += 1
        return Read(np.frombuffer(fc.random_dna(P * STEP - 1, self.read_seed), np.uint8).copy(), P)

    def _flank(self, at, sep):
        v = other(sep)
        assert not self.core[at] and (not self.flank[at] or self.g[at] == v)
        self.g[at], self.flank[at] = v, True

    def plant(self, rd, h, k, s):
        """piece k of view h so that the view starts at s: a proposal of s on strand h"""
        x, a = rd.view[h], k * STEP
        p = s + a
        assert s >= 0 and p + PIECE < self.n - PLAIN and not self.core[p:p + PIECE].any() and not self.flank[p:p + PIECE].any()
        self.g[p:p + PIECE] = x[a:a + PIECE]
        self.core[p:p + PIECE] = True
        if a > 0:
            self._flank(p - 1, x[a - 1])
        if a + PIECE < len(x):
            self._flank(p + PIECE, x[a + PIECE])
        self.cur = max(self.cur, p + PIECE + 1)

    def next_start(self, rd, h, a=0):
        """the next start of view h whose planting at view offset a is free and which is GAP after the strand's last"""
        p = self.cur + 1
        if rd.last[h] is not None:
            p = max(p, rd.last[h] + GAP + a)
        rd.last[h] = p - a
        return p - a

    def single(self, rd, h, k):
        """one piece on its own: a start no other planting of the read proposes"""
        self.plant(rd, h, k, self.next_start(rd, h, k * STEP))

    def copy(self, rd, h, skip=(), only=None):
        """the whole view h at one start (its separators changed), without the pieces `skip` / with the pieces `only` alone"""
        s = self.next_start(rd, h)
        for k in range(rd.P) if only is None else only:
            if k not in skip:
                self.plant(rd, h, k, s)
        self.cur = max(self.cur, s + len(rd.x) + 1)
        return s

    def cluster(self, rd, h, deltas, k0=0):
        """pieces k0, k0 + 1, .. of view h proposing s + deltas (ascending); returns s"""
        s = self.next_start(rd, h, k0 * STEP)
        for i, d in enumerate(deltas):
            self.plant(rd, h, k0 + i, s + d)
        rd.last[h] = s + deltas[-1]
        return s


# ----------------------------------------------------------------------------------------------------------- the cases


def case(kind, x, records, rows_f, rows_r, kept_f, kept_r, starts=None, **more):
    """what a read was built for (pad 25, both strands): record count, rows per half (nh: all the rows its voting records
    resolve), kept starts per strand (counts; `starts`: the starts themselves, (forward list, reverse list))"""
    return dict(kind=kind, x=np.ascontiguousarray(x), records=records, rows_f=rows_f, rows_r=rows_r, kept_f=kept_f, kept_r=kept_r,
                starts=starts, **more)


def distinct(G, P, nh):
    """nh hits, every one a start of its own; every third hit on the reverse strand"""
    rd = G.new_read(P)
    n = [0, 0]
    for i in range(nh):
        k = i % P  # (round i // P plants piece k once more)
        h = R if i % 3 == 2 else F
        G.single(rd, h, k if h == F else P - 1 - k)
        n[h] += 1
    return case("distinct", rd.x, min(nh, P), n[F], n[R], n[F], n[R], nh=nh)


def stacked(G, P, nh):
    """whole copies, every third on the reverse strand; nh % P == 1: one piece more, at the smallest start; nh % P == P - 1:
    the first copy lacks a piece — the runs of equal keys then lie across the blocks of 64"""
    rd = G.new_read(P)
    n, kept = [0, 0], [0, 0]
    if nh % P == 1:
        G.copy(rd, F, only=[P // 2])
        n[F], kept[F] = 1, 1
    for j in range((nh + 1) // P):
        h = R if j % 3 == 1 else F
        skip = (5,) if nh % P == P - 1 and j == 0 else ()
        G.copy(rd, h, skip=skip)
        n[h] += P - len(skip)
        kept[h] += 1
    assert n[F] + n[R] == nh
    return case("stacked", rd.x, P, n[F], n[R], kept[F], kept[R], nh=nh)


def split(G, P, cap, nf, nr):
    """nf rows in the T half and nr in the R half: whole copies and, for the rest, pieces on their own"""
    rd = G.new_read(P)
    assert nf // P + nr // P + (1 if nf % P + nr % P else 0) <= cap and nf % P + nr % P <= P
    for _ in range(nf // P):
        G.copy(rd, F)
    for _ in range(nr // P):
        G.copy(rd, R)
    for k in range(nf % P):
        G.single(rd, F, k)
    for k in range(nf % P, nf % P + nr % P):
        G.single(rd, R, P - 1 - k)
    return case("split", rd.x, P, nf, nr, nf // P + nf % P, nr // P + nr % P, nh=nf + nr)


def truncated(G, P, cap):
    """P + 1 pieces with `cap` whole copies each: the first P records in push order make P x cap hits, the last one is cut"""
    rd = G.new_read(P + 1)
    for j in range(cap):
        G.copy(rd, R if j % 2 else F)
    nf = (cap + 1) // 2
    return case("truncated", rd.x, P + 1, nf * P, (cap - nf) * P, nf, cap - nf, nh=P * cap, truncated=True)


def end_reads(G):
    """reads at the first and last bases of T and hanging over them by 10 bases and by one, each with its reverse complement"""
    t, n, L = G.g, G.n, END_L
    junk = np.frombuffer(fc.random_dna(10, 77), np.uint8).copy()
    out = []

    def both(kind, x, hit, start):
        """hit: the read's one row lies in a half; start: the forward start it proposes there (None: dropped)"""
        kf = [] if start is None else [start]
        out.append(case(kind, x, 1, int(hit), 0, len(kf), 0, starts=(kf, [])))
        out.append(case(kind + "/rc", revcomp(x), 1, 0, int(hit), 0, len(kf), starts=([], kf)))

    both("head", t[:L], True, 0)                           # p = 0 = a; revcomp: p + len = 2 n_t + 1, q + L = n_t + a
    both("tail", t[n - L:], True, n - L)                   # p + len = n_t; revcomp: p = n_t + 1
    for j in (10, 1):
        jk = junk[:j].copy()
        both("over_head_%d" % j, np.concatenate([jk, t[:L - j]]), True, None)          # p = 0 < a = j; revcomp: q + L = n_t + a + j
        both("over_tail_%d" % j, np.concatenate([t[n - L + j:], jk]), True, n - L + j)  # kept, the window clipped at n_t
    jk = junk.copy()
    jk[-1] = other(t[9])
    both("at_head", np.concatenate([jk, t[10:L]]), True, 0)                             # p = a = 10: s = 0
    jk = junk.copy()
    jk[0] = other(t[n - 10])
    both("at_tail", np.concatenate([t[n - L:n - 10], jk]), True, n - L)                 # the read ends at n_t with its junk
    r0 = revcomp(t)[:40]
    x = np.concatenate([t[n - 40:], np.frombuffer(b"$", np.uint8), r0])
    assert (revcomp(x) == x).all()  # its own reverse complement, through the sentinel
    out.append(case("sentinel", x, 1, 0, 0, 0, 0, starts=([], []), rows_none=1))
    return out


def ordinary_reads(G, count, seed):
    """reads of 100 - 150 bases from the unplanted end of T: exact, with substitutions, every other one reverse complemented"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        L = int(rng.integers(100, 151))
        s = int(rng.integers(G.n - PLAIN + 200, G.n - 400 - L))
        x = G.g[s:s + L].tobytes()
        if i % 3 == 1:
            x = fc.substituted(x, 31)
        x = np.frombuffer(x, np.uint8)
        out.append(dict(kind="ordinary", x=revcomp(x) if i % 2 else x.copy(), truth=(R if i % 2 else F, s)))
    return out


def count_batch(G, name):
    """the count cases of one shape, the reads at T's ends and ordinary reads; a 1024-hit read first in a pass of CHUNK reads,
    another last in one, a third at the very end of the batch"""
    P, cap = SHAPES[name]["max_smems"], SHAPES[name]["max_occ"]
    small = P // 4  # pieces of the distinct reads up to 129 hits (their records then hold up to 129 / small rows each)
    edge = [distinct(G, small if nh else 4, nh) for nh in NH_VALUES if nh <= 129]
    edge += [stacked(G, P, nh) for nh in (512, 513, 1023, 1024)]
    edge += [split(G, P, cap, nf, nr) for nf, nr in SPLITS]
    edge.append(truncated(G, P, cap))
    heavy = [distinct(G, P, 1024), stacked(G, P, 1024), split(G, P, cap, 512, 512)]
    return edge, heavy


def arrange(edge, heavy, ends, plain):
    """edge and ordinary reads in turn; heavy[0] at index CHUNK (first of a pass), heavy[1] at 3 CHUNK - 1 (last of one),
    heavy[2] last of all, at an index that ends a short pass"""
    rest, k = [], 0
    for i, c in enumerate(edge + ends):
        rest.append(c)
        if i % 2 == 0 and k < len(plain):
            rest.append(plain[k])
            k += 1
    rest += plain[k:]
    rest.insert(CHUNK, heavy[0])
    rest.insert(3 * CHUNK - 1, heavy[1])
    if len(rest) % CHUNK == CHUNK - 1:
        rest.append(dict(plain[0]))
    rest.append(heavy[2])
    assert rest[CHUNK] is heavy[0] and rest[3 * CHUNK - 1] is heavy[1] and rest[-1] is heavy[2] and len(rest) % CHUNK
    return rest


def merge_batch(G):
    """proposals pad / 2 and pad / 2 + 1 apart for pad / 2 = 12 and 0, chains, both strands; equal and near starts across the
    strands.  `kept`: {pad: (forward, reverse)} kept starts relative to nothing — counts."""
    out = []
    P = 8
    for h in (F, R):
        o = R if h == F else F

        def kept(nf):  # {pad: (forward count, reverse count)} from the count on strand h
            return {pad: ((n, 0) if h == F else (0, n)) for pad, n in nf.items()}

        rd = G.new_read(P)  # 12 apart: merged at pad 25 and 24; 13 apart: kept
        G.cluster(rd, h, (0, 12))
        G.cluster(rd, h, (0, 13), k0=2)
        out.append(case("gap_12_13", rd.x, 4, *((4, 0) if h == F else (0, 4)), 0, 0, kept=kept({25: 3, 24: 3, 1: 4, 0: 4})))
        rd = G.new_read(P)  # a chain: each start is compared with the last one kept, not with the one before it
        G.cluster(rd, h, (0, 12, 24, 36, 48))
        out.append(case("chain_12", rd.x, 5, *((5, 0) if h == F else (0, 5)), 0, 0, kept=kept({25: 3, 24: 3, 1: 5, 0: 5})))
        rd = G.new_read(P)  # equal starts merge whatever the pad; one apart is kept when pad / 2 = 0
        G.cluster(rd, h, (0, 0))
        G.cluster(rd, h, (0, 1), k0=2)
        G.cluster(rd, h, (0, 0, 0), k0=4)
        G.cluster(rd, h, (0, 1, 2), k0=0)
        out.append(case("gap_0_1", rd.x, 7, *((10, 0) if h == F else (0, 10)), 0, 0, kept=kept({25: 4, 24: 4, 1: 7, 0: 7})))
        rd = G.new_read(P)  # strand h at s, the other strand 5 further: both kept, at every pad
        s = G.cluster(rd, h, (0,))
        G.plant(rd, o, 2, s + 5)
        rd.last[o] = s + 5
        out.append(case("strands_5_apart", rd.x, 2, 1, 1, 0, 0, kept={pad: (1, 1) for pad in PADS}))
        rd = G.new_read(P)  # the same start on both strands, of a read that is not its own reverse complement
        s = G.cluster(rd, h, (0,))
        G.plant(rd, o, 2, s)
        rd.last[o] = s
        out.append(case("strands_equal", rd.x, 2, 1, 1, 0, 0, kept={pad: (1, 1) for pad in PADS}))
    # a read equal to its own reverse complement, planted once: one record of two rows, the same start on both strands
    half = np.frombuffer(fc.random_dna(30, 4242), np.uint8)
    pal = np.concatenate([half, revcomp(half)])
    assert (revcomp(pal) == pal).all()
    s = G.cur + 40
    assert not G.core[s - 1:s + 61].any() and not G.flank[s - 1:s + 61].any()
    G.g[s:s + 60] = pal
    G.core[s:s + 60] = True
    G.cur = s + 100
    out.append(case("palindrome", pal, 1, 1, 1, 0, 0, kept={pad: (1, 1) for pad in PADS}, starts=([s], [s])))
    for c in out:
        c["kept_f"], c["kept_r"] = c["kept"][25]
    return out


# ---------------------------------------------------------------------------------------------------------- restatement


def merged(starts, pad):
    kept = []
    for s in sorted(starts):
        if not kept or (s != kept[-1] and s - kept[-1] > pad // 2):
            kept.append(s)
    return kept


def restate(ofmd, sa, n_t, reads, off, min_seed_len, max_smems, max_occ, pad, strands=sso.STRAND_BOTH):
    """per read, from its records and the suffix array: n_records, truncated, panicked, rows {F, R, None: rows of its voting
    records per half / in neither}, dropped {F, R: rows in a half whose start lies outside [0, n_t)}, props and kept {F, R:
    starts}, nh (all the rows), n_seed_hits and n_candidates (of the strands that ran)"""
    out = []
    for r in range(len(off) - 1):
        x = reads[int(off[r]):int(off[r + 1])]
        L = len(x)
        recs = sso.records(ofmd, x, min_seed_len)
        d = dict(panicked=recs is None, n_records=0 if recs is None else len(recs), rows={F: 0, R: 0, None: 0}, dropped={F: 0, R: 0},
                 props={F: [], R: []})
        for lower, size, a, ln in (recs or [])[:max_smems]:
            if size < 1 or size > max_occ:
                continue
            for p in sa[lower:lower + size]:
                p = int(p)
                if p + ln <= n_t:                                 # the T half: read[a ..] at T[p ..]
                    h, s = F, p - a
                elif p >= n_t + 1 and p + ln <= 2 * n_t + 1:      # the R half: read[a ..] at R[q ..], the read over R[q - a, q - a + L)
                    h, s = R, n_t - (p - n_t - 1 - a + L)
                else:
                    h = None
                d["rows"][h] += 1
                if h is not None:
                    if 0 <= s < n_t:
                        d["props"][h].append(s)
                    else:
                        d["dropped"][h] += 1
        ran = [h for h, bit in ((F, sso.STRAND_FORWARD), (R, sso.STRAND_REVERSE)) if strands & bit]
        d["truncated"] = d["n_records"] > max_smems
        d["kept"] = {h: merged(d["props"][h], pad) if h in ran else [] for h in (F, R)}
        d["nh"] = sum(d["rows"].values())
        d["n_seed_hits"] = sum(d["rows"][h] for h in ran)
        d["n_candidates"] = sum(len(d["kept"][h]) for h in ran)
        out.append(d)
    return out


# ---------------------------------------------------------------------------------------------------------- the corpus


class Corpus:
    def __init__(self):
        G = Genome()
        parts = {name: count_batch(G, name) for name in SHAPES}
        merge = merge_batch(G)
        assert G.cur < G.n - PLAIN
        ends = end_reads(G)
        self.cases = {name: arrange(edge, heavy, [dict(c) for c in ends], ordinary_reads(G, 24, 5 + len(name) + i))
                      for i, (name, (edge, heavy)) in enumerate(parts.items())}
        self.cases["merge"] = merge + ordinary_reads(G, 6, 9)
        self.fwd = G.g
        self.n_t = G.n
        self.text = np.frombuffer(fc.full_text(G.g.tobytes()), np.uint8)
        self.sa = np.asarray(suffix_array(self.text), np.uint64)
        self.bwt = np.frombuffer(bytes(orc.bwt(self.text, self.sa)), np.uint8)
        self.less = np.asarray(orc.less(self.bwt, fc.ALPHA), np.uint64)
        self.ofmd = orc.FMDIndex(self.bwt, self.less, orc.Occ(self.bwt, 3, fc.ALPHA))
        self.reads = {name: fc.concat([c["x"].tobytes() for c in cs]) for name, cs in self.cases.items()}
        self.check()

    def params(self, name, pad=25):
        return dict(min_seed_len=MIN_SEED_LEN, pad=pad, **SHAPES["s64" if name == "merge" else name])

    def restate(self, name, pad=25, strands=sso.STRAND_BOTH):
        return restate(self.ofmd, self.sa, self.n_t, *self.reads[name], strands=strands, **self.params(name, pad))

    def heavy(self, name):
        """indexes of the 1024-hit reads a pass boundary lies next to: (first of a pass of CHUNK, last of one, last of the batch)"""
        return CHUNK, 3 * CHUNK - 1, len(self.cases[name]) - 1

    def check(self):
        """every case is what it was built for"""
        for name, cs in self.cases.items():
            for pad in PADS if name == "merge" else (25,):
                for r, (c, d) in enumerate(zip(cs, self.restate(name, pad))):
                    what = (name, pad, r, c["kind"])
                    assert not d["panicked"], what
                    if c["kind"] == "ordinary":
                        h, s = c["truth"]
                        assert s in d["kept"][h], what
                        continue
                    kf, kr = c["kept"][pad] if "kept" in c else (c["kept_f"], c["kept_r"])
                    got = (d["n_records"], d["rows"][F], d["rows"][R], d["rows"][None], len(d["kept"][F]), len(d["kept"][R]), d["truncated"])
                    want = (c["records"], c["rows_f"], c["rows_r"], c.get("rows_none", 0), kf, kr, c.get("truncated", False))
                    assert got == want, (what, got, want)
                    if "nh" in c:
                        assert d["nh"] == c["nh"], what
                    if c["starts"] is not None:
                        assert (d["kept"][F], d["kept"][R]) == (list(c["starts"][0]), list(c["starts"][1])), what
                    if c["kind"] == "distinct":  # every hit a start of its own, more than the largest pad from the next
                        for h in (F, R):
                            assert len(d["props"][h]) == d["rows"][h] and (np.diff(sorted(d["props"][h])) > max(PADS)).all(), what
        for name in SHAPES:
            i, j, k = self.heavy(name)
            cs = self.cases[name]
            assert [cs[v]["nh"] for v in (i, j, k)] == [1024] * 3 and i % CHUNK == 0 and (j + 1) % CHUNK == 0 and k % CHUNK != CHUNK - 1


@functools.lru_cache(maxsize=None)
def corpus():
    return Corpus()
