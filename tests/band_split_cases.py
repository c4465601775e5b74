"""Pairs with hand-made bands that sit on the edges of the banded aligner's interior runs (band_split in
rust-bio_amd/csrc/banded_kernels.h): the run's first and last strip, column 0 and the last column, row shapes on the
traceback's 16-byte groups, gaps and mismatches that cross the border between the two traceback byte layouts
(banded_traceback.hip: in_lo / in_hi), and batches that mix pairs with different runs inside one wavefront.

Generators only: numpy, nothing of the GPU, deterministic by seed.  tests/test_band_split_cases.py proves with the CPU
oracle that every case holds what it is for (and that the constants below still equal the ones in the sources);
tests/test_gpu_banded_split_edges.py runs the cases through Aligner.align_bands_arrays.

A band is n + 1 half-open row ranges start[j]..end[j], one per column of y (row i belongs to x[i - 1]).  Here it is a
stripe around the path of the edit script that made x out of y — `right` cells above and `left` cells below the path's
rows in every column, clamped to [0, m + 1) — with column 0 set to [0, end_0) and column n to [start_n, m + 1), made
monotone by a running maximum of the ends (left to right) and a running minimum of the starts (right to left), so that
both imposed ranges stay exactly what the case asks for."""
import numpy as np

# Copies of the kernels' constants.  test_band_split_cases.py reads the originals out of banded_kernels.h,
# banded_fill2i.hip and banded_fill2p.hip: a constant that moves breaks that test instead of moving the cases off their edge.
STRIP_ROWS = 32    # kSplitStripRows
TB_ROW_ALIGN = 16  # kTbRowAlign: traceback bytes of a row come in groups of this many cells
TB_LINE_ROWS = 8   # kTbLineRows: rows whose groups share a 128-byte line
RING = 32          # K3i / K3p: bytes of LDS per row
FLUSH = 16         # K3i / K3p: steps between two hand-overs of complete groups

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
MIN_SCORE = -858993459

# The scorings that admit interior runs (x kept whole, a real y-prefix clip): (name, mode, scoring).  The last one has no
# price for opening a gap, which K3p's keys do not take: its runs go to K3i alone.
SCORINGS = (
    ("semiglobal-5-1+1-1", "semiglobal", dict(gap_open=-5, gap_extend=-1, match=1, mismatch=-1)),
    ("semiglobal-3-2+2-4", "semiglobal", dict(gap_open=-3, gap_extend=-2, match=2, mismatch=-4)),
    ("custom-yclips-3-2", "custom", dict(gap_open=-4, gap_extend=-1, match=3, mismatch=-2, yclip_prefix=-3, yclip_suffix=-2)),
    ("custom-yprefix0", "custom", dict(gap_open=-6, gap_extend=0, match=1, mismatch=-3, yclip_prefix=0, yclip_suffix=MIN_SCORE)),
    ("semiglobal-open0", "semiglobal", dict(gap_open=0, gap_extend=-1, match=1, mismatch=-1)),
)


class Case:
    """name, x, y, start[], end[] and what the case states about itself: has_run, s_a, s_b (0 where band_split leaves
    before it computes them; the name carries both) and meta (family-specific: rows of the gaps / mismatches, the row
    shape; no_answer_without_y_suffix_clip: the reference has no alignment when yclip_suffix is MIN_SCORE)"""

    def __init__(self, name, x, y, start, end, has_run, s_a, s_b, **meta):
        self.name = name + (f":a{s_a}b{s_b}" if s_a else ":early")  # (early: band_split returns before s_a and s_b)
        self.x = np.ascontiguousarray(x, dtype=np.uint8).tobytes()
        self.y = np.ascontiguousarray(y, dtype=np.uint8).tobytes()
        self.start = np.ascontiguousarray(start, dtype=np.uint32)
        self.end = np.ascontiguousarray(end, dtype=np.uint32)
        self.has_run, self.s_a, self.s_b = has_run, s_a, s_b
        self.meta = meta

    @property
    def m(self):
        return len(self.x)

    @property
    def n(self):
        return len(self.y)

    @property
    def strips(self):
        """strips of the interior run (0 without one)"""
        return self.s_b - self.s_a if self.has_run else 0

    @property
    def kind(self):
        """Z: empty x; N: no run; O: a run of one strip; L: a longer run"""
        if self.m == 0:
            return "Z"
        return "N" if not self.has_run else "O" if self.strips == 1 else "L"

    def __repr__(self):
        return f"Case({self.name}, m={self.m}, n={self.n})"


# ---- band_split and the row view of a band, restated
def split_of(start, end, m):
    """(has_run, s_a, s_b) of band_split (banded_kernels.h) for a band of n + 1 column ranges; s_a = s_b = 0 where it
    returns before computing them"""
    n = len(start) - 1
    start_n = int(start[n])
    if m < 2 or start_n < 1:
        return False, 0, 0
    cols_m = [j for j in range(n + 1) if int(start[j]) <= m < int(end[j])]  # row m's band cells
    if not cols_m or cols_m[-1] < 1:
        return False, 0, 0
    rows0 = int(end[0]) if int(end[0]) > int(start[0]) else 0
    s_a = max(1, (rows0 + STRIP_ROWS - 1) // STRIP_ROWS)
    s_b = min((start_n - 1) // STRIP_ROWS, (m - 1) // STRIP_ROWS)
    return s_a < s_b, s_a, s_b


def rows_of(start, end, m):
    """per row i = 0..m the columns inside the band: (cf, cl, cells); cf > cl for a row outside it.  cells == cl - cf + 1
    on every row is what the device layout needs (one interval per row)."""
    s = np.asarray(start, dtype=np.int64)
    e = np.asarray(end, dtype=np.int64)
    out = []
    for i in range(m + 1):
        cols = np.nonzero((s <= i) & (i < e))[0]
        out.append((int(cols[0]), int(cols[-1]), len(cols)) if len(cols) else (1, 0, 0))
    return out


def monotone(start, end):
    """Band::monotone: starts and ends of the non-empty columns never decrease"""
    ne = [(int(s), int(e)) for s, e in zip(start, end) if e > s]
    return all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(ne, ne[1:]))


# ---- one pair from an edit script
def _other(rng, *avoid):
    """a base different from all of `avoid`"""
    return rng.choice([b for b in _ACGT if b not in avoid])


def make_pair(rng, m, a, left, right, end_0, start_n, subs=(), ins=(), dels=(), n_sub=0, keep_clear=()):
    """x of m bases out of y[a:]: row r of `subs` substituted, (r, k) of `ins`: rows r .. r + k - 1 are inserted bases,
    (r, k) of `dels`: k bases of y deleted behind row r (the D run lies on row r); n_sub more substitutions on random rows at
    least 6 rows from every event and outside the row ranges (lo, hi) of keep_clear.  The inserted and the deleted
    segment differ from their neighbours at both ends, so that the gap cannot slide.  y ends with x (column n holds row m).
    Returns (x, y, start, end)."""
    ins_rows = {r + t: (r, k) for r, k in ins for t in range(k)}
    del_at = dict(dels)
    n = a + m - len(ins_rows) + sum(del_at.values())
    y = _ACGT[rng.integers(0, 4, size=n)].copy()
    x = np.zeros(m, dtype=np.uint8)
    lo = np.full(n + 1, m + 1, dtype=np.int64)   # rows of the path in each column
    hi = np.full(n + 1, -1, dtype=np.int64)

    def touch(i, j):
        lo[j] = min(lo[j], i)
        hi[j] = max(hi[j], i)

    j = a
    touch(0, a)
    for i in range(1, m + 1):
        if i in ins_rows:
            x[i - 1] = 0  # filled below
        else:
            j += 1
            x[i - 1] = y[j - 1]
        touch(i, j)
        if i in del_at:
            k = del_at[i]
            # y[j .. j + k) is deleted: deleting y[j - 1 .. j + k - 1) or y[j + 1 .. j + k + 1) instead must not give the same x
            after = y[j + k] if j + k < n else 0
            y[j] = _other(rng, after, y[j - 1] if k == 1 else 0)
            if k > 1:
                y[j + k - 1] = _other(rng, y[j - 1])
            for t in range(k):
                j += 1
                touch(i, j)
    assert j == n
    # x again (the deleted segments' ends have moved y), then the inserted bases and the substitutions
    j = a
    for i in range(1, m + 1):
        if i not in ins_rows:
            j += 1
            x[i - 1] = y[j - 1]
        j += del_at.get(i, 0)
    for r, k in ins:
        seg = _ACGT[rng.integers(0, 4, size=k)].copy()
        before, behind = (x[r - 2] if r >= 2 else 0), (x[r + k - 1] if r + k - 1 < m else 0)
        seg[0] = _other(rng, behind, before if k == 1 else 0)  # the segment one row later / earlier is another x
        if k > 1:
            seg[-1] = _other(rng, before)
        x[r - 1:r - 1 + k] = seg
    events = [r for r in subs] + [r + t for r, k in ins for t in (0, k - 1)] + [r for r, _ in dels]
    blocked = set(ins_rows)
    for e in events:
        blocked.update(range(e - 6, e + 7))
    for lo_r, hi_r in keep_clear:
        blocked.update(range(lo_r, hi_r + 1))
    free = [i for i in range(2, m) if i not in blocked]
    extra = rng.choice(free, size=min(n_sub, len(free)), replace=False) if n_sub and free else []
    for r in list(subs) + [int(v) for v in extra]:
        x[r - 1] = _other(rng, x[r - 1])
    # the stripe around the path; columns before the path continue its diagonal upwards
    for jj in range(a):
        lo[jj] = hi[jj] = jj - a
    start = np.clip(lo - right, 0, m + 1)
    end = np.clip(hi + left + 1, 0, m + 1)
    return (x, y) + impose(start, end, m, end_0, start_n)


def impose(start, end, m, end_0, start_n):
    """column 0 = [0, end_0), column n = [start_n, m + 1), then monotone"""
    start, end = start.copy(), end.copy()
    start[0], end[0] = 0, end_0
    start[-1], end[-1] = start_n, m + 1
    end = np.maximum.accumulate(end)
    start = np.minimum.accumulate(start[::-1])[::-1]
    empty = end <= start
    start[empty], end[empty] = m + 1, 0  # (what Band::new leaves in a column nothing was added to)
    if start_n >= m + 1:
        start[-1], end[-1] = start_n, 0
    return start, end


# ---- family 1: the run's borders
END_0 = (0, 1, 31, 32, 33, 64, 65)
START_N = (64, 65, 66, 96, 97)
RB_M = (64, 65, 96, 97, 128, 129)
# what the rule gives for each of them, written out by hand (split_of is checked against these)
S_A_OF_END_0 = {0: 1, 1: 1, 31: 1, 32: 1, 33: 2, 64: 2, 65: 3}
S_B_OF_START_N = {64: 1, 65: 2, 66: 2, 96: 2, 97: 3}
S_B_OF_M = {64: 1, 65: 2, 96: 2, 97: 3, 128: 3, 129: 4}


def run_borders():
    """END_0 x START_N x RB_M where the last column's range fits (start_n <= m + 1; with start_n == m + 1 column n is empty
    and (m - 1) / 32 alone binds), and pairs that have no run for another reason: start_n == 0, row m inside column 0
    only, an x of one base, two empty x."""
    out = []
    for t, (e0, sn, m) in enumerate((e0, sn, m) for e0 in END_0 for sn in START_N for m in RB_M):
        if sn > m + 1:
            continue
        rng = np.random.default_rng([201, t])
        a = 6 + t % 5
        ins, dels = ([(20 + t % 7, 1)], [(44 + t % 9, 1)]) if t % 3 else ([], [(30 + t % 11, 2)])
        x, y, st, en = make_pair(rng, m, a, 5, 6, e0, sn, ins=ins, dels=dels, n_sub=4)
        s_a, s_b = S_A_OF_END_0[e0], min(S_B_OF_START_N[sn], S_B_OF_M[m])
        out.append(Case(f"rb.e{e0}.s{sn}.m{m}", x, y, st, en, s_a < s_b, s_a, s_b, end_0=e0, start_n=sn))
    rng = np.random.default_rng([202])
    x, y, st, en = make_pair(rng, 100, 7, 5, 6, 1, 0, n_sub=5)
    out.append(Case("rb.start_n0", x, y, st, en, False, 0, 0, end_0=1, start_n=0))
    # row m inside the band of column 0 and of no other column: every other column is empty
    x, y = _ACGT[rng.integers(0, 4, size=70)], _ACGT[rng.integers(0, 4, size=40)]
    st, en = np.full(41, 71), np.zeros(41, dtype=np.int64)
    st[0], en[0] = 0, 71
    # (no path reaches (m, n) inside such a band: with yclip_suffix = MIN_SCORE the reference panics, whatever m and n)
    out.append(Case("rb.row_m_in_column0_only", x, y, st, en, False, 0, 0, end_0=71, start_n=71,
                    no_answer_without_y_suffix_clip=True))
    x, y, st, en = make_pair(rng, 1, 40, 3, 3, 1, 1)
    out.append(Case("rb.m1", x, y, st, en, False, 0, 0, end_0=1, start_n=1))
    out.append(empty_x(rng, 50, "rb.m0.n50"))
    out.append(empty_x(rng, 33, "rb.m0.n33"))
    return out


def empty_x(rng, n, name):
    """x of no base: row 0 in every column"""
    return Case(name, np.zeros(0, dtype=np.uint8), _ACGT[rng.integers(0, 4, size=n)], np.zeros(n + 1), np.ones(n + 1),
                False, 0, 0, end_0=1, start_n=0)


# ---- family 2: row shapes inside a run
WIDTHS = (1, 15, 16, 17, 31, 32, 33)
CF_RESIDUES = (0, 1, 15)
SHAPE_GEOM = dict(m=160, end_0=1, start_n=150, s_a=1, s_b=4)    # run rows 33 .. 128
LONG_GEOM = dict(m=320, end_0=65, start_n=300, s_a=3, s_b=9)    # run rows 97 .. 288
JUMPS = ((130, 17), (200, 40))  # (row, columns cf moves right between this row and the next)
HOLD = (150, 20)                # cf stays where it is on the 20 rows behind this one


def row_shapes():
    """Rows of WIDTHS cells whose first column is 0, 1 and 15 mod 16 on the run's first row (left != right for the even
    widths); a stripe whose first column jumps by 17 and by 40 columns from one row to the next (x lacks 16 and 39
    bases of y there); a stripe that keeps its first column for 20 rows (x has 20 more)."""
    out = []
    g = SHAPE_GEOM
    in_lo = g["s_a"] * STRIP_ROWS + 1
    for w in WIDTHS:
        left = w // 2
        right = w - 1 - left
        for r in CF_RESIDUES:
            rng = np.random.default_rng([203, w, r])
            a = (r - in_lo + left) % TB_ROW_ALIGN  # cf(i) = i + a - left on rows the edit script has not shifted
            while a < left + 2:
                a += TB_ROW_ALIGN
            gaps = dict(dels=[(146, 2)], ins=[(153, 1)]) if w >= 15 else {}  # (behind the run: its rows keep their width)
            x, y, st, en = make_pair(rng, g["m"], a, left, right, g["end_0"], g["start_n"], n_sub=5,
                                     keep_clear=[(in_lo - 2, in_lo + 2)], **gaps)
            out.append(Case(f"shape.w{w}.cf{r}", x, y, st, en, True, g["s_a"], g["s_b"], width=w, residue=r, left=left))
    g = LONG_GEOM
    left, right = 6, 7
    rng = np.random.default_rng([204])
    x, y, st, en = make_pair(rng, g["m"], 11, left, right, g["end_0"], g["start_n"], n_sub=8,
                             dels=[(r - left, d - 1) for r, d in JUMPS])
    out.append(Case("shape.jumps", x, y, st, en, True, g["s_a"], g["s_b"], jumps=JUMPS))
    x, y, st, en = make_pair(rng, g["m"], 11, left, right, g["end_0"], g["start_n"], n_sub=8,
                             ins=[(HOLD[0] - left + 1, HOLD[1])])
    out.append(Case("shape.hold", x, y, st, en, True, g["s_a"], g["s_b"], hold=HOLD))
    return out


# ---- family 3: moves across the border between the two traceback layouts
MOVE_GEOMS = (dict(tag="g1", m=160, end_0=1, start_n=140, s_a=1, s_b=4),   # run rows 33 .. 128
              dict(tag="g2", m=160, end_0=40, start_n=100, s_a=2, s_b=3))  # a run of one strip: rows 65 .. 96
INS_LEN, DEL_LEN = 4, 5


def border_moves():
    """per geometry: four inserted rows in_lo - 2 .. in_lo + 1, four inserted rows in_hi - 1 .. in_hi + 2, a deletion whose
    D run lies on row in_lo - 1, in_lo, in_hi, in_hi + 1 (one pair each), mismatches on rows in_lo and in_hi"""
    out = []
    for gi, g in enumerate(MOVE_GEOMS):
        in_lo, in_hi = g["s_a"] * STRIP_ROWS + 1, g["s_b"] * STRIP_ROWS
        specs = [("ins_lo", dict(ins=[(in_lo - 2, INS_LEN)])), ("ins_hi", dict(ins=[(in_hi - 1, INS_LEN)]))]
        specs += [(f"del_row{r}", dict(dels=[(r, DEL_LEN)])) for r in (in_lo - 1, in_lo, in_hi, in_hi + 1)]
        specs += [("subst", dict(subs=[in_lo, in_hi]))]
        for si, (tag, ev) in enumerate(specs):
            rng = np.random.default_rng([205, gi, si])
            x, y, st, en = make_pair(rng, g["m"], 9, 7, 7, g["end_0"], g["start_n"], n_sub=4, **ev)
            out.append(Case(f"move.{g['tag']}.{tag}", x, y, st, en, True, g["s_a"], g["s_b"], in_lo=in_lo, in_hi=in_hi,
                            ins_rows=[r + t for r, k in ev.get("ins", []) for t in range(k)],
                            del_rows=[r for r, _ in ev.get("dels", [])], sub_rows=list(ev.get("subs", []))))
    return out


# ---- family 4: wavefront mixes
# N: no run, O: a run of one strip, L: a longer run (in turn the longest one, strips 3 .. 8, and one from strip 1),
# Z: an empty x.  Pairs 2g and 2g + 1 share K3p's registers: over all batches every ordered couple of the four kinds
# occurs, and the odd batches leave their last pair without a partner.  Eight consecutive pairs share a wavefront's strip
# loop: every full group holds N, O and the longest run, its smallest s_a and its largest s_b on different pairs.
MIXES = {1: "O", 2: "LZ", 7: "NOOLZNL", 8: "NLLOZZON", 9: "LLNNOOZLO", 17: "LNOZZONZLONLZLONL"}


def wavefront_mixes(borders=None, shapes=None, moves=None):
    """{batch size: [Case]} drawn from the three families above"""
    borders = borders or run_borders()
    shapes = shapes or row_shapes()
    moves = moves or border_moves()
    pool = {"N": [c for c in borders if c.kind == "N"][::7] + [c for c in borders if c.name.startswith("rb.start_n0")],
            "O": [c for c in borders if c.kind == "O" and c.s_a == 1][::5] + [c for c in moves if c.kind == "O"][::3],
            "LB": [c for c in shapes if c.s_b == LONG_GEOM["s_b"]],
            "LA": [c for c in moves if c.kind == "L"] + [c for c in shapes if c.kind == "L" and c.s_a == 1][::4],
            "Z": [c for c in borders if c.kind == "Z"]}
    taken = {k: 0 for k in pool}
    out = {}
    for size, kinds in MIXES.items():
        assert len(kinds) == size
        batch, longs = [], 0
        for kd in kinds:
            if kd == "L":
                kd = "LB" if longs % 2 == 0 else "LA"
                longs += 1
            batch.append(pool[kd][taken[kd] % len(pool[kd])])
            taken[kd] += 1
        out[size] = batch
    return out


def admitted(cases, kw):
    """the cases the reference has an answer for under this scoring"""
    return [c for c in cases if not (c.meta.get("no_answer_without_y_suffix_clip") and kw.get("yclip_suffix", 0) == MIN_SCORE)]


def orders(batch):
    """the batch as it is, reversed, and rotated by one: partners and lane groups change"""
    return {"asis": list(batch), "reversed": list(batch[::-1]), "rotated": list(batch[1:]) + list(batch[:1])}


def one_row_short(borders=None):
    """the pairs of the run-border family that miss a run by one row: s_a == s_b"""
    return [c for c in (borders or run_borders()) if not c.has_run and c.m >= 2 and c.s_a == c.s_b and c.s_a > 0]


def concat(cases):
    """(x, x_off, y, y_off, band_off, start, end) of a batch, as Aligner.align_bands_arrays takes them"""
    def cat(parts, dtype):
        off = np.zeros(len(parts) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(p) for p in parts])
        flat = np.concatenate([np.frombuffer(p, dtype=dtype) if isinstance(p, bytes) else p for p in parts]) if parts else np.zeros(0, dtype)
        return np.ascontiguousarray(flat, dtype=dtype), off
    x, xo = cat([c.x for c in cases], np.uint8)
    y, yo = cat([c.y for c in cases], np.uint8)
    st, bo = cat([c.start for c in cases], np.uint32)
    en, _ = cat([c.end for c in cases], np.uint32)
    return x, xo, y, yo, bo, st, en
