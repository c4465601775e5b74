"""The last-column epilogue of K1p's LF flavours (sw_fill_pk16.inc, LF: Aligner::local with gap_open < 0 and mismatch < 0),
which computes and publishes of column n only what a local traceback reads: the score, Lx[n] and the S nibble of (m, n), the
row i* its x-suffix clip jumps to (aux[3]) with that row's S nibble and Ly, and row 0 — no second pass (mod.rs:825-843), no I
nibbles, no other row.  K2 refuses any other column-n entry with BG_ERR_TRACEBACK, so status == 0 everywhere also says
that no valid input asks for one.
  - on the CPU: a model of the reference's fill and traceback that records every cell a walk visits, checked against the
    oracle, shows that a local walk is never in layer I or D in column n and visits there rows {0, i*, m} only, and that the
    second pass changes neither the record nor the operations;
  - on the GPU: records and every operation against the oracle over the geometries, batch shapes, alphabets and constructed
    pairs that decide who owns row m, who owns i*, and which ties the first-maximum rule has to break, on the three cells
    (FR 0, 1, 2) and the 2-bit entry."""
import numpy as np
import pytest

import oracle_py as orc
from rust_bio_amd import _lib
from test_gpu_pk16 import BASE, local_vs_oracle, related_pairs
from test_gpu_pk16_cell3 import packed_equals
from test_gpu_pk16_frame import frame_fits, rows_per_lane
from test_gpu_pk16_max3 import max3_fits

gpu = pytest.mark.gpu
F = _lib.FILL
ALPHA = np.frombuffer(b"ACGT", dtype=np.uint8)
FR1 = dict(gap_open=-5, gap_extend=-1, match=8, mismatch=-8)     # match - mismatch > 15: framed, the v_pk_max_i16 cell
FR0 = dict(gap_open=-12, gap_extend=-10, match=3, mismatch=-2)   # at n = 150 the frame does not fit: the plain LF cell
MIN = -858993459
START, INS, DEL, SUBST, MATCH, XP, XS, YP, YS = range(9)


# ---------------------------------------------------------------- the reference's walk, cell by cell (CPU)

def model_local(kw, x, y, second_pass=True):
    """Aligner::local of the reference (custom with all four clip penalties 0) for one pair, plain Python: returns (score,
    xstart, xend, ystart, yend, operations as orc.decode_ops names them, visited = [(layer, i, j)], i* or
    None)"""
    go, ge, ma, mi = kw["gap_open"], kw["gap_extend"], kw["match"], kw["mismatch"]
    m, n = len(x), len(y)
    S = [[MIN] * (m + 1) for _ in range(2)]
    I = [[MIN] * (m + 1) for _ in range(2)]
    D = [[MIN] * (m + 1) for _ in range(2)]
    tb = [[[START, START, START] for _ in range(n + 1)] for _ in range(m + 1)]  # s, i, d nibbles
    Lx, Ly, Sn = [0] * (n + 1), [0] * (m + 1), [MIN] * (m + 1)
    Sn[0], Ly[0] = 0, n
    for k in range(2):
        S[k][0] = 0
        for i in range(1, m + 1):
            c = [START, START, START]
            if i == 1:
                I[k][i] = go
            else:
                i_score, c_score = go + ge * (i - 1), go
                I[k][i], c[1] = (i_score, INS) if i_score > c_score else (c_score, XP)
            if i == m:
                c[0] = XS
            else:
                S[k][i] = MIN
            if I[k][i] > S[k][i]:
                S[k][i], c[0] = I[k][i], INS
            if 0 > S[k][i]:
                S[k][i], c[0] = 0, XP
            if i != m and S[k][i] > S[k][m]:
                S[k][m], Lx[0] = S[k][i], m - i
            if k == 0:
                tb[i][0] = c
            if S[k][i] > Sn[i]:
                Sn[i], Ly[i] = S[k][i], n
    for j in range(1, n + 1):
        cur, prv = j % 2, 1 - j % 2
        c = [START, START, START]
        I[cur][0] = MIN
        if j == 1:
            D[cur][0] = go
        else:
            d_score, c_score = go + ge * (j - 1), go
            D[cur][0], c[2] = (d_score, DEL) if d_score > c_score else (c_score, YP)
        if D[cur][0] > 0:
            S[cur][0], c[0] = D[cur][0], DEL
        else:
            S[cur][0], c[0] = 0, YP
        if j == n and Sn[0] > S[cur][0]:
            S[cur][0], c[0] = Sn[0], YS
        elif S[cur][0] > Sn[0]:
            Sn[0], Ly[0] = S[cur][0], n - j
        tb[0][j] = c
        for i in range(1, m + 1):
            S[cur][i] = MIN
        xclip = max(0, go + ge * (j - 1))
        for i in range(1, m + 1):
            c = [XS, START, START]
            m_score = S[prv][i - 1] + (ma if x[i - 1] == y[j - 1] else mi)
            i_score, s_score = I[cur][i - 1] + ge, S[cur][i - 1] + go
            best_i, c[1] = (i_score, INS) if i_score > s_score else (s_score, tb[i - 1][j][0])
            d_score, s_score = D[prv][i] + ge, S[prv][i] + go
            best_d, c[2] = (d_score, DEL) if d_score > s_score else (s_score, tb[i][j - 1][0])
            best = S[cur][i]
            if m_score > best:
                best, c[0] = m_score, MATCH if x[i - 1] == y[j - 1] else SUBST
            if best_i > best:
                best, c[0] = best_i, INS
            if best_d > best:
                best, c[0] = best_d, DEL
            if xclip > best:
                best, c[0] = xclip, XP
            yclip = go + ge * (i - 1)
            if yclip > best:
                best, c[0] = yclip, YP
            S[cur][i], I[cur][i], D[cur][i] = best, best_i, best_d
            if S[cur][i] > S[cur][m]:
                S[cur][m], Lx[j] = S[cur][i], m - i
            if S[cur][i] > Sn[i]:
                Sn[i], Ly[i] = S[cur][i], n - j
            tb[i][j] = c
    cur = n % 2
    for i in range(m + 1):
        if Sn[i] > S[cur][i]:
            S[cur][i], tb[i][n][0] = Sn[i], YS
        if S[cur][i] > S[cur][m]:
            S[cur][m], Lx[n], tb[m][n][0] = S[cur][i], m - i, XS
    if second_pass:
        for i in range(1, m + 1):
            s_score = S[cur][i - 1] + go
            if s_score > I[cur][i]:
                I[cur][i], tb[i][n][1] = s_score, tb[i - 1][n][0]
            if s_score > S[cur][i]:
                S[cur][i], tb[i][n][0] = s_score, INS
                if S[cur][i] > S[cur][m]:
                    S[cur][m], Lx[n], tb[m][n][0] = S[cur][i], m - i, XS
    istar = m - Lx[n] if tb[m][n][0] == XS else None
    i, j, ops, visited = m, n, [], []
    xstart, ystart, xend, yend = 0, 0, m, n
    layer = tb[m][n][0]
    while layer != START:
        visited.append((layer, i, j))
        if layer == INS:
            ops.append("I")
            layer, i = tb[i][j][1], i - 1
        elif layer == DEL:
            ops.append("D")
            layer, j = tb[i][j][2], j - 1
        elif layer in (MATCH, SUBST):
            ops.append("M" if layer == MATCH else "S")
            layer, i, j = tb[i - 1][j - 1][0], i - 1, j - 1
        elif layer == XP:
            xstart, i = i, 0
            layer = tb[0][j][0]
        elif layer == XS:
            i -= Lx[j]
            xend, layer = i, tb[i][j][0]
        elif layer == YP:
            ystart, j = j, 0
            layer = tb[i][0][0]
        else:
            j -= Ly[i]
            yend, layer = j, tb[i][j][0]
    return S[n % 2][m], xstart, xend, ystart, yend, ops[::-1], visited, istar


def argument_holds(kw, xs, ys):
    """the model equals the oracle; the walk stays out of layers I / D and off unpublished rows in column n; the second pass
    changes nothing the caller sees"""
    x, xo = _lib.concat(xs)
    y, yo = _lib.concat(ys)
    oout, oops, stride = orc.align_batch(orc.make_scoring(**kw, xclip_prefix=MIN, xclip_suffix=MIN, yclip_prefix=MIN, yclip_suffix=MIN),
                                         "local", x, xo, y, yo, threads=8)
    for p, (a, b) in enumerate(zip(xs, ys)):
        score, xstart, xend, ystart, yend, ops, visited, istar = model_local(kw, a, b)
        want = oout[p]
        assert (score, xstart, xend, ystart, yend) == tuple(int(want[f]) for f in ("score", "xstart", "xend", "ystart", "yend")), (kw, a, b)
        got = orc.decode_ops(oops[p * stride:p * stride + int(want["n_ops"])])
        assert [o for o in got if o in ("M", "S", "D", "I")] == ops, (kw, a, b, got)
        n, m = len(b), len(a)
        for layer, i, j in visited:
            if j == n:
                assert layer not in (INS, DEL), (kw, a, b, layer, i)
                assert i in (0, m, istar), (kw, a, b, layer, i, istar)
        assert model_local(kw, a, b, second_pass=False)[:6] == (score, xstart, xend, ystart, yend, ops), (kw, a, b)


# ---------------------------------------------------------------- inputs

def tails(rng, m, n, alpha=ALPHA):
    """x equals y plus a long unrelated tail, and the mirror image: below the best row the reference's second pass rewrites
    column-n cells (S(i, n) = S(i*, n) + go + ge k beats what the fill left)"""
    xs, ys = [], []
    for core in (n // 2, n - 1, n):
        y = alpha[rng.integers(0, len(alpha), size=n)]
        x = np.concatenate([y[n - core:], alpha[rng.integers(0, len(alpha), size=m)]])[:m]
        xs += [x.tobytes(), y[:m].tobytes() if m <= n else np.resize(y, m).tobytes()]
        ys += [y.tobytes(), np.concatenate([x[:min(m, n) // 2], alpha[rng.integers(0, len(alpha), size=n)]])[:n].tobytes()]
    return xs, ys


def row_m_winners(rng, m, n):
    """the alignment ends at (m, n); at (m, j < n), where Sn[m] wins; at (i < m, n) with no y clip"""
    core = ALPHA[rng.integers(0, 4, size=max(m, n) + 8)]
    k = max(1, min(m, n) - 2)
    xs = [core[:m].tobytes()[-k:].rjust(m, b"N")]                 # x's suffix == y's suffix: ends at (m, n)
    ys = [core[:m].tobytes()[-k:].rjust(n, b"n")]
    xs.append(core[:k].tobytes().rjust(m, b"N"))                   # x's suffix inside y, y goes on: ends at (m, j < n)
    ys.append((core[:k].tobytes() + b"n" * n)[:n] if n > k else core[:n].tobytes())
    xs.append((core[:k].tobytes() + b"N" * m)[:m])                 # y's suffix inside x, x goes on: ends at (i < m, n)
    ys.append(core[:k].tobytes().rjust(n, b"n"))
    return xs, ys


def check(kw, xs, ys, framed, max3, opts=None):
    out, ops, ctx = local_vs_oracle(kw, xs, ys, opts=opts)
    where = (kw, len(xs), len(xs[0]), len(ys[0]))
    assert ctx.last_fill_kernels() == F["K1P_LF"], where
    assert ctx.last_fill_framed() == framed and ctx.last_fill_max3() == max3, where
    return out, ops


def cell_of(kw, xs, ys):
    """(framed, max3) plan_fill gives this batch"""
    mx, my = max(len(x) for x in xs), max(len(y) for y in ys)
    r, lp = rows_per_lane(mx)
    d = 16 * (kw["match"] - kw["mismatch"]) + 2
    return frame_fits(kw, my, r, lp), max3_fits(kw, my, r, lp) and d <= 256


# ---------------------------------------------------------------- CPU: the argument

def test_local_walks_read_only_rows_0_istar_m_of_column_n():
    rng = np.random.default_rng(1)
    for kw in (BASE, FR1, FR0, dict(gap_open=-1, gap_extend=-1, match=2, mismatch=-1)):
        xs, ys = [], []
        for alpha in (ALPHA, ALPHA[:2], ALPHA[:1]):
            for _ in range(400):
                m, n = int(rng.integers(1, 13)), int(rng.integers(1, 13))
                a, b = related_pairs(rng, 1, lambda p: m, lambda p: n, alpha=alpha)
                xs += a
                ys += b
        for m, n in ((9, 20), (20, 9), (11, 11), (24, 30)):
            for a, b in (tails(rng, m, n), tails(rng, m, n, ALPHA[:2]), row_m_winners(rng, m, n)):
                xs += a
                ys += b
        xs += [b"A" * 7, b"A" * 9, b"AC" * 5, b"A", b"", b"ACGT", b"", b"AC", b"A"]
        ys += [b"C" * 9, b"A" * 7, b"GT" * 6, b"A", b"", b"", b"ACGT", b"", b""]
        argument_holds(kw, xs, ys)
    a, b = related_pairs(rng, 6, lambda p: 150, lambda p: 150)
    ta, tb_ = tails(rng, 150, 150)
    argument_holds(BASE, a + ta[:2], b + tb_[:2])


# ---------------------------------------------------------------- GPU

LP16 = [1, 2, 9, 10, 11, 20, 149, 150, 151, 160, 192]
LP32 = [193, 200, 384]


def geometry_batch(rng, m, n):
    xs, ys = related_pairs(rng, 9, lambda p: m, lambda p: n)
    for a, b in (tails(rng, m, n), row_m_winners(rng, m, n)):
        xs += a
        ys += b
    return xs, ys


@gpu
@pytest.mark.parametrize("m", LP16 + LP32)
def test_geometry_row_m_owner_and_unused_lanes(m):
    # m fixes the lane and the row within it that own row m (first, middle, last lane; mrow 0 and R - 1; lanes past m unused),
    # n != m in both directions moves the last column's step
    rng = np.random.default_rng(m)
    group = LP16 if m in LP16 else LP32
    for n in sorted({group[(group.index(m) + 1) % len(group)], group[group.index(m) - 1], m}):
        xs, ys = geometry_batch(rng, m, n)
        check(BASE, xs, ys, *cell_of(BASE, xs, ys))


@gpu
@pytest.mark.parametrize("n_pairs", [1, 3, 4, 5, 9])
def test_batch_shapes_lone_a_missing_b_partial_wavefront(n_pairs):
    rng = np.random.default_rng(n_pairs)
    for m, n in ((150, 150), (11, 20), (200, 193)):
        xs, ys = geometry_batch(rng, m, n)
        check(BASE, xs[-n_pairs:], ys[-n_pairs:], *cell_of(BASE, xs, ys))


@gpu
def test_ragged_batch_runs_single_pair_passes_and_the_permuted_traceback():
    rng = np.random.default_rng(7)
    lens = [150, 149, 150, 151, 20, 150, 1, 160, 150, 11, 150, 2, 192, 150, 9, 10, 150]
    xs, ys = related_pairs(rng, 4 * len(lens), lambda p: lens[p % len(lens)], lambda p: lens[(p * 7) % len(lens)])
    for m, n in ((150, 20), (9, 150), (151, 149)):
        a, b = tails(rng, m, n)
        xs += a
        ys += b
    # empty sequences: with n == 0 column n is column 0, whose own fold (mod.rs:658-661) sends (m, 0) to row 1
    xs += [b"", b"ACGT", b"", b"A", b"AC" * 40, b"AC"]
    ys += [b"", b"", b"ACGT", b"", b"", b""]
    check(BASE, xs, ys, *cell_of(BASE, xs, ys))


@gpu
@pytest.mark.parametrize("m,n", [(150, 150), (20, 11), (200, 384)])
def test_ties_keep_the_first_row_and_the_first_column(m, n):
    # two letters and homopolymers: many rows and columns share the maximum
    rng = np.random.default_rng(m + n)
    xs, ys = related_pairs(rng, 24, lambda p: m, lambda p: n, alpha=ALPHA[:2])
    a, b = tails(rng, m, n, ALPHA[:2])
    xs += a + [b"A" * m, b"A" * m, b"AC" * (m // 2), b"A" * (m - 1) + b"C"]
    ys += b + [b"A" * n, b"A" * (n // 2 + 1), b"AC" * (n // 2), b"C" + b"A" * (n - 1)]
    out, _ = check(BASE, xs, ys, *cell_of(BASE, xs, ys))
    assert out["score"][-4] == min(m, n) and out["score"][-3] == min(m, n // 2 + 1)


@gpu
@pytest.mark.parametrize("m,n", [(150, 150), (10, 9), (193, 200)])
def test_all_mismatch_pairs_score_zero_with_an_empty_alignment(m, n):
    xs = [b"A" * m, b"G" * m, b"AC" * (m // 2), b"A" * m, b"T" * m]
    ys = [b"C" * n, b"T" * n, b"GT" * (n // 2), b"G" * n, b"A" * n]
    out, _ = check(BASE, xs, ys, *cell_of(BASE, xs, ys))
    assert (out["score"] == 0).all() and (out["n_ops"] == 0).all()


@gpu
@pytest.mark.parametrize("m,n", [(150, 150), (149, 151), (11, 20), (200, 193)])
def test_winner_is_row_m_or_a_row_above_without_y_clip(m, n):
    rng = np.random.default_rng(3 * m + n)
    xs, ys = row_m_winners(rng, m, n)
    out, _ = check(BASE, xs * 3, ys * 3, *cell_of(BASE, xs, ys))
    k = max(1, min(m, n) - 2)
    assert out["score"][0] >= k and (out["xend"][0], out["yend"][0]) == (m, n)
    if n > k + 2 and m > k + 2:
        assert out["xend"][1] == m and out["yend"][1] < n
        assert out["xend"][2] < m and out["yend"][2] == n


@gpu
@pytest.mark.parametrize("m,n", [(150, 150), (150, 20), (20, 150), (384, 200)])
def test_pairs_whose_second_pass_rewrites_column_n(m, n):
    rng = np.random.default_rng(m * 5 + n)
    xs, ys = tails(rng, m, n)
    a, b = tails(rng, m, n, ALPHA[:2])
    check(BASE, xs + a, ys + b, *cell_of(BASE, xs, ys))


@gpu
@pytest.mark.parametrize("kw,framed,max3", [(BASE, True, True), (FR1, True, False), (FR0, False, False)])
def test_the_three_cells_and_the_packed_entry(kw, framed, max3):
    rng = np.random.default_rng(kw["match"])
    xs, ys = related_pairs(rng, 9, lambda p: 150, lambda p: 150)
    a, b = tails(rng, 150, 150)
    xs, ys = xs + a, ys + b
    assert cell_of(kw, xs, ys) == (framed, max3)
    out, ops = check(kw, xs, ys, framed, max3)
    for m, n in ((11, 150), (149, 150)):
        a, b = geometry_batch(rng, m, n)
        check(kw, a, b, framed, max3)
    if max3:  # the 2-bit loader on the same reads (packed_equals expects the FR == 2 cell)
        packed_equals(kw, xs, ys, b"ACGT", out, ops)
