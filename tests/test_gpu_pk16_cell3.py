"""GPU parity of the three savings of the framed LF cell of v_pk_maximum3_f16 (sw_fill_pk16.inc, FR == 2) against the CPU
oracle, against the cell of v_pk_max_i16 (no_pk16_max3) and against the general K1p (no_local_fast), records and every
operation, and which cell ran:
  - the local floor enters through D (D' = max(D, F)): gaps whose D meets the floor exactly, D below the floor for whole fills;
  - symbols in the high byte of a half, the match term by one saturating subtract: bytes that differ in one bit, 0x00 / 0x80,
    0xff, N against N, the 2-bit flavour on the same reads, and the admission bound 16 (match - mismatch) + 2 <= 256;
  - row maxima of a two-step trip by one maximum of three: zero, one and several trips, odd and even ends, a merge between
    trips, ties of a row's maximum in adjacent columns inside a trip, across trips and across a 16-step block, key 0 only."""
import numpy as np
import pytest

import oracle_py as orc
from rust_bio_amd import _lib
from rust_bio_amd.pairwise import Aligner, Scoring, decode_ops
from test_gpu_pk16 import BASE, local_vs_oracle, related_pairs
from test_gpu_pk16_frame import reads, rows_per_lane
from test_gpu_pk16_max3 import EDGES, check, max3_fits

gpu = pytest.mark.gpu
ALPHA = np.frombuffer(b"ACGT", dtype=np.uint8)


def delta(kw):
    """pk16_delta (sw_kernels.h) restated: match key - mismatch key, (match << 4 | C_MATCH << 1) - (mismatch << 4 | C_SUBST << 1)"""
    return 16 * (kw["match"] - kw["mismatch"]) + 2


def cell3_fits(kw, max_ylen, r, lp):
    """pk16_max3_fits (sw_kernels.h) restated, the symbol compare's bound included"""
    return max3_fits(kw, max_ylen, r, lp) and 0 <= delta(kw) <= 256


def test_every_scoring_of_the_max3_tests_is_admitted():
    # no GPU: tests/test_gpu_pk16_max3.py expects the FR == 2 cell for these, at the lengths it states
    for kw, n_top in EDGES:
        assert delta(kw) <= 256 and cell3_fits(kw, n_top, 10, 16) and not cell3_fits(kw, n_top + 1, 10, 16)
    assert delta(BASE) == 34 and cell3_fits(BASE, 169, 10, 16) and cell3_fits(BASE, 319, 10, 32)
    assert delta(dict(match=8, mismatch=-7)) == 242 and delta(dict(match=8, mismatch=-8)) == 258


# ---------------------------------------------------------------- the floor through D

def gap_pairs(rng, m, n):
    """k matches (S = k), then g symbols of y the read does not have: D = k + go + ge g right of them — with -5 / -1 and k = 6,
    g = 1 exactly the floor 0, one less or more around it; after o unrelated symbols, so that rows and steps vary"""
    xs, ys = [], []
    for k in (5, 6, 7, 8):
        for g in (1, 2, 3):
            for o in (0, 3, 9):
                core = ALPHA[rng.integers(0, 4, size=m)]
                x = np.concatenate([np.full(o, ord("N"), np.uint8), core])[:m]
                y = np.concatenate([np.full(o, ord("n"), np.uint8), core[:k], np.full(g, ord("X"), np.uint8), core[k:]])[:n]
                xs.append(x.tobytes())
                ys.append(y.tobytes())
    return xs, ys


@gpu
@pytest.mark.parametrize("m", [16, 150])
def test_gap_whose_d_meets_the_floor(m):
    assert rows_per_lane(m) == ((2, 16) if m == 16 else (10, 16))
    assert BASE["gap_open"] + BASE["gap_extend"] == -6  # D right of six matches is 0
    check(BASE, *gap_pairs(np.random.default_rng(m), m, m), max3=True)


@gpu
@pytest.mark.parametrize("m", [16, 150])
def test_d_below_the_floor_all_along(m):
    # all-mismatch pairs: every D, I and diagonal stays below F(r, s), every best key is the floor's, every row maximum key 0
    xs = [b"A" * m] * 5 + [b"G" * m] * 4 + [b"AC" * (m // 2)] * 4
    ys = [b"C" * m] * 5 + [b"T" * (m + 3)] * 4 + [b"GT" * (m // 2)] * 4
    check(BASE, xs, ys, max3=True)


# ---------------------------------------------------------------- the symbol compare

SYMBOLS = {"one_bit": b"AaCc", "top_bit": b"\x00\x80\x01\x81", "ff": b"\xff\x7f\xfe\xef", "with_n": b"ACGN"}


def packed_equals(kw, xs, ys, codes, out, ops):
    """the 2-bit flavour on the same reads (codes: their four symbols): the byte flavour's records and operations, FR == 2"""
    import torch
    from rust_bio_amd import pack2
    x, xo = _lib.concat(xs)
    y, yo = _lib.concat(ys)
    al = Aligner.with_scoring(Scoring.from_scores(kw["gap_open"], kw["gap_extend"], kw["match"], kw["mismatch"]))
    dxo, dyo = torch.from_numpy(xo.astype(np.int64)).to("cuda:0"), torch.from_numpy(yo.astype(np.int64)).to("cuda:0")
    xpk, bx = pack2.pack_dev(torch.from_numpy(x.copy()).to("cuda:0"), codes=codes)
    ypk, by = pack2.pack_dev(torch.from_numpy(y.copy()).to("cuda:0"), codes=codes)
    assert bx == 0 and by == 0
    n, mx, my = len(xs), max(len(s) for s in xs), max(len(s) for s in ys)
    stride = mx + my + 4
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device="cuda:0")
    d_ops = torch.zeros(n * stride, dtype=torch.uint8, device="cuda:0")
    al.align_packed_dev(3, n, xpk.data_ptr(), dxo.data_ptr(), ypk.data_ptr(), dyo.data_ptr(), mx, my, d_out.data_ptr(), d_ops.data_ptr(),
                        stride, codes=codes)
    torch.cuda.synchronize()
    assert al.ctx.last_fill_kernels() == _lib.FILL["K1P_LF"] and al.ctx.last_fill_framed() and al.ctx.last_fill_max3()
    out2, ops2 = d_out.cpu().numpy().view(_lib.ALN_DTYPE), d_ops.cpu().numpy()
    for f in ("score", "xstart", "xend", "ystart", "yend", "xlen", "ylen", "n_ops", "status"):
        assert np.array_equal(out[f], out2[f]), f
    for p in range(n):
        assert decode_ops(out2[p], ops2) == decode_ops(out[p], ops), p


@gpu
@pytest.mark.parametrize("name", sorted(SYMBOLS))
@pytest.mark.parametrize("m", [16, 150])
def test_symbols_that_differ_in_one_bit_or_fill_the_byte(name, m):
    alpha = np.frombuffer(SYMBOLS[name], dtype=np.uint8)
    rng = np.random.default_rng(m + len(name))
    xs, ys = related_pairs(rng, 21, lambda p: m, lambda p: m + p % 3, alpha=alpha)
    # every symbol against itself and against each of the others, all along
    for a in range(4):
        for b in range(4):
            xs.append(bytes([alpha[a]]) * m)
            ys.append(bytes([alpha[b]]) * m)
    out, ops, _ = local_vs_oracle(BASE, xs, ys)
    for a in range(4):
        for b in range(4):
            assert out["score"][21 + 4 * a + b] == (m if a == b else 0)
    check(BASE, xs, ys, max3=True)
    packed_equals(BASE, xs, ys, SYMBOLS[name], out, ops)


# ---------------------------------------------------------------- the admission bound of the symbol compare

@gpu
@pytest.mark.parametrize("mismatch,admitted", [(-7, True), (-8, False)])
def test_delta_gate(mismatch, admitted):
    # match 8: 16 (8 + 7) + 2 = 242 <= 256 runs the cell, 16 (8 + 8) + 2 = 258 the one of v_pk_max_i16; both framed
    # (B = 112 / 128, g = 16: the top key 144 n + 527 / 543 stays below 0x7c00 up to n = 216), both inside K1p's 12 bits
    kw = dict(gap_open=-5, gap_extend=-1, match=8, mismatch=mismatch)
    assert (delta(kw) <= 256) == admitted and max3_fits(kw, 150, 10, 16) and cell3_fits(kw, 150, 10, 16) == admitted
    rng = np.random.default_rng(-mismatch)
    xs, ys = reads(rng, 35, 150, 150)
    check(kw, xs, ys, max3=admitted, framed=True)
    assert rows_per_lane(16) == (2, 16) and cell3_fits(kw, 16, 2, 16) == admitted
    check(kw, *reads(rng, 35, 16, 16), max3=admitted, framed=True)


# ---------------------------------------------------------------- row maxima of a two-step trip

@gpu
@pytest.mark.parametrize("n", [15, 16, 17, 18, 19, 31, 32, 33, 34])
def test_trips_none_one_several_odd_and_even_ends(n):
    # 16 lanes: unpredicated steps 15 .. n - 1, one on its own at 15, trips from 16; merge_rows after steps 15 and 31
    check(BASE, *reads(np.random.default_rng(n), 35, 150, n), max3=True)


@gpu
@pytest.mark.parametrize("n", [33, 250])
def test_trips_lp32(n):
    assert rows_per_lane(250) == (10, 32)
    check(BASE, *reads(np.random.default_rng(n), 29, 250, n), max3=True)


M_TIE, N_TIE = 150, 190


def tie_pairs():
    """x = A^k G^(m - k), y = C^o A^(k + 1) C^(n - o - k - 1): row k has its maximum k in the two columns o + k and o + k + 1 (a
    tie that reaches column n goes to column n: mod.rs:706-714 wants strictly more for the clip), the first at step
    s = o + k - 1 + (k - 1) // 10 of lane (k - 1) // 10.  Returns the pairs and, for each, (k, o, s)."""
    xs, ys, where = [], [], []
    for k in (20, 41, 77, 100, 133, 150):
        for o in range(0, 19):
            xs.append(b"A" * k + b"G" * (M_TIE - k))
            ys.append(b"C" * o + b"A" * (k + 1) + b"C" * (N_TIE - o - k - 1))
            where.append((k, o, o + k - 1 + (k - 1) // 10))
    return xs, ys, where


def tie_class(s):
    """where the first two columns of the tie fall: 'a' both steps of one trip (trips start on even steps), 'c' either side
    of a 16-step block boundary, 'b' different trips of one block"""
    return "a" if s % 2 == 0 else "c" if s % 16 == 15 else "b"


def test_tie_pairs_tie_in_the_oracle():
    # no GPU: S(k, o + k) == S(k, o + k + 1) == k in the oracle's local matrix (an alignment that has to end in that cell: no
    # suffix clips, free prefixes), k is the score of the pair, and the oracle ends it in the earlier column
    xs, ys, where = tie_pairs()
    assert {tie_class(s) for _, _, s in where} == {"a", "b", "c"}
    assert all(15 <= s and s + 1 < N_TIE for _, _, s in where)  # unpredicated steps both
    ends_here = orc.make_scoring(**BASE, xclip_prefix=0, yclip_prefix=0)
    local = orc.make_scoring(**BASE)
    for (k, o, s), x, y in list(zip(where, xs, ys))[::7]:
        for j in (o + k, o + k + 1):
            assert orc.align(ends_here, "custom", x[:k], y[:j])["score"] == k, (k, o, j)
        a = orc.align(local, "local", x, y)
        assert (a["score"], a["xend"], a["yend"]) == (k, k, o + k), (k, o)


@gpu
def test_row_maximum_ties_keep_the_earlier_column():
    xs, ys, where = tie_pairs()
    out, _, _ = local_vs_oracle(BASE, xs, ys)
    for p, (k, o, s) in enumerate(where):
        assert (out["score"][p], out["xend"][p], out["yend"][p]) == (k, k, o + k), (k, o, tie_class(s))
    check(BASE, xs, ys, max3=True)


@gpu
def test_ragged_couples_and_empty_y():
    rng = np.random.default_rng(17)
    for top in (150, 300):
        xs, ys = related_pairs(rng, 151, lambda p: int(rng.integers(1, top + 1)), lambda p: int(rng.integers(0, top + 20)))
        xs[7], ys[7] = b"A" * top, b"A" * (top + 19)
        xs[8], ys[8] = b"A" * top, b""
        check(BASE, xs, ys, max3=True)
