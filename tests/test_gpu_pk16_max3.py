"""GPU parity of the framed LF cell's three-input maximum (sw_fill_pk16.inc, FR == 2: the best key taken with two
v_pk_maximum3_f16 on keys that are non-negative finite half-precision bit patterns) against the same call with the cell of
v_pk_max_i16 (no_pk16_max3), against the general K1p (no_local_fast) and against the CPU oracle: the lengths at which every
key just stays below 0x7c00 (pk16_max3_fits, sw_kernels.h) and just does not, keys at the top of that range and in the
denormal range, every rows-per-lane instantiation, ramp-only fills, ragged couples."""
import numpy as np
import pytest

from rust_bio_amd import _lib
from rust_bio_amd.pairwise import decode_ops
from test_gpu_pk16 import BASE, local_vs_oracle, related_pairs
from test_gpu_pk16_frame import reads, rows_per_lane

pytestmark = pytest.mark.gpu
F = _lib.FILL
ALPHA = np.frombuffer(b"ACGT", dtype=np.uint8)


def frame_top(kw, max_ylen, r, lp):
    """the largest key of the frame, the left side of pk16_frame_fits / pk16_max3_fits (sw_kernels.h) restated"""
    g = -16 * kw["gap_extend"]
    mk = kw["mismatch"] * 16 + 10  # (mismatch << 4) | C_SUBST << 1
    b = max(2 * g, -mk, -(kw["gap_open"] * 16 + 6), -(kw["gap_open"] * 16 + 4))
    b = (b + 15) & ~15
    return 16 * kw["match"] * max_ylen + b + g * (r + max_ylen + lp - 1) + 15


def max3_fits(kw, max_ylen, r, lp):
    return frame_top(kw, max_ylen, r, lp) < 0x7c00  # +inf in half precision


def frame_fits(kw, max_ylen, r, lp):
    return frame_top(kw, max_ylen, r, lp) < 0x8000


def all_ops(out, ops):
    return [decode_ops(out[p], ops) for p in range(len(out))]


def check(kw, xs, ys, max3, framed=True):
    """records and operations against the oracle (local_vs_oracle), against the v_pk_max_i16 cell and against the general
    K1p, and the cell each call got"""
    out, ops, ctx = local_vs_oracle(kw, xs, ys)
    where = (kw, len(xs[0]), max(len(y) for y in ys))
    assert ctx.last_fill_kernels() == F["K1P_LF"], where
    assert ctx.last_fill_framed() == framed and ctx.last_fill_max3() == max3, where
    want = all_ops(out, ops)
    out1, ops1, ctx = local_vs_oracle(kw, xs, ys, opts={"no_pk16_max3": 1})
    assert ctx.last_fill_kernels() == F["K1P_LF"] and ctx.last_fill_framed() == framed and not ctx.last_fill_max3(), where
    assert np.array_equal(out, out1) and all_ops(out1, ops1) == want, where
    out2, ops2, ctx = local_vs_oracle(kw, xs, ys, opts={"no_local_fast": 1})
    assert ctx.last_fill_kernels() == F["K1P"] and not ctx.last_fill_framed() and not ctx.last_fill_max3(), where
    assert np.array_equal(out, out2) and all_ops(out2, ops2) == want, where


# m = 150: 16 lanes per pair, 10 rows per lane; the 12-bit K1p bound (13 x 152, 12 x 152 <= 2040) admits every case.
# match 13, gaps -5 / -1 (B = 80, g = 16): the top key is 224 n + 495, below 0x7c00 up to n = 139 (and below 0x8000 up
# to 144); match 3, gaps -12 / -10 (B = 320, g = 160): 208 n + 4335, up to n = 131 (0x8000: 136)
EDGES = [(dict(gap_open=-5, gap_extend=-1, match=13, mismatch=-1), 139),
         (dict(gap_open=-12, gap_extend=-10, match=3, mismatch=-2), 131)]


@pytest.mark.parametrize("kw,n_top", EDGES)
@pytest.mark.parametrize("over", [0, 1])
def test_admission_edges(kw, n_top, over):
    assert rows_per_lane(150) == (10, 16)
    longest = max(n for n in range(1, 400) if max3_fits(kw, n, 10, 16))
    assert longest == n_top and max3_fits(kw, n_top, 10, 16) and not max3_fits(kw, n_top + 1, 10, 16)
    assert frame_top(kw, n_top, 10, 16) < 0x7c00 <= frame_top(kw, n_top + 1, 10, 16)
    assert frame_fits(kw, n_top + 1, 10, 16)  # one column more still runs framed, through the v_pk_max_i16 cell
    n = n_top + over
    check(kw, *reads(np.random.default_rng(n + kw["match"]), 45, 150, n), max3=not over, framed=True)


@pytest.mark.parametrize("kw,n_top", EDGES)
def test_key_extremes(kw, n_top):
    # all-match pairs at the admitted maximum: the last cells' keys reach the top of the frame, just below 0x7c00;
    # all-mismatch pairs: every key stays at the floor F(r, s) = B + g (r + s), which starts below 0x0400 — denormal
    # half-precision bit patterns, which a flushing maximum would turn into 0
    assert frame_top(kw, 0, 0, 1) - 15 < 0x0400
    rng = np.random.default_rng(n_top)
    y = ALPHA[rng.integers(0, 4, size=max(150, n_top))]
    xs = [y[:150].tobytes()] * 9 + [np.resize(y[:n_top], 150).tobytes()] * 9 + [b"A" * 150] * 9 + [b"G" * 150] * 9
    ys = [y[:n_top].tobytes()] * 18 + [b"T" * n_top] * 9 + [b"C" * n_top] * 9
    check(kw, xs, ys, max3=True)


def test_denormal_keys_short_reads():
    # 16 x 16 under the usual scoring (B = 80, g = 16, two rows per lane): every key of the whole fill, the all-match
    # pairs' included, stays below 0x0400
    assert rows_per_lane(16) == (2, 16) and frame_top(BASE, 16, 2, 16) < 0x0400
    rng = np.random.default_rng(3)
    y = ALPHA[rng.integers(0, 4, size=16)]
    rx, ry = related_pairs(rng, 19, lambda p: 16, lambda p: 16)
    check(BASE, [y.tobytes()] * 9 + [b"A" * 16] * 9 + rx, [y.tobytes()] * 9 + [b"C" * 16] * 9 + ry, max3=True)


@pytest.mark.parametrize("r", range(2, 13))
def test_every_rows_per_lane_lp16(r):
    rng = np.random.default_rng(r)
    for m in (16 * r, 16 * r - 1):
        check(BASE, *reads(rng, 35, m, m), max3=True)


def test_lp32():
    rng = np.random.default_rng(32)
    assert rows_per_lane(250) == (10, 32)
    check(BASE, *reads(rng, 29, 250, 247), max3=True)


@pytest.mark.parametrize("m,n", [(150, 1), (150, 7), (150, 15), (250, 20)])
def test_short_y_ramp_steps_only(m, n):
    # n < lanes per pair: no step has every lane inside its matrix, the fill is ramp steps alone
    assert n < rows_per_lane(m)[1]
    check(BASE, *reads(np.random.default_rng(m + n), 35, m, n), max3=True)


def test_ragged_couples():
    # lengths differ within couples (the second launch) and between wavefronts; some y empty
    rng = np.random.default_rng(13)
    for top in (150, 300):
        xs, ys = related_pairs(rng, 151, lambda p: int(rng.integers(1, top + 1)), lambda p: int(rng.integers(0, top + 20)))
        xs[7], ys[7] = b"A" * top, b"A" * (top + 19)
        check(BASE, xs, ys, max3=True)
