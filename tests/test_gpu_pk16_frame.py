"""GPU parity of K1p's framed LF cell (sw_fill_pk16.inc, FR: keys kept as K + B + g (r + s)) against the CPU oracle and
against the general K1p (no_local_fast): the scorings whose frame just fits and just misses 15 bits (pk16_frame_fits,
sw_kernels.h), every rows-per-lane instantiation, all-match and all-mismatch reads, ragged couples."""
import numpy as np
import pytest

from rust_bio_amd import _lib
from test_gpu_pk16 import BASE, local_vs_oracle, related_pairs

pytestmark = pytest.mark.gpu
F = _lib.FILL
ALPHA = np.frombuffer(b"ACGT", dtype=np.uint8)


def frame_fits(kw, max_ylen, r, lp):
    """pk16_frame_fits (sw_kernels.h) restated"""
    g = -16 * kw["gap_extend"]
    mk = kw["mismatch"] * 16 + 10  # (mismatch << 4) | C_SUBST << 1
    b = max(2 * g, -mk, -(kw["gap_open"] * 16 + 6), -(kw["gap_open"] * 16 + 4))
    b = (b + 15) & ~15
    return 16 * kw["match"] * max_ylen + b + g * (r + max_ylen + lp - 1) + 15 < 0x8000


def rows_per_lane(m):
    """the R sw_api.hip picks for reads of up to m symbols (every R of 2..12 at 16 lanes, 7..12 at 32)"""
    lp = 16 if m <= 192 else 32
    lo = max((m + lp - 1) // lp, 2 if lp == 16 else 7)
    return next((r for r in range(lo, 13) if m % r == 0), lo), lp


def check(kw, xs, ys, framed):
    """records and operations against the oracle, with and without the frame, and the cell each call got"""
    out, ops, ctx = local_vs_oracle(kw, xs, ys)
    assert ctx.last_fill_kernels() == F["K1P_LF"]
    assert ctx.last_fill_framed() == framed, (kw, len(xs[0]), max(len(y) for y in ys))
    out2, _, ctx = local_vs_oracle(kw, xs, ys, opts={"no_local_fast": 1})
    assert ctx.last_fill_kernels() == F["K1P"] and not ctx.last_fill_framed()
    assert np.array_equal(out, out2)
    _, _, ctx = local_vs_oracle(kw, xs, ys, opts={"no_pk16_frame": 1})
    assert ctx.last_fill_kernels() == F["K1P_LF"] and not ctx.last_fill_framed()


def reads(rng, n_pairs, m, n):
    """related pairs, plus one all-match and one all-mismatch pair"""
    xs, ys = related_pairs(rng, n_pairs, lambda p: m, lambda p: n)
    y = ALPHA[rng.integers(0, 4, size=n)]
    xs.append(np.resize(y, m).tobytes())
    ys.append(y.tobytes())
    xs.append(b"A" * m)
    ys.append(b"C" * n)
    return xs, ys


# m = 150: 16 lanes per pair, 10 rows per lane.  With match 13 and gap costs -5 / -1 (B = 80, g = 16) the frame takes
# 224 n + 495 < 2^15: n = 144 is the longest y that fits; the 12-bit K1p bound (13 x 152 <= 2040) admits both
@pytest.mark.parametrize("kw,n,framed", [
    (dict(gap_open=-5, gap_extend=-1, match=13, mismatch=-1), 144, True),
    (dict(gap_open=-5, gap_extend=-1, match=13, mismatch=-1), 145, False),
    (dict(gap_open=-5, gap_extend=-1, match=12, mismatch=-13), 150, True),
    (dict(gap_open=-9, gap_extend=-4, match=3, mismatch=-2), 150, True),
    (dict(gap_open=-12, gap_extend=-10, match=3, mismatch=-2), 150, False),
    (dict(gap_open=-13, gap_extend=0, match=13, mismatch=-13), 150, True),
])
def test_frame_edges(kw, n, framed):
    assert rows_per_lane(150) == (10, 16) and frame_fits(kw, n, 10, 16) == framed
    check(kw, *reads(np.random.default_rng(n + kw["match"]), 61, 150, n), framed)


@pytest.mark.parametrize("r", range(2, 13))
def test_every_rows_per_lane_lp16(r):
    rng = np.random.default_rng(r)
    m = 16 * r
    for n in (m, m + 9, 7):
        check(BASE, *reads(rng, 45, m, n), True)


@pytest.mark.parametrize("m", [200, 224, 250, 288, 320, 352, 384])
def test_lp32(m):
    rng = np.random.default_rng(m)
    check(BASE, *reads(rng, 29, m, m - 3), True)
    kw = dict(gap_open=-4, gap_extend=-2, match=5, mismatch=-4)  # 5 x 386 <= 2040
    check(kw, *reads(rng, 29, m, m), frame_fits(kw, m, *rows_per_lane(m)))


def test_all_match_and_all_mismatch():
    rng = np.random.default_rng(5)
    for m, n in ((150, 150), (150, 40), (40, 150), (1, 150), (150, 1)):
        y = ALPHA[rng.integers(0, 4, size=max(m, n))]
        xs = [y[:m].tobytes()] * 9 + [b"A" * m] * 9
        ys = [y[:n].tobytes()] * 9 + [b"T" * n] * 9
        check(BASE, xs, ys, True)


def test_ragged_couples():
    # lengths differ within couples (the second launch) and between wavefronts; some y empty
    rng = np.random.default_rng(11)
    for top in (150, 192, 300):
        xs, ys = related_pairs(rng, 301, lambda p: int(rng.integers(1, top + 1)), lambda p: int(rng.integers(0, top + 20)))
        xs[7], ys[7] = b"A" * top, b"A" * (top + 19)
        check(BASE, xs, ys, True)
