"""The narrow-score fill kernels at the edges of the ranges they are admitted for, against the oracle (every record and
every operation) and against the same call on a wider kernel.  Each admission rule of sw_api.hip / banded_api.hip is
restated below; the edge scorings are derived from it, and every case asserts which fill families the call launched
(bg_last_fill_kernels), so that a case at a bound really ran the narrow kernel and the case one step past it did not."""
import os

import numpy as np
import pytest

from rust_bio_amd import _lib, synth
from rust_bio_amd.banded import Aligner as BandedAligner
from rust_bio_amd.pairwise import MIN_SCORE, Aligner, Scoring, decode_ops
from test_gpu_banded import differential, oracle_banded
from test_gpu_pk16 import local_vs_oracle
from test_oracle_score_edges import TIE_SCORINGS, families, magnitude_scorings

import oracle_py as orc

pytestmark = pytest.mark.gpu
F = _lib.FILL
NEG = MIN_SCORE
CLIP_NAMES = ("xclip_prefix", "xclip_suffix", "yclip_prefix", "yclip_suffix")


# ---- admission rules --------------------------------------------------------------------------------------------------

def mode_clips(mode, clips):
    """the four clips a mode aligns with (the wrappers overwrite them, mod.rs:934-999)"""
    if mode == "global":
        return (NEG,) * 4
    if mode == "semiglobal":
        return (NEG, NEG, 0, 0)
    if mode == "local":
        return (0,) * 4
    return tuple((clips or {}).get(c, NEG) for c in CLIP_NAMES)


def magnitude(kw, clips4):
    """largest absolute finite number of the scoring (clips at MIN_SCORE are 'minus infinity')"""
    vals = [kw["gap_open"], kw["gap_extend"], kw["match"], kw["mismatch"]] + [c for c in clips4 if c != NEG]
    return max(abs(v) for v in vals)


def k1p_admits(mag, max_x, max_y):  # sw_api.hip: two pairs per lane, int16 keys (x up to 32 lanes x 12 rows)
    return 1 <= max_x <= 384 and mag * (max(max_x, max_y) + 2) <= 2040


def k1_narrow_admits(mag, max_x, max_y):  # sw_api.hip: int32 keys score << 4
    return mag * (max_x + max_y + 8) < 1 << 24


def local_flavour(kw, clips4):  # sw_api.hip: the LF flavours (Aligner::local with costly gaps and mismatches)
    return clips4 == (0,) * 4 and kw["gap_open"] < 0 and kw["mismatch"] < 0 and kw["match"] >= 0


def sw_fill(kw, mode, clips, max_x, max_y, opts=None):
    """the one fill family an Aligner call launches: plan_fill (sw_api.hip) in the same order — K1p if admitted, K1's
    LF flavour if admitted and x fits one strip, else K1 by its keys"""
    opts = opts or {}
    c4 = mode_clips(mode, clips)
    mag = magnitude(kw, c4)
    lf = local_flavour(kw, c4) and not opts.get("no_local_fast")
    if not opts.get("no_pk16") and k1p_admits(mag, max_x, max_y):
        return F["K1P_LF"] if lf else F["K1P"]
    narrow = not opts.get("force_wide") and k1_narrow_admits(mag, max_x, max_y)
    if narrow and lf and max_x <= 512:  # (x of one strip: 64 lanes x 8 rows beyond 384)
        return F["K1_LF"]
    return F["K1_NARROW"] if narrow else F["K1_WIDE"]


NARROW_NEG_CLIP = NEG + (1 << 20)  # banded_kernels.h: kNarrowNegClip


def banded_clip_ok(c):  # banded_api.hip: 'minus infinity' to the narrow kernels, or a small real score
    return c <= NARROW_NEG_CLIP or c >= -(1 << 22)


def k3p_target_minus_thresh(match, mismatch, gap_open):  # banded_api.hip / banded_fill2p.hip
    mk, mis = (match << 4) + 12, (-mismatch << 4) - 10
    target = (0xfff0 - (mk + mis) - (match << 9) - 32) & ~15
    thresh = (match << 9) + 16 + (-gap_open << 4) + 32
    return target - thresh


def k3p_admits(kw, max_y):
    return (0 <= kw["match"] <= 64 and -1024 <= kw["mismatch"] <= -1 and -1024 <= kw["gap_open"] <= -1 and
            -1024 <= kw["gap_extend"] <= 0 and max_y < 65536 and
            k3p_target_minus_thresh(kw["match"], kw["mismatch"], kw["gap_open"]) >= 1 << 14)


def banded_fills(kw, mode, max_x, max_y, opts):
    """the families a banded call launches, for a batch of at most 2048 pairs (one sub-batch)"""
    if opts.get("band_fill_v1", 0) >= 0:
        return F["K3"]  # (small batches: one pair per wavefront)
    c4 = mode_clips(mode, kw)
    mag = max(abs(kw["gap_open"]), abs(kw["gap_extend"]), abs(kw["match"]), abs(kw["mismatch"]), 1)
    narrow = (not opts.get("force_wide") and mag * (max_x + max_y + 8) < 1 << 24 and all(banded_clip_ok(c) for c in c4))
    if not narrow:
        return F["K3V2_WIDE"]
    split = c4[0] <= NARROW_NEG_CLIP and c4[1] <= NARROW_NEG_CLIP and c4[2] > NARROW_NEG_CLIP
    if not split:
        return F["K3V2_NARROW"]
    packed = not opts.get("band_packed_off") and k3p_admits(kw, max_y)
    return F["K3V2_NARROW"] | F["K3I"] | (F["K3P"] if packed else 0)


def test_rules_give_the_documented_edges():
    assert k1p_admits(13, 150, 150) and not k1p_admits(14, 150, 150)
    assert k1p_admits(1, 8, 2038) and not k1p_admits(1, 8, 2039) and not k1p_admits(0, 385, 10)
    assert k1_narrow_admits(8355, 1000, 1000) and not k1_narrow_admits(8356, 1000, 1000)
    assert banded_clip_ok(NEG) and banded_clip_ok(NEG + (1 << 20)) and not banded_clip_ok(int(NEG / 2))
    assert not banded_clip_ok(-(1 << 22) - 1) and banded_clip_ok(-(1 << 22))


# ---- K1p and K1 -------------------------------------------------------------------------------------------------------

def k1p_bound_edges():
    """every (mag, L) with mag * (L + 2) == 2040"""
    return [(mag, 2040 // mag - 2) for mag in range(1, 2041) if 2040 % mag == 0 and 2040 // mag - 2 >= 1]


def edge_batch(rng, L):
    """L on x (x == y, disjoint letters, 1-8 symbol x, related and unrelated: ragged couples) up to 384, else on y with
    a short x"""
    pairs = families(rng, L, L) if L <= 384 else families(rng, 8, L)
    return [p[0] for p in pairs], [p[1] for p in pairs]


def sw_case(kw, mode, clips, xs, ys, opts=None):
    out, ops, ctx = local_vs_oracle(kw, xs, ys, mode, clips, opts)
    mask = ctx.last_fill_kernels()
    want = sw_fill(kw, mode, clips, max(len(x) for x in xs), max(len(y) for y in ys), opts)
    assert mask == want, (kw, mode, clips, opts, hex(mask), hex(want))
    return out, ops


def same_call(a, b):
    (o1, p1), (o2, p2) = a, b
    assert o1.tobytes() == o2.tobytes()
    n = int(o1["n_ops"].sum())
    assert (p1[:n] == p2[:n]).all()


def custom_clips(mag, flip):
    m = -mag
    return (dict(xclip_prefix=m, xclip_suffix=NEG, yclip_prefix=NEG, yclip_suffix=m) if flip else
            dict(xclip_prefix=NEG, xclip_suffix=m, yclip_prefix=m, yclip_suffix=NEG))


@pytest.mark.parametrize("mag,L", k1p_bound_edges(), ids=lambda v: str(v))
def test_k1p_at_its_bound_and_one_step_past(mag, L):
    rng = np.random.default_rng(mag * 1000 + L)
    kws = magnitude_scorings(mag)
    kw = kws[mag % 2]
    for it, (m_, L_) in enumerate(((mag, L), (mag, L + 1), (mag + 1, L))):
        at_bound = it == 0
        kw_ = magnitude_scorings(m_)[mag % 2]
        xs, ys = edge_batch(rng, L_)
        assert k1p_admits(m_, max(len(x) for x in xs), max(len(y) for y in ys)) == at_bound
        for mode, clips in (("global", None), ("semiglobal", None), ("local", None), ("custom", custom_clips(m_, mag % 2))):
            r = sw_case(kw_, mode, clips, xs, ys)
            if at_bound:
                same_call(r, sw_case(kw_, mode, clips, xs, ys, {"no_pk16": 1}))
        if at_bound:  # local on the general K1p (no LF flavour); the mixed scoring too
            same_call(sw_case(kw, "local", None, xs, ys, {"no_local_fast": 1}), sw_case(kw, "local", None, xs, ys))
            sw_case(kws[2], "custom", custom_clips(mag, 1 - mag % 2), xs, ys)


@pytest.mark.parametrize("mode", ["global", "semiglobal", "local", "custom"])
def test_k1p_scorings_where_every_path_ties(mode):
    rng = np.random.default_rng(17)
    for L in (384, 150, 2000):
        xs, ys = edge_batch(rng, L)
        for kw in TIE_SCORINGS:
            clips = dict(xclip_prefix=0, xclip_suffix=NEG, yclip_prefix=NEG, yclip_suffix=0) if mode == "custom" else None
            r = sw_case(kw, mode, clips, xs, ys)
            same_call(r, sw_case(kw, mode, clips, xs, ys, {"no_pk16": 1}))


@pytest.mark.parametrize("m,n", [(1000, 1000), (300, 1700), (8, 2000)])
def test_k1_narrow_at_its_bound_and_one_step_past(m, n):
    rng = np.random.default_rng(m + n)
    pairs = families(rng, m, n)
    xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    mag_max = ((1 << 24) - 1) // (m + n + 8)
    for mag in (mag_max, mag_max + 1):
        assert k1_narrow_admits(mag, m, n) == (mag == mag_max)
        assert abs(MIN_SCORE) + 2 * mag * (m + n + 2) < 1 << 31  # (beyond that the reference's i32 overflows)
        for kw in magnitude_scorings(mag)[::2]:
            for mode, clips in (("global", None), ("custom", custom_clips(mag, 0)), ("custom", custom_clips(mag, 1)),
                                ("local", None)):
                r = sw_case(kw, mode, clips, xs, ys)
                same_call(r, sw_case(kw, mode, clips, xs, ys, {"force_wide": 1}))


# ---- banded: K3v2 narrow, K3i, K3p ------------------------------------------------------------------------------------

def long_reads(seed, n_pairs=20):
    """related 2-4 kb reads with long indels (x inside y, y inside x), unrelated pairs (test_gpu_banded.py's interior runs)"""
    rng = np.random.default_rng(seed)
    xs, ys = [], []
    for p in range(n_pairs):
        n = int(rng.integers(1800, 4200))
        y = synth.random_dna(n, seed * 100 + 7000 + p)
        if p % 7 == 6:
            x = synth.random_dna(int(rng.integers(300, 900)), seed * 100 + 9000 + p)
        else:
            xm, lens = synth.mutate_fixed(y.reshape(1, -1), seed * 100 + 8000 + p, 0.05, 0.03, 0.03)
            x = xm[0][:int(lens[0])]
            if p % 5 == 0:
                c = int(rng.integers(200, len(x) - 400))
                x = np.concatenate([x[:c], x[c + int(rng.integers(20, 90)):]])
                c = int(rng.integers(200, len(x) - 200))
                x = np.concatenate([x[:c], synth.random_dna(int(rng.integers(20, 90)), seed * 100 + 9500 + p), x[c:]])
            if p % 4 == 1:
                x = x[int(rng.integers(1, 300)):len(x) - int(rng.integers(1, 300))]
        xs.append(np.asarray(x, dtype=np.uint8).tobytes())
        ys.append(np.asarray(y, dtype=np.uint8).tobytes())
    return xs, ys


def with_clips(kw):
    """the four clips (MIN_SCORE where kw names none; the modes other than custom overwrite them anyway)"""
    return dict({c: NEG for c in CLIP_NAMES}, **kw)


def banded_oracle(kw, mode, k, w, xs, ys):
    return oracle_banded(with_clips(kw), True, mode, k, w, xs, ys)


def banded_case(kw, mode, k, w, xs, ys, opts, wants):
    kw = with_clips(kw)
    try:
        differential(kw, True, mode, k, w, xs, ys, opts, wants)
    finally:  # (differential leaves its options at 0; the suite's default fill choice is BG_BAND_FILL_V1's)
        differential.last_ctx.set_option("band_fill_v1", int(os.environ.get("BG_BAND_FILL_V1", "0")))
    ctx = differential.last_ctx
    mask = ctx.last_fill_kernels()
    want = banded_fills(kw, mode, max(len(x) for x in xs), max(len(y) for y in ys), opts)
    assert mask == want, (kw, mode, opts, hex(mask), hex(want))
    return ctx


BASE = dict(gap_open=-5, gap_extend=-1, match=1, mismatch=-1)
# interior runs need x clips at 'minus infinity' and a real y-prefix clip
SPLIT = dict(BASE, xclip_prefix=NEG, xclip_suffix=NEG, yclip_prefix=-3, yclip_suffix=-2)
CLIP_EDGES = [-(1 << 22), -(1 << 22) - 1, NEG + (1 << 26) - 1, NEG + (1 << 26), -700_000_000, int(NEG / 2), int(NEG / 2) + 1,
              NEG + (1 << 20) + 1, NEG + (1 << 20), NEG + 1, NEG]
BANDED_RUNS = ({"band_fill_v1": -1}, {"band_fill_v1": 1}, {"band_fill_v1": -1, "force_wide": 1})


@pytest.mark.parametrize("clip", CLIP_NAMES)
def test_banded_clip_edges(clip):
    """each clip position at the ends of the narrow kernels' map (banded_fill2.inc: to_s) and of clip_ok"""
    xs, ys = long_reads(3, 12)
    for v in CLIP_EDGES:
        kw = dict(SPLIT, **{clip: v})
        wants = banded_oracle(kw, "custom", 12, 20, xs, ys)
        for opts in BANDED_RUNS:
            banded_case(kw, "custom", 12, 20, xs, ys, opts, wants)


@pytest.mark.parametrize("kw", [dict(BASE, match=3, mismatch=-2), dict(BASE, gap_extend=0, mismatch=-4)], ids=["a", "b"])
def test_banded_narrow_product_bound(kw):
    """mag * (max_x + max_y + 8) just below 2^24 (narrow) and at it (wide), with the split scoring (K3i)"""
    xs, ys = long_reads(5, 10)
    span = max(len(x) for x in xs) + max(len(y) for y in ys) + 8
    mag_max = ((1 << 24) - 1) // span
    for mag in (mag_max, mag_max + 1):
        for kw_ in (dict(SPLIT, **dict(kw, gap_open=-mag)), dict(SPLIT, **dict(kw, match=mag)), dict(SPLIT, **dict(kw, mismatch=-mag))):
            wants = banded_oracle(kw_, "custom", 12, 20, xs, ys)
            for opts in BANDED_RUNS + ({"band_fill_v1": -1, "band_packed_off": 1},):
                banded_case(kw_, "custom", 12, 20, xs, ys, opts, wants)
        for mode in ("global", "local"):
            kw_ = dict(kw, gap_open=-mag)
            banded_case(kw_, mode, 12, 20, xs, ys, {"band_fill_v1": -1}, banded_oracle(kw_, mode, 12, 20, xs, ys))


def k3p_edge_scorings():
    """scorings on both sides of each of K3p's limits"""
    out = []
    fit = [mt for mt in range(0, 200) if k3p_target_minus_thresh(mt, -1, -1) >= 1 << 14]
    out += [dict(BASE, match=0, gap_open=-1), dict(BASE, match=max(fit), gap_open=-1), dict(BASE, match=max(fit) + 1, gap_open=-1)]
    for f in ("mismatch", "gap_open", "gap_extend"):
        out += [dict(BASE, **{f: v}) for v in (-1, -1024, -1025)]
    # target - thresh within 16 of 2^14 on either side (gap_open moves it by 16 per unit)
    for mt in range(0, 65):
        for go in range(1, 1024):
            if k3p_target_minus_thresh(mt, -3, -go) >= 1 << 14 > k3p_target_minus_thresh(mt, -3, -go - 1):
                d0, d1 = k3p_target_minus_thresh(mt, -3, -go), k3p_target_minus_thresh(mt, -3, -go - 1)
                if d0 - (1 << 14) < 16 and (1 << 14) - d1 <= 16:
                    out += [dict(BASE, match=mt, mismatch=-3, gap_open=-go), dict(BASE, match=mt, mismatch=-3, gap_open=-go - 1)]
        if len(out) > 14:
            break
    out.append(dict(BASE, gap_open=-1024, gap_extend=-1024))
    return out


@pytest.mark.parametrize("kw", k3p_edge_scorings(), ids=lambda kw: "m%d_x%d_o%d_e%d" % (kw["match"], kw["mismatch"], kw["gap_open"], kw["gap_extend"]))
def test_k3p_admission_limits(kw):
    xs, ys = long_reads(7)
    wants = banded_oracle(kw, "semiglobal", 12, 20, xs, ys)
    inside = k3p_admits(kw, max(len(y) for y in ys))
    for opts in ({"band_fill_v1": -1}, {"band_fill_v1": -1, "band_packed_thresh": 65535}, {"band_fill_v1": -1, "band_packed_off": 1}):
        ctx = banded_case(kw, "semiglobal", 12, 20, xs, ys, opts, wants)
        redo = ctx.band_redo_pairs()
        if not inside or opts.get("band_packed_off"):
            assert redo == 0, (opts, redo)
        elif opts.get("band_packed_thresh"):
            assert redo >= 10, (opts, redo)  # every pair with an interior run
        elif kw["gap_open"] == kw["gap_extend"] == -1024:
            assert redo >= 1, redo  # band cells sink below their strip's floor on real data: detect-and-recompute runs


@pytest.mark.parametrize("n", [65535, 65536])
def test_k3p_longest_y(n):
    y = synth.random_dna(n, 4242)
    xm, lens = synth.mutate_fixed(y[30_000:33_000].reshape(1, -1), 4243, 0.04, 0.02, 0.02)
    xs, ys = [np.asarray(xm[0][:int(lens[0])], dtype=np.uint8).tobytes()], [y.tobytes()]
    wants = banded_oracle(BASE, "semiglobal", 12, 20, xs, ys)
    ctx = banded_case(BASE, "semiglobal", 12, 20, xs, ys, {"band_fill_v1": -1}, wants)
    assert ctx.band_redo_pairs() == 0
    ctx = banded_case(BASE, "semiglobal", 12, 20, xs, ys, {"band_fill_v1": -1, "band_packed_thresh": 65535}, wants)
    assert ctx.band_redo_pairs() == (1 if n < 65536 else 0)


# ---- the benchmark's scorings keep their kernels ----------------------------------------------------------------------

def test_headline_scorings_keep_their_kernels():
    x, xo, y, yo = synth.sw_pairs(512, 150, seed=1)
    xs = [x[int(xo[p]):int(xo[p + 1])].tobytes() for p in range(512)]
    ys = [y[int(yo[p]):int(yo[p + 1])].tobytes() for p in range(512)]
    head = dict(gap_open=-5, gap_extend=-1, match=1, mismatch=-1)
    assert local_vs_oracle(head, xs, ys, "local")[2].last_fill_kernels() == F["K1P_LF"]
    assert local_vs_oracle(head, xs, ys, "semiglobal")[2].last_fill_kernels() == F["K1P"]
    wide = dict(gap_open=-500, gap_extend=-100, match=100, mismatch=-100)
    assert local_vs_oracle(wide, xs, ys, "local")[2].last_fill_kernels() == F["K1_LF"]
    assert sw_fill(wide, "local", None, 150, 150) == F["K1_LF"]
    # the banded leg: 10 kb semiglobal pairs, k 16, w 32, more pairs than one small batch, the default fill choice
    P, L = 2100, 10_000
    bx, bo, by, _ = synth.sw_pairs(P, L, seed=4, sub=0.06, ins=0.02, dele=0.02)
    al = BandedAligner.with_scoring(Scoring.from_scores(-5, -1, 1, -1), 16, 32)
    al.ctx.set_option("band_fill_v1", 0)
    try:
        out, ops = al.align_arrays(2, bx, bo, by, bo)
        mask = al.ctx.last_fill_kernels()
    finally:
        al.ctx.set_option("band_fill_v1", int(os.environ.get("BG_BAND_FILL_V1", "0")))
    assert mask == F["K3V2_NARROW"] | F["K3I"] | F["K3P"], hex(mask)
    assert (out["status"] == 0).all()
    osc = orc.make_scoring(-5, -1, 1, -1)
    for p in range(0, P, 300):
        want = orc.banded_align(osc, "semiglobal", 16, 32, bx[int(bo[p]):int(bo[p + 1])], by[int(bo[p]):int(bo[p + 1])])
        assert int(out["score"][p]) == want["score"] and decode_ops(out[p], ops) == want["ops"], p
