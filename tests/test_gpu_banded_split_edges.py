"""The banded aligner's interior runs at strip, column-0 and last-column edges: the hand-made bands of
tests/band_split_cases.py through Aligner.align_bands_arrays (bg_align_banded_bands_batch) against the oracle's
compute_alignment over the same bands — every record field, band_cells and the complete operation list, bit for bit —
under every split-admitting scoring and every variant of the interior kernels.  Each call asserts which fill families it
launched, and with every run flagged for recomputation the count of redone pairs pins split_of (the Python restatement of
band_split the cases are built with) to the device's own evaluation of the rule.

K4 decides by the row number alone which of the two traceback byte layouts it reads (banded_traceback.hip: in_lo, in_hi).
With either border moved by one row there (in_lo = s_a * 32 + 2, or in_hi = s_b * 32 - 1) test_border_moves and
test_run_borders fail: the cases reach both borders."""
import os

import numpy as np
import pytest

import band_split_cases as bc
import oracle_py as orc
from rust_bio_amd import _lib
from rust_bio_amd.banded import Aligner
from test_gpu_banded import MODES, engine_scoring
from test_gpu_score_edges import banded_fills, k3p_admits, with_clips

pytestmark = pytest.mark.gpu
F = _lib.FILL
MID_THRESH = 63000  # (test_gpu_banded.py: some partners of a lane group flagged, others not)
# name -> options on top of band_fill_v1 = -1 (K3v2 and its interior kernels also for a small call)
VARIANTS = {
    "default": {},
    "packed-off": {"band_packed_off": 1},
    "redo-all": {"band_packed_thresh": 65535},
    "redo-some": {"band_packed_thresh": MID_THRESH},
    "interior-off": {"band_interior_off": 1},
    "wide": {"force_wide": 1},
}
OP_CODE = {"M": 0, "S": 1, "D": 2, "I": 3, "X": 4, "Y": 5}
SCORING_IDS = [s[0] for s in bc.SCORINGS]


@pytest.fixture(scope="module")
def fam():
    f = dict(borders=bc.run_borders(), shapes=bc.row_shapes(), moves=bc.border_moves())
    f["mixes"] = bc.wavefront_mixes(f["borders"], f["shapes"], f["moves"])
    return f


_wants = {}


def want_of(c, scoring):
    """the oracle's answer for one case under one scoring, computed once: (record fields, band_cells, op bytes, clip lengths)"""
    name, mode, kw = scoring
    key = (c.name, name)
    if key not in _wants:
        w = orc.banded_align_bands(orc.make_scoring(**kw), mode, c.x, c.y, c.start, c.end)
        ops = np.array([OP_CODE[t[0]] for t in w["ops"]], dtype=np.uint8)
        clips = [int(t[1:]) for t in w["ops"] if t[0] in "XY"]
        rec = tuple(w[f] for f in ("score", "xstart", "xend", "ystart", "yend", "xlen", "ylen", "mode")) + (len(ops),)
        _wants[key] = (rec, w["band_cells"], ops, clips)
    return _wants[key]


def run(cases, scoring, variant):
    """one call of align_bands_arrays; every pair against the oracle; returns the context (for the launch mask / redo count)"""
    _, mode, kw = scoring
    kwc = with_clips(kw)
    al = Aligner.with_scoring(engine_scoring(kwc, True), 0, 0)
    opts = dict(VARIANTS[variant], band_fill_v1=-1)
    x, xo, y, yo, bo, st, en = bc.concat(cases)
    for k_, v_ in opts.items():
        al.ctx.set_option(k_, v_)
    try:
        out, ops = al.align_bands_arrays(MODES[mode], x, xo, y, yo, bo, st, en)
        mask, redo = al.ctx.last_fill_kernels(), al.ctx.band_redo_pairs()
    finally:  # (the default context is shared between Aligners)
        for k_ in opts:
            al.ctx.set_option(k_, 0)
        al.ctx.set_option("band_fill_v1", int(os.environ.get("BG_BAND_FILL_V1", "0")))
    for p, c in enumerate(cases):
        rec, cells, wops, wclips = want_of(c, scoring)
        r = out[p]
        assert int(r["status"]) == 0, (c, variant, r)
        got = tuple(int(r[f]) for f in ("score", "xstart", "xend", "ystart", "yend", "xlen", "ylen", "mode", "n_ops"))
        assert got == rec, (c, scoring[0], variant, p, got, rec)
        assert int(al.last_cells[p]) == cells, (c, variant)
        gops = ops[int(r["ops_off"]):int(r["ops_off"]) + int(r["n_ops"])]
        assert gops.tobytes() == wops.tobytes(), (c, scoring[0], variant, p, bytes(gops), bytes(wops))
        assert int(r["n_clips"]) == len(wclips) and [int(v) for v in r["clip_len"][:len(wclips)]] == wclips, (c, variant, p)
    # the call ran the kernels it names
    if opts.get("band_interior_off"):
        want_mask = F["K3V2_NARROW"]
    else:
        want_mask = banded_fills(kwc, mode, max(c.m for c in cases), max(c.n for c in cases), opts)
    assert mask == want_mask, (scoring[0], variant, hex(mask), hex(want_mask))
    packed = k3p_admits(kw, max(c.n for c in cases))
    runs = sum(bc.split_of(c.start, c.end, c.m)[0] for c in cases)
    if variant == "redo-all" and packed:
        assert redo == runs, (scoring[0], [c.name for c in cases], redo, runs)
    if variant in ("packed-off", "interior-off", "wide") or not packed:
        assert redo == 0, (scoring[0], variant, redo)
    print("band_redo_pairs", scoring[0], variant, "pairs", len(cases), "with a run", runs, "redone", redo)
    assert redo <= runs  # (K3p flags what it computed: pairs with a run)
    return al.ctx


def family_case(fam, name, scoring, variant):
    cases = bc.admitted(fam[name], scoring[2])
    assert len(fam[name]) - len(cases) <= 1
    run(cases, scoring, variant)


def test_scorings_are_what_they_are_for():
    packed = [k3p_admits(kw, 400) for _, _, kw in bc.SCORINGS]
    assert packed == [True, True, True, True, False]  # the last one: K3i alone
    for _, mode, kw in bc.SCORINGS:
        assert banded_fills(with_clips(kw), mode, 320, 400, {"band_fill_v1": -1}) & F["K3I"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("scoring", bc.SCORINGS, ids=SCORING_IDS)
def test_run_borders(fam, scoring, variant):
    """end_0 x start_n x m around the strip borders: runs of 0, 1 and 2 strips, column 0 outside the band, column n empty,
    start_n == 0, row m inside column 0 only, x of one base and of none"""
    family_case(fam, "borders", scoring, variant)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("scoring", bc.SCORINGS, ids=SCORING_IDS)
def test_row_shapes(fam, scoring, variant):
    """rows of 1 .. 33 cells starting 0, 1 and 15 mod 16 on the run's first row; first columns that jump by 17 and 40
    from one row to the next, and one that stays for 20 rows"""
    family_case(fam, "shapes", scoring, variant)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("scoring", bc.SCORINGS, ids=SCORING_IDS)
def test_border_moves(fam, scoring, variant):
    """insertions, deletions and mismatches on the rows either side of in_lo and in_hi"""
    family_case(fam, "moves", scoring, variant)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("scoring", bc.SCORINGS, ids=SCORING_IDS)
def test_wavefront_mixes(fam, scoring, variant):
    """batches of 1, 2, 7, 8, 9 and 17 pairs with different runs (and none) in one wavefront and in one K3p couple; as
    they are, reversed and rotated by one — a pair's result does not depend on its neighbours"""
    for size, batch in fam["mixes"].items():
        for order, cases in bc.orders(batch).items():
            if size == 1 and order != "asis":
                continue
            run(cases, scoring, variant)


@pytest.mark.parametrize("scoring", bc.SCORINGS, ids=SCORING_IDS)
def test_one_row_short_of_a_run_redoes_nothing(fam, scoring):
    """a batch of pairs with s_a == s_b only: every run flagged for recomputation, and nothing is recomputed"""
    short = bc.one_row_short(fam["borders"])
    assert len(short) >= 20 and not any(bc.split_of(c.start, c.end, c.m)[0] for c in short)
    ctx = run(short, scoring, "redo-all")
    assert ctx.band_redo_pairs() == 0
