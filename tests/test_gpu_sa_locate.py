"""GPU parity tests of the suffix-array lookups (kernel K6 through the C ABI): `Interval::occ`
over a raw and a sampled suffix array — against the reference's own sampled-SA test
(suffix_array.rs:912-964), the CPU oracle, and the raw SA itself.  K6 is one kernel over both index
layouts (uint32 and uint64 positions): the small texts run on both, the wide one forced by the ctx
option fm_wide_from = 1, with one block per superblock and with four."""
import functools
import json
import os

import numpy as np
import pytest

import oracle_py as orc
from rust_bio_amd import _lib, synth
from rust_bio_amd.bwt import Occ, bwt, less
from rust_bio_amd.fmindex import FMIndex, Interval
from rust_bio_amd.suffix_array import NONE, RawSuffixArray, SampledSuffixArray, suffix_array

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "sampled_sa_kats.json")))
ALPHA = b"ACGTNacgtn$"


# the index layouts K6 serves: (id, fm_wide_sb_shift of a ctx that forces 64-bit positions, or None for the default ctx)
LAYOUTS = [("narrow", None), ("wide_sb0", 0), ("wide_sb2", 2)]


def layout_ctx(sb_shift):
    if sb_shift is None:
        return None
    ctx = _lib.Context(0)
    ctx.set_option("fm_wide_from", 1)
    ctx.set_option("fm_wide_sb_shift", sb_shift)
    return ctx


def build(text, k=3, ctx=None, alphabet=ALPHA):
    sa = suffix_array(text)
    b = bwt(text, sa)
    ls = less(b, alphabet)
    return sa, b, ls, FMIndex(b, ls, Occ(b, k, alphabet), ctx=ctx)


# (the narrow cases keep the ids they had before the layout became a parameter)
@pytest.mark.parametrize("case,sb_shift", [(c, sb) for c in GOLD["texts"] for _, sb in LAYOUTS],
                         ids=[c["name"] if sb is None else c["name"] + "-" + name for c in GOLD["texts"] for name, sb in LAYOUTS])
def test_reference_sampled_matches(case, sb_shift):
    text = case["text"].encode()
    sa, b, ls, fm = build(text, GOLD["occ_k"], ctx=layout_ctx(sb_shift))
    rows = np.arange(len(sa) + 2, dtype=np.uint64)  # two rows past the end -> None
    for rate in GOLD["rates"]:
        ssa = SampledSuffixArray(sa, text, b, rate, fmindex=fm)
        got = ssa.get_batch(rows)
        assert (got[:len(sa)] == sa).all(), (case["name"], rate)
        assert (got[len(sa):] == NONE).all()
        assert ssa.get(len(sa)) is None and ssa.get(0) == int(sa[0])
    raw = RawSuffixArray(sa, fm)
    got = raw.get_batch(rows)
    assert (got[:len(sa)] == sa).all() and (got[len(sa):] == NONE).all()


def test_sample_layout_matches_oracle():
    text = GOLD["texts"][-1]["text"].encode()
    sa, b, ls, fm = build(text)
    occ = orc.Occ(b, 3, ALPHA)
    for rate in (2, 5, 16):
        ours = SampledSuffixArray(sa, text, b, rate)
        sample, erow, epos = orc.SampledSuffixArray(sa, text, b, ls, occ, rate).arrays()
        assert (ours.sample == sample).all() and (ours.extra_rows == erow).all() and (ours.extra_pos == epos).all()


def test_interval_occ_kat():
    # fmindex.rs:125-142: TTA in GCCTTAACATTATTACGCCTA$ -> positions [3, 12, 9] (any order in the doc; SA order here)
    text = b"GCCTTAACATTATTACGCCTA$"
    sa, b, ls, fm = build(text)
    res = fm.backward_search(b"TTA")
    host = res.interval.occ(sa)
    assert sorted(host) == [3, 9, 12]
    assert res.interval.occ(RawSuffixArray(sa, fm)) == host
    assert res.interval.occ(SampledSuffixArray(sa, text, b, 4, fmindex=fm)) == host
    with pytest.raises(Exception):  # "Interval out of range of suffix array"
        Interval(0, len(sa) + 1).occ(RawSuffixArray(sa, fm))
    assert Interval(5, 5).occ(RawSuffixArray(sa, fm)) == []


@pytest.mark.parametrize("rate", [1, 7, 32, 64])
def test_genome_locate_vs_oracle(rate):
    # 300 kbp genome with stray N's (exceptions in the 2-bit stream) and three sentinels
    g = synth.random_dna(300_000, seed=21).copy()
    rng = np.random.default_rng(5)
    g[rng.integers(0, len(g), size=40)] = ord("N")
    g[100_000] = g[200_000] = ord("$")
    text = g.tobytes() + b"$"
    sa, b, ls, fm = build(text, k=32)
    ssa = SampledSuffixArray(sa, text, b, rate, fmindex=fm)
    rows = rng.integers(0, len(sa), size=50_000).astype(np.uint64)
    got = ssa.get_batch(rows)
    assert (got == sa[rows.astype(np.intp)]).all()
    # a sample of the same rows through the oracle's restatement of SampledSuffixArray::get
    occ = orc.Occ(b, 32, ALPHA)
    ossa = orc.SampledSuffixArray(sa, text, b, ls, occ, rate)
    for r in rows[:300]:
        assert ossa.get(int(r)) == int(sa[int(r)])
    # intervals of real patterns: occ over sampled == raw
    pats = [text[p:p + 12] for p in rng.integers(0, len(text) - 13, size=2000)]
    res = fm.backward_search_batch([p for p in pats if b"$" not in p])
    lo = [r.interval.lower for r in res if r.kind == "Complete"]
    hi = [r.interval.upper for r in res if r.kind == "Complete"]
    off, pos = fm.interval_occ_arrays(lo, hi)
    want = np.concatenate([sa[a:b_] for a, b_ in zip(lo, hi)])
    assert (pos == want).all() and int(off[-1]) == len(want)


@functools.lru_cache(maxsize=None)
def boundary_text():
    """1 200 symbols of DNA, 12 of them N (sparse exceptions), two inner '$' + the final one (three sentinel rows on the
    side): 7 rank blocks — rows on both sides of pos % 192 == 0 — in 2 superblocks of four blocks, or 7 of one"""
    g = synth.random_dna(1200, seed=12).copy()
    inner = [400, 800]
    rng = np.random.default_rng(1200)
    g[rng.choice(np.setdiff1d(np.arange(1200), inner), size=12, replace=False)] = ord("N")
    g[inner] = ord("$")
    text = g.tobytes() + b"$"
    sa = suffix_array(text)
    b = bwt(text, sa)
    return text, sa, b, less(b, ALPHA)


@pytest.mark.parametrize("sb_shift", [sb for _, sb in LAYOUTS], ids=[name for name, _ in LAYOUTS])
def test_every_row_of_a_text_that_crosses_every_boundary(sb_shift):
    text, sa, b, ls = boundary_text()
    n = len(sa)
    assert n == 1201 and (np.frombuffer(b, dtype=np.uint8) == ord("$")).sum() == 3
    fm = FMIndex(b, ls, Occ(b, 3, ALPHA), ctx=layout_ctx(sb_shift))
    rows = np.arange(n + 2, dtype=np.uint64)  # every row, and two past the end -> None
    some = np.random.default_rng(50).choice(n, size=50, replace=False)
    occ = orc.Occ(b, 3, ALPHA)
    for rate in (1, 2, 5, 32, 1201):  # 1201: a single sample — every walk ends at row 0 or at a sentinel row
        ssa = SampledSuffixArray(sa, text, b, rate, fmindex=fm)
        assert len(ssa.sample) == (n + rate - 1) // rate
        got = ssa.get_batch(rows)
        assert (got[:n] == sa).all(), rate
        assert (got[n:] == NONE).all(), rate
        off, pos = fm.interval_occ_arrays([0], [n])
        assert (pos == sa).all() and int(off[-1]) == n, rate
        # the oracle's restatement of SampledSuffixArray::get on the same rows
        ossa = orc.SampledSuffixArray(sa, text, b, ls, occ, rate)
        for r in some:
            assert ossa.get(int(r)) == int(sa[int(r)]) == int(got[int(r)]), (rate, r)
    fm.close()


def test_dense_symbols_are_located_through_their_bit_vectors():
    """Narrow layout only (a 64-bit index refuses such a text: test_gpu_fm_wide.py): 20 letters — more than 1 024
    positions outside the four most frequent bytes, so the others are ranked in bit vectors (1 501 bits: four 480-bit
    blocks each) and K6 reads bwt[pos] from the raw BWT"""
    alpha = b"ARNDCQEGHILKMFPSTWYV$"
    rng = np.random.default_rng(20)
    text = np.frombuffer(alpha[:20], dtype=np.uint8)[rng.integers(0, 20, size=1500)].tobytes() + b"$"
    sa, b, ls, fm = build(text, alphabet=alpha)
    assert np.sort(np.bincount(np.frombuffer(b, dtype=np.uint8)))[:-4].sum() > 1024
    rows = np.arange(len(sa), dtype=np.uint64)
    for rate in (1, 7, 64):
        ssa = SampledSuffixArray(sa, text, b, rate, fmindex=fm)
        assert (ssa.get_batch(rows) == sa).all(), rate
