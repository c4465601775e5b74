"""Seed-and-extend at the edges of its proposal and seed limits: reads whose seed hit counts are set by construction
(tests/seed_edges.py: 0 .. 1024 hits per read, S = 64 x max_occ 16 and S = 32 x max_occ 32; proposals exactly pad / 2 and
pad / 2 + 1 apart; starts below 0 and windows clipped at both ends of the text; reads shorter than a seed) through
`bg_seed_extend_batch[_dev]`, `_strands_` and `_pairs_`, on the 32-bit and the 64-bit index layout with raw and sampled suffix
arrays.  Hit and candidate counts against the header's rule restated on exact occurrence counts, everything else against the
oracle's composition (oracle/pipeline.cpp, tests/pair_oracle.py), read by read; then every limit the host checks, one value on
each side, through all six entry points."""
import numpy as np
import pytest
import torch

import oracle_py as orc
import seed_edges as se
from rust_bio_amd import _lib
from rust_bio_amd.bwt import Occ, bwt, less
from rust_bio_amd.fmindex import FMIndex
from rust_bio_amd.pairwise import MIN_SCORE, Scoring
from rust_bio_amd.pipeline import (PairParams, SeedParams, attach_text, seed_extend_arrays, seed_extend_dev, seed_extend_pairs_arrays,
                                   seed_extend_pairs_dev, seed_extend_strands_arrays, seed_extend_strands_dev)
from rust_bio_amd.suffix_array import RawSuffixArray, SampledSuffixArray, suffix_array
from test_gpu_pipeline import ALPHA, compare
from test_gpu_seed_extend_pairs import check, oracle_pairs
from test_gpu_seed_extend_strands import oracle_strands

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SC = (-5, -1, 1, -1)
TOO_LARGE, OPS_CAP, UNSUPPORTED = -8, -9, -11
CANARY = 0xA5  # no operation kind has this value
LAYOUTS = [("narrow", 0), ("narrow", 8), ("wide", 0), ("wide", 8)]
_oracle = {}


@pytest.fixture(scope="module")
def case():
    c = se.Case()
    sa = suffix_array(c.text)
    b = bwt(c.text, sa)
    return c, sa, b, less(b, ALPHA)


@pytest.fixture(scope="module", params=LAYOUTS, ids=[f"{w}-sa{s}" for w, s in LAYOUTS])
def fm(request, case):
    """the index in one layout: 64-bit (fm_wide_from = 1, proposals sorted as uint64) or 32-bit; raw or sampled suffix array"""
    c, sa, b, ls = case
    wide, sampled = request.param
    ctx = _lib.Context(0)
    if wide == "wide":
        ctx.set_option("fm_wide_from", 1)
        ctx.set_option("fm_wide_sb_shift", 2)
    f = FMIndex(b, ls, Occ(b, 64, ALPHA), ctx=ctx)
    if sampled:
        SampledSuffixArray(sa, c.text, b, sampled, fmindex=f)
    else:
        RawSuffixArray(sa, f)
    attach_text(f, c.text)
    yield f
    f.close()
    ctx.close()


def oracle(case, batch, stride, max_occ, pad):
    """the oracle's composition on a batch (computed once per parameter set)"""
    key = (batch, stride, max_occ, pad)
    if key not in _oracle:
        c, sa, b, ls = case
        _oracle[key] = orc.seed_extend_batch(b, ls, orc.Occ(b, 64, ALPHA), sa, c.text, c.n_text, orc.make_scoring(*SC),
                                             *getattr(c, batch), seed_len=20, stride=stride, max_occ=max_occ, pad=pad, threads=8)
    return _oracle[key]


def dev_buffers(R, max_len, pad, extra=0):
    """operation slots of exactly the minimum stride, a canary region behind the last one; every byte set to CANARY"""
    stride = 2 * max_len + 2 * pad + 4 + extra
    d_ops = torch.full((R * stride + 4096,), CANARY, dtype=torch.uint8, device=DEV)
    return stride, d_ops


def untouched_outside_slots(hits, ops, stride):
    """the call wrote operations only at [ops_off, ops_off + n_ops) of each read, ending exactly at (r + 1) * stride"""
    R = len(hits)
    n_ops = hits["aln"]["n_ops"].astype(np.int64)
    assert (hits["aln"]["ops_off"].astype(np.int64) == (np.arange(R) + 1) * stride - n_ops).all()
    mask = np.ones(len(ops), bool)
    for r in range(R):
        mask[(r + 1) * stride - n_ops[r]:(r + 1) * stride] = False
    assert (ops[mask] == CANARY).all()
    assert (ops[R * stride:] == CANARY).all()


def run_dev(kind, fm, reads, off, max_len, prm, ops_extra=0, pp=None):
    """one of the three device flavours with every output, operation slots at the minimum stride (+ ops_extra) and a
    canary behind them: (hits, strand, pairs, ops, stride)"""
    R = len(off) - 1
    stride, d_ops = dev_buffers(R, max_len, prm.pad, ops_extra)
    d_reads = torch.from_numpy(reads).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.zeros(R * 96, dtype=torch.uint8, device=DEV)
    d_strand = torch.full((R,), 77, dtype=torch.uint8, device=DEV)
    d_pairs = torch.zeros((max(R // 2, 1) * 16,), dtype=torch.uint8, device=DEV)
    sc, st = Scoring.from_scores(*SC), torch.cuda.current_stream().cuda_stream
    if kind == "single":
        seed_extend_dev(fm, sc, R, d_reads.data_ptr(), d_off.data_ptr(), max_len, d_hits.data_ptr(), d_ops.data_ptr(), stride, prm, st)
    elif kind == "strands":
        seed_extend_strands_dev(fm, sc, R, d_reads.data_ptr(), d_off.data_ptr(), max_len, d_hits.data_ptr(), d_strand.data_ptr(),
                                d_ops.data_ptr(), stride, prm, _lib.STRAND_BOTH, st)
    else:
        seed_extend_pairs_dev(fm, sc, R // 2, d_reads.data_ptr(), d_off.data_ptr(), max_len, d_hits.data_ptr(), d_pairs.data_ptr(),
                              d_strand.data_ptr(), d_ops.data_ptr(), stride, prm, pp or PairParams(), st)
    torch.cuda.synchronize()
    return (d_hits.cpu().numpy().view(_lib.SEED_HIT_DTYPE), d_strand.cpu().numpy(), d_pairs.cpu().numpy().view(_lib.PAIR_HIT_DTYPE)[:R // 2],
            d_ops.cpu().numpy(), stride)


def run_host(kind, fm, reads, off, prm, pp=None):
    sc = Scoring.from_scores(*SC)
    if kind == "single":
        return seed_extend_arrays(fm, sc, reads, off, params=prm)
    if kind == "strands":
        return seed_extend_strands_arrays(fm, sc, reads, off, params=prm)
    return seed_extend_pairs_arrays(fm, sc, reads, off, params=prm, pair_params=pp or PairParams())


# ------------------------------------------------------------------------------------------------- 1, 2: hit counts, layouts


@pytest.mark.parametrize("pad,max_occ", [(25, 16), (1, 16), (25, 1)])
def test_main_batch_at_every_hit_count(fm, case, pad, max_occ):
    """S = 64 seeds (L = 83, stride 1): 0 .. 1024 hits per read, register-rank and LDS sorts, merges at pad / 2 and pad / 2 + 1,
    starts below 0, clipped windows, short reads; both flavours (the device one at the minimum ops_stride, canary behind)"""
    c = case[0]
    reads, off = c.main
    prm = SeedParams(20, 1, max_occ, pad)
    rs = se.restate(c.table, c.n_text, reads, off, 1, max_occ, pad)
    ohits, oops, ostride = oracle(case, "main", 1, max_occ, pad)
    hits, ops = run_host("single", fm, reads, off, prm)
    assert (hits["n_seed_hits"] == [d["nh"] for d in rs]).all()
    assert (hits["n_candidates"] == [len(d["kept"]) for d in rs]).all()
    compare(hits, ops, ohits, oops, ostride)
    dh, _, _, dops, stride = run_dev("single", fm, reads, off, 83, prm)
    compare(dh, dops, ohits, oops, ostride)
    untouched_outside_slots(dh, dops, stride)
    # what the batch reached, from the assertions above
    nh = hits["n_seed_hits"]
    if max_occ == 16:
        assert set(se.NH_VALUES) <= set(nh.tolist())
        assert hits["n_candidates"].max() == 1024 and ((nh > 64) & (hits["n_candidates"] > 64)).sum() >= 20
        assert se.merges_at(rs, pad // 2)
        assert any(d["dropped"] and d["nh"] > 64 for d in rs)
        occ_reads = [r for r, k in enumerate(c.main_labels) if k == "max_occ"]
        assert nh[occ_reads].tolist() == [16, 3]  # seed copies 16 + 17: only the 16 vote; 1 + 2: both
    else:
        occ_reads = [r for r, k in enumerate(c.main_labels) if k == "max_occ"]
        assert nh[occ_reads].tolist() == [0, 1]   # at max_occ 1: the single copy votes, two copies do not
    short = [r for r, k in enumerate(c.main_labels) if k == "short"]
    assert np.diff(off)[short].tolist() == [19, 20, 21, 25, 82] and (hits["n_seed_hits"][short][0] == 0)


@pytest.mark.parametrize("pad", [25, 0])
def test_wide_occ_batch_at_every_hit_count(fm, case, pad):
    """S = 32 seeds (L = 82, stride 2), max_occ 32: S x max_occ = 1024 again, each seed with up to 32 copies"""
    c = case[0]
    reads, off = c.wide
    prm = SeedParams(20, 2, 32, pad)
    rs = se.restate(c.table, c.n_text, reads, off, 2, 32, pad)
    ohits, oops, ostride = oracle(case, "wide", 2, 32, pad)
    hits, ops = run_host("single", fm, reads, off, prm)
    assert (hits["n_seed_hits"] == [d["nh"] for d in rs]).all()
    assert (hits["n_candidates"] == [len(d["kept"]) for d in rs]).all()
    compare(hits, ops, ohits, oops, ostride)
    dh, _, _, dops, stride = run_dev("single", fm, reads, off, 82, prm)
    compare(dh, dops, ohits, oops, ostride)
    untouched_outside_slots(dh, dops, stride)
    assert {0, 1, 64, 65, 512, 513, 1023, 1024} <= set(hits["n_seed_hits"].tolist())
    assert hits["n_candidates"].max() == 1024


# ----------------------------------------------------------------------------------------------------- 3: strands and pairs


def test_both_strands_at_hundreds_of_hits(fm, case):
    """revcomp seeds planted as well: both strands of a read with hundreds of hits each; the joined oracle"""
    c, sa, b, ls = case
    reads, off = c.main
    prm = SeedParams(20, 1, 16, 25)
    ohits, ostrand, oops, ostride = oracle_strands(b, ls, sa, c.text, c.n_text, reads, off, seed_len=20, stride=1, max_occ=16, pad=25)
    hits, strand, ops = run_host("strands", fm, reads, off, prm)
    compare(hits, ops, ohits, oops, ostride)
    assert (strand == ostrand).all()
    dh, ds, _, dops, stride = run_dev("strands", fm, reads, off, 83, prm)
    compare(dh, dops, ohits, oops, ostride)
    assert (ds == ostrand).all()
    untouched_outside_slots(dh, dops, stride)
    fwd = se.restate(c.table, c.n_text, reads, off, 1, 16, 25)
    for r, rc in c.main_rev.items():
        assert hits["n_seed_hits"][r] == fwd[r]["nh"] + rc.planned(16) and rc.planned(16) >= 200, r
    both = [r for r, rc in c.main_rev.items() if fwd[r]["nh"] >= 300 and rc.planned(16) >= 300]
    assert len(both) >= 2 and (strand[list(c.main_rev)] == _lib.HIT_REVERSE).any()


def test_pairs_at_the_top_and_bottom_of_the_candidate_lists(fm, case):
    """the winning combination at candidate 1023 of a 1024-candidate list (orientation A and B), at candidate 0 of both
    lists, and a pair whose partner decides between two equal placements; the pair oracle, host and device flavours"""
    c, sa, b, ls = case
    reads, off = c.pairs
    prm = SeedParams(20, 1, 16, 25)
    pp = PairParams(0, 1000, 17)
    er, ep, cands = oracle_pairs(b, ls, sa, c.text, c.n_text, reads, off, pp, seed_len=20, stride=1, max_occ=16, pad=25)
    hits, strand, pairs, ops = run_host("pairs", fm, reads, off, prm, pp)
    check(hits, strand, pairs, ops, er, ep)
    dh, ds, dp, dops, stride = run_dev("pairs", fm, reads, off, 83, prm, pp=pp)
    check(dh, ds, dp, dops, er, ep)
    untouched_outside_slots(dh, dops, stride)
    assert pairs["proper"].all()
    for p, (kind, F, R) in enumerate(c.pair_info):
        fm_ = 1 if kind == "top_b" else 0  # the mate reported on the forward strand
        lf = cands[4 * p + 2 * fm_]
        i = [x["start"] for x in lf].index(F)
        assert strand[2 * p + fm_] == _lib.HIT_FORWARD and hits["ref_start"][2 * p + fm_] == F
        assert hits["ref_start"][2 * p + 1 - fm_] == R and strand[2 * p + 1 - fm_] == _lib.HIT_REVERSE
        if kind in ("top", "top_b"):
            assert (i, len(lf)) == (1023, 1024)
        elif kind == "bottom":
            assert i == 0 and [x["start"] for x in cands[4 * p + 3]].index(R) == 0
    # the partner's pair moves mate 1 off the copy the strands call picks
    p = [k for k, *_ in c.pair_info].index("partner")
    sh, _, _ = seed_extend_strands_arrays(fm, Scoring.from_scores(*SC), reads, off, params=prm)
    assert sh["ref_start"][2 * p] < hits["ref_start"][2 * p] and sh["aln"]["score"][2 * p] == hits["aln"]["score"][2 * p]


# --------------------------------------------------------------------------------------------------------- 4: limits of the call


KINDS = ("single", "strands", "pairs")


def expect(status, fn, *a, **kw):
    if status == 0:
        return fn(*a, **kw)
    with pytest.raises(_lib.BiogpuError) as e:
        fn(*a, **kw)
    assert e.value.status == status, (fn.__name__, a[0])


@pytest.fixture(scope="module")
def fm_narrow(case):
    c, sa, b, ls = case
    ctx = _lib.Context(0)
    f = FMIndex(b, ls, Occ(b, 64, ALPHA), ctx=ctx)
    RawSuffixArray(sa, f)
    attach_text(f, c.text)
    yield f
    f.close()
    ctx.close()


def two_reads(case, L):
    """an edge read with hits (the main batch's anchored 1024) cut to L, and a random read of length L"""
    c = case[0]
    x = [rd.x for rd, k in zip(c.main_reads, c.main_labels) if k == "anchored"][-1]
    y = se.Genome(1000, seed=7).new_read(L, 1).x
    return se.flat([np.resize(x, L) if L > len(x) else x[:L], y])


@pytest.mark.parametrize("kind", KINDS)
def test_seed_slots_and_proposals_per_read(fm_narrow, case, kind):
    """S = 64 accepted, 65 refused; S x max_occ = 1024 accepted, 1025 refused — host and device flavours"""
    for L, stride, max_occ, status in ((83, 1, 1, 0), (84, 1, 1, UNSUPPORTED), (51, 1, 32, 0), (60, 1, 25, UNSUPPORTED),
                                       (60, 1, 24, 0), (51, 1, 33, UNSUPPORTED)):
        reads, off = two_reads(case, L)
        prm = SeedParams(20, stride, max_occ, 25)
        expect(status, run_host, kind, fm_narrow, reads, off, prm)
        expect(status, run_dev, kind, fm_narrow, reads, off, L, prm)
        if status == 0:
            ohits, oops, ostride = orc.seed_extend_batch(case[2], case[3], orc.Occ(case[2], 64, ALPHA), case[1], case[0].text,
                                                         case[0].n_text, orc.make_scoring(*SC), reads, off, seed_len=20, stride=stride,
                                                         max_occ=max_occ, pad=25, threads=8)
            if kind == "single":
                hits, ops = run_host(kind, fm_narrow, reads, off, prm)
                compare(hits, ops, ohits, oops, ostride)
                assert hits["n_seed_hits"][0] == (16 * (L - 19) if max_occ >= 16 else 0)  # 16 copies of every seed


@pytest.mark.parametrize("kind", KINDS)
def test_read_length_and_pad(fm_narrow, case, kind):
    """max_read_len and pad 65535 accepted (a read whose seeds find nothing), 65536 refused — host and device flavours"""
    y = se.Genome(70_000, seed=9).new_read(65_536, 1).x
    for L, pad, status in ((65_535, 25, 0), (65_536, 25, TOO_LARGE), (83, 65_535, 0), (83, 65_536, TOO_LARGE)):
        reads, off = se.flat([y[:L], y[:40]])
        prm = SeedParams(20, 1100 if L > 83 else 1, 16, pad)
        got = expect(status, run_host, kind, fm_narrow, reads, off, prm)
        dev = expect(status, run_dev, kind, fm_narrow, reads, off, L, prm)
        if status == 0:
            for h in (got[0], dev[0]):
                assert (h["n_seed_hits"] == 0).all() and (h["n_candidates"] == 0).all() and (h["aln"]["score"] == MIN_SCORE).all()
            untouched_outside_slots(dev[0], dev[3], dev[4])


@pytest.mark.parametrize("kind", KINDS)
def test_ops_stride_at_its_minimum(fm_narrow, case, kind):
    """ops_stride = 2 max_read_len + 2 pad + 4 accepted (operations end at (r + 1) ops_stride, nothing written behind the last
    slot), one byte less refused with BG_ERR_OPS_CAP"""
    c = case[0]
    reads, off = c.main if kind != "pairs" else c.pairs
    prm = SeedParams(20, 1, 16, 25)
    hits, _, _, ops, stride = run_dev(kind, fm_narrow, reads, off, 83, prm)
    assert stride == 2 * 83 + 2 * 25 + 4
    untouched_outside_slots(hits, ops, stride)
    assert (hits["aln"]["n_ops"] > 0).sum() >= 8
    expect(OPS_CAP, run_dev, kind, fm_narrow, reads, off, 83, prm, ops_extra=-1)
