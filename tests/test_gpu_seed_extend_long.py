"""Seed-and-extend on reads of 192 .. 2049 bases (tests/seed_long_cases.py: one class on each side of every switch of
plan_fill, sw_api.hip), through every `bg_seed_extend_*` entry point, against the oracle's composition read by read: every field
of the hit and every operation byte, no tolerances.  tests/test_oracle_seed_extend_long.py holds the cases to the oracle first.

Each call asserts the fill family it launched (bg_last_fill_kernels).  What the mask describes after a seed-and-extend call, from
seed_extend.hip: se_align's bg_align_batch_dev_hint ORs in the family of the candidate alignments (max_read_len x max_read_len +
2 pad), once per pass; the rescue calls' R3 (se_rescue) ORs in the family of the rescue alignments (max_read_len x max_span);
nothing resets the mask between seed-and-extend calls.  So every test opens a context of its own, every call of a test is
expected to add nothing to the class's family, and the rescue calls are expected to add exactly R3's.

A max_read_len below the longest read is refused by the SMEM call alone, which checks the lengths for K7's sake before anything
runs; for the other calls it is the caller's promise (the aligner's geometry is sized by it), so only the SMEM call is tried.

Operation slots have the minimum stride, are filled with a canary and followed by a canary region: nothing outside [ops_off,
ops_off + n_ops) may change."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import multi_oracle as mo
import rescueq_oracle as rq
import seed_long_cases as lc
import smem_seed_oracle as sso
import tiered_seed_oracle as tso
import oracle_py as orc
from rescue_cases import flat_of, oracle_rescue
from rust_bio_amd import _lib
from rust_bio_amd.bwt import Occ
from rust_bio_amd.fmindex import FMIndex
from rust_bio_amd.pairwise import Scoring
from rust_bio_amd.pipeline import (MultiParams, PairQualityParams, SeedParams, SmemSeedParams, TieredSeedParams,
                                   attach_text, seed_extend_arrays, seed_extend_dev, seed_extend_multi_dev, seed_extend_pairs_dev,
                                   seed_extend_pairs_rescue_dev, seed_extend_pairs_rescue_mapq_dev, seed_extend_smem_dev,
                                   seed_extend_strands_dev, seed_extend_tiered_dev)
from rust_bio_amd.suffix_array import RawSuffixArray, SampledSuffixArray
from test_gpu_pipeline import compare
from test_gpu_seed_extend_edges import CANARY, untouched_outside_slots
from test_gpu_seed_extend_multi import check as check_multi
from test_gpu_seed_extend_pairq import check_records
from test_gpu_seed_extend_pairs import check, oracle_pairs
from test_gpu_seed_extend_tiered import tables
from test_oracle_seed_extend_long import PP, rescue_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID_ARG, OPS_CAP = -1, -9
NAMES = list(lc.CLASSES)
F = _lib.FILL
FMD_ALPHA = b"ACGTNacgtn"


@contextlib.contextmanager
def open_index(wide=False, sampled=0, fmd=False):
    """the index in a context of its own (a fresh fill mask): the forward text, or the FMD index over T$R$ of the SMEM calls"""
    ctx = _lib.Context(0)
    if wide:
        ctx.set_option("fm_wide_from", 1)
        ctx.set_option("fm_wide_sb_shift", 2)
    if fmd:
        text, sa, b, ls = tables(lc.genome()[0].tobytes(), FMD_ALPHA)[:4]
        fm = FMIndex(b, ls, Occ(b, 3, FMD_ALPHA), ctx=ctx)
    else:
        text, (sa, b, ls) = lc.genome()[1], lc.index()
        fm = FMIndex(b, ls, Occ(b, 64, lc.ALPHA), ctx=ctx)
    if sampled:
        SampledSuffixArray(sa, text, b, sampled, fmindex=fm)
    else:
        RawSuffixArray(sa, fm)
    attach_text(fm, text)
    try:
        yield fm
    finally:
        fm.close()
        ctx.close()


def fill(fm):
    return fm.ctx.last_fill_kernels()


def dev(kind, fm, cs, max_len=None, K=1, qp=None, smem=None, tiered=None, reads=None, off=None):
    """one device flavour with every output; operation slots of exactly the minimum stride, canary in them and behind them.
    Returns a dict of host arrays (hits, strand, pairs, rescued, multi, tier, ops), the stride, totals and the status."""
    reads = cs.reads if reads is None else reads
    off = cs.off if off is None else off
    R = len(off) - 1
    L = cs.L if max_len is None else max_len
    rescue = kind in ("rescue", "rescue_mapq")
    stride = L + max(L + 2 * cs.pad, lc.MAX_SPAN if rescue else 0) + 4
    d_ops = torch.full((R * K * stride + 4096,), CANARY, dtype=torch.uint8, device=DEV)
    d_reads = torch.from_numpy(np.concatenate([reads, np.zeros(16, np.uint8)])).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.full((R * K * 96,), 0x5A, dtype=torch.uint8, device=DEV)
    d_strand = torch.full((R * K,), 77, dtype=torch.uint8, device=DEV)
    d_pairs = torch.full((max(R // 2, 1) * 16,), 0x55, dtype=torch.uint8, device=DEV)
    d_resc = torch.full((max(R // 2, 1),), 0x55, dtype=torch.uint8, device=DEV)
    d_multi = torch.full((R * 16,), 0x55, dtype=torch.uint8, device=DEV)
    d_tier = torch.full((R,), 77, dtype=torch.uint8, device=DEV)
    sc, st, prm = Scoring.from_scores(*cs.sc), torch.cuda.current_stream().cuda_stream, SeedParams(**cs.seed_kw)
    p = dict(reads=d_reads.data_ptr(), off=d_off.data_ptr(), hits=d_hits.data_ptr(), strand=d_strand.data_ptr(), ops=d_ops.data_ptr(),
             pairs=d_pairs.data_ptr(), resc=d_resc.data_ptr(), multi=d_multi.data_ptr(), tier=d_tier.data_ptr())
    tot = np.full(4, 99, dtype=np.uint64)
    status = 0
    try:
        if kind == "single":
            seed_extend_dev(fm, sc, R, p["reads"], p["off"], L, p["hits"], p["ops"], stride, prm, st, tot)
        elif kind == "strands":
            seed_extend_strands_dev(fm, sc, R, p["reads"], p["off"], L, p["hits"], p["strand"], p["ops"], stride, prm, _lib.STRAND_BOTH, st, tot)
        elif kind == "pairs":
            seed_extend_pairs_dev(fm, sc, R // 2, p["reads"], p["off"], L, p["hits"], p["pairs"], p["strand"], p["ops"], stride, prm, PP, st, tot)
        elif kind == "rescue":
            seed_extend_pairs_rescue_dev(fm, sc, R // 2, p["reads"], p["off"], L, p["hits"], p["pairs"], p["resc"], p["strand"], p["ops"], stride,
                                         prm, PP, rescue_params(cs.L), st, tot)
        elif kind == "rescue_mapq":
            seed_extend_pairs_rescue_mapq_dev(fm, sc, R // 2, p["reads"], p["off"], L, p["hits"], p["pairs"], p["resc"], p["multi"], p["strand"],
                                              p["ops"], stride, prm, PP, rescue_params(cs.L), qp, st, tot)
        elif kind == "multi":
            seed_extend_multi_dev(fm, sc, R, p["reads"], p["off"], L, p["hits"], p["multi"], p["strand"], p["ops"], stride, prm,
                                  MultiParams(K), _lib.STRAND_BOTH, st, tot)
        elif kind == "smem":
            seed_extend_smem_dev(fm, sc, R, p["reads"], p["off"], L, p["hits"], p["strand"], p["ops"], stride, SmemSeedParams(**smem),
                                 _lib.STRAND_BOTH, st, tot)
        else:
            seed_extend_tiered_dev(fm, sc, R, p["reads"], p["off"], L, p["hits"], p["strand"], p["tier"], p["ops"], stride,
                                   TieredSeedParams(prm, SmemSeedParams(**smem), tiered), _lib.STRAND_BOTH, st, tot)
    except _lib.BiogpuError as e:
        status = e.status
    finally:
        torch.cuda.synchronize()
    return dict(hits=d_hits.cpu().numpy().view(_lib.SEED_HIT_DTYPE), strand=d_strand.cpu().numpy(), ops=d_ops.cpu().numpy(),
                pairs=d_pairs.cpu().numpy().view(_lib.PAIR_HIT_DTYPE)[:R // 2], rescued=d_resc.cpu().numpy()[:R // 2],
                multi=d_multi.cpu().numpy().view(_lib.MULTI_HIT_DTYPE)[:R], tier=d_tier.cpu().numpy(), stride=stride, totals=tot, status=status)


def counted(name, kind, n):
    """(shown with -s) the reads a call kind compared for a class: all of them"""
    assert n == len(lc.case(name).items) or kind == "multi" or "pairs" in kind
    print(f"class {name}: {kind}: {n} reads compared, fill family {hex(lc.case(name).fill)}")


def single_and_strands(fm, cs, name, what=""):
    """the forward call and the strands call of a class against the oracle; the fill family after each"""
    oh, oops, ostride = lc.oracle_single(name)
    d = dev("single", fm, cs)
    assert d["status"] == 0 and fill(fm) == cs.fill, (what, hex(fill(fm)))
    compare(d["hits"], d["ops"], oh, oops, ostride)
    untouched_outside_slots(d["hits"], d["ops"], d["stride"])
    assert (int(d["totals"][0]), int(d["totals"][1])) == (int(oh["n_seed_hits"].sum()), int(oh["n_candidates"].sum()))
    counted(name, "single" + what, len(oh))
    bh, bstrand, bops, bstride = lc.oracle_both(name)
    d = dev("strands", fm, cs)
    assert d["status"] == 0 and fill(fm) == cs.fill, (what, hex(fill(fm)))
    compare(d["hits"], d["ops"], bh, bops, bstride)
    assert (d["strand"] == bstrand).all()
    untouched_outside_slots(d["hits"], d["ops"], d["stride"])
    counted(name, "strands" + what, len(bh))
    return d


@pytest.mark.parametrize("name", NAMES)
def test_forward_and_both_strands(name):
    cs = lc.case(name)
    with open_index() as fm:
        d = single_and_strands(fm, cs, name)
        placed = [r for r, it in enumerate(cs.items) if it.s is not None]
        assert (d["hits"]["aln"]["score"][placed] > sso.MIN_SCORE).all()  # every planted read, on either strand
        assert (d["strand"][cs.of_kind("rev")] == _lib.HIT_REVERSE).all()
        if name in ("C", "D", "G", "W"):  # the host flavour: max_read_len is the longest read it finds
            oh, oops, ostride = lc.oracle_single(name)
            hits, ops = seed_extend_arrays(fm, Scoring.from_scores(*cs.sc), cs.reads, cs.off, params=SeedParams(**cs.seed_kw))
            assert fill(fm) == cs.fill, hex(fill(fm))
            compare(hits, ops, oh, oops, ostride)
            assert len(ops) == int(hits["aln"]["n_ops"].sum())
            counted(name, "host", len(oh))


@pytest.mark.parametrize("name", ["D", "G"])
def test_wide_layout_with_a_sampled_suffix_array(name):
    cs = lc.case(name)
    with open_index(wide=True, sampled=8) as fm:
        single_and_strands(fm, cs, name, " (wide layout)")


def same_bytes(a, b):
    for k in ("hits", "strand", "ops"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name", ["G", "D"])
def test_passes_and_aligner_sub_batches_change_nothing(name):
    """at least 3 passes (seed_chunk_reads), and a pass's candidates over several aligner sub-batches of 7 (chunk_pairs): in the
    ragged class a sub-batch mixes lengths from 1 to 1500.  Byte for byte the single-pass run: hits, strands, every slot byte"""
    cs = lc.case(name)
    R = len(cs.off) - 1
    with open_index() as fm:
        ref = {k: dev(k, fm, cs) for k in ("single", "strands")}
        bh, bstrand, bops, bstride = lc.oracle_both(name)
        compare(ref["strands"]["hits"], ref["strands"]["ops"], bh, bops, bstride)
        assert int(bh["n_candidates"].sum()) > 3 * 7  # several sub-batches of 7
        for opts in ({"seed_chunk_reads": R // 4}, {"chunk_pairs": 7}, {"seed_chunk_reads": R // 4, "chunk_pairs": 7}):
            assert "seed_chunk_reads" not in opts or -(-R // opts["seed_chunk_reads"]) >= 3
            for k, v in opts.items():
                fm.ctx.set_option(k, v)
            try:
                for kind in ("single", "strands"):
                    got = dev(kind, fm, cs)
                    assert got["status"] == 0 and fill(fm) == cs.fill, (opts, hex(fill(fm)))
                    same_bytes(got, ref[kind])
                    assert (got["totals"] == ref[kind]["totals"]).all()
            finally:
                for k in opts:
                    fm.ctx.set_option(k, 0)
    counted(name, "passes", R)


# ------------------------------------------------------------------------------------------------------------------ pairs


@functools.lru_cache(maxsize=None)
def pair_expectation(name):
    cs = lc.pair_case(name)
    text, (sa, b, ls) = lc.genome()[1], lc.index()
    er, ep, _ = oracle_pairs(b, ls, sa, text, lc.N_TEXT, cs.reads, cs.off, PP, scores=cs.sc, **cs.seed_kw)
    want = oracle_rescue(b, ls, sa, text, lc.N_TEXT, cs.reads, cs.off, PP, rescue_params(cs.L), scores=cs.sc, **cs.seed_kw)
    return er, ep, want


@pytest.mark.parametrize("name", lc.PAIR_CLASSES)
def test_pairs_rescue_and_rescue_mapq(name):
    cs = lc.pair_case(name)
    er, ep, want = pair_expectation(name)
    R = len(cs.off) - 1
    with open_index() as fm:
        d = dev("pairs", fm, cs)
        assert d["status"] == 0 and fill(fm) == cs.fill, hex(fill(fm))
        check(d["hits"], d["strand"], d["pairs"], d["ops"], er, ep)
        untouched_outside_slots(d["hits"], d["ops"], d["stride"])
    # the rescue calls: the candidates' family and, from R3, that of a mate against a window of max_span
    both = cs.fill | lc.fill_of(cs.sc, cs.L, lc.MAX_SPAN)
    assert both == (F["K1P"] | F["K1_NARROW"] if name == "B" else F["K1_NARROW"])
    rr, rp, rescued, n_al, _, cands, nh = want
    assert (rescued != 0).sum() >= 5
    with open_index() as fm:
        d = dev("rescue", fm, cs)
        assert d["status"] == 0 and fill(fm) == both, hex(fill(fm))
        check(d["hits"], d["strand"], d["pairs"], d["ops"], rr, rp)
        assert (d["rescued"] == rescued).all()
        untouched_outside_slots(d["hits"], d["ops"], d["stride"])
        assert [int(t) for t in d["totals"]] == [int(nh.sum()), sum(len(c) for c in cands), n_al, int((rescued != 0).sum())]
        qp = PairQualityParams()
        q = dev("rescue_mapq", fm, cs, qp=qp)
        assert q["status"] == 0 and fill(fm) == both, hex(fill(fm))
        for k in ("hits", "strand", "pairs", "rescued", "ops"):
            assert q[k].tobytes() == d[k].tobytes(), k
        g, text = lc.genome()
        _, _, vr, voff = lc.candidates(name, paired=True)
        p = rescue_params(cs.L)
        recs, _, resc2, _ = rq.expected(orc, orc.make_scoring(*cs.sc), cands, voff, vr, text, lc.N_TEXT, R // 2, PP.min_span, PP.max_span,
                                        PP.pen_unpaired, p.max_anchors, p.min_score, qp.min_score, qp.mapq_cap)
        assert (resc2 == rescued).all()
        check_records(q["multi"], recs)
    counted(name, "pairs, rescue, rescue_mapq", R)


# --------------------------------------------------------------------------------------------------- SMEM, tiered, multi


def smem_params(cs):
    return dict(min_seed_len=19, max_smems=64, max_occ=16, pad=cs.pad)


@functools.lru_cache(maxsize=None)
def smem_expectation(name):
    cs = lc.case(name)
    fwd = lc.genome()[0].tobytes()
    _, sa, b, ls, occ, ofmd = tables(fwd, FMD_ALPHA)
    sc = orc.make_scoring(*cs.sc)
    res = sso.candidates(orc, ofmd, sa, np.frombuffer(fwd, np.uint8), sc, cs.reads, cs.off, **smem_params(cs))
    tiered = tso.tiered(orc, (b, ls, occ, sa), ofmd, np.frombuffer(fwd, np.uint8), sc, cs.reads, cs.off, window=cs.seed_kw,
                        smem=smem_params(cs), reseed_below=cs.L // 2)
    return res, tiered


@pytest.mark.parametrize("name", ["E", "G"])
def test_smem_and_tiered_seeds(name):
    """K7's scratch follows max_read_len; the candidates go the same road as the fixed seeds'"""
    cs = lc.case(name)
    res, tiered = smem_expectation(name)
    want = sso.expected(res)
    n = len(want)
    with open_index(fmd=True) as fm:
        d = dev("smem", fm, cs, smem=smem_params(cs))
        assert d["status"] == (OPS_CAP if res["truncated"].any() else 0) and fill(fm) == cs.fill, (d["status"], hex(fill(fm)))
        sso.compare(d["hits"], d["strand"], d["ops"], want, name)
        untouched_outside_slots(d["hits"], d["ops"], d["stride"])
        placed = [r for r, it in enumerate(cs.items) if it.s is not None]
        assert (d["hits"]["aln"]["score"][placed] > sso.MIN_SCORE).all()
        t = dev("tiered", fm, cs, smem=smem_params(cs), tiered=cs.L // 2)
        assert t["status"] == tiered["status"] and fill(fm) == cs.fill, (t["status"], hex(fill(fm)))
        sso.compare(t["hits"], t["strand"], t["ops"], tiered["want"], name)
        assert (t["tier"] == tiered["tier"]).all() and tuple(int(v) for v in t["totals"][:3]) == tuple(tiered["totals"])
        assert tiered["totals"][2] >= 3  # reads re-seeded with SMEMs
        untouched_outside_slots(t["hits"], t["ops"], t["stride"])
    counted(name, "smem, tiered", n)


def test_a_read_longer_than_max_read_len_is_refused():
    """max_read_len one below the longest read of the ragged class: the SMEM call, whose K7 sizes its interval lists by it, checks
    the lengths before anything runs and refuses, hits, strands and operation slots untouched"""
    cs = lc.case("G")
    with open_index(fmd=True) as fm:
        d = dev("smem", fm, cs, max_len=cs.L - 1, smem=smem_params(cs))
        assert d["status"] == INVALID_ARG
        assert (d["hits"].view(np.uint8) == 0x5A).all() and (d["strand"] == 77).all() and (d["ops"] == CANARY).all()
        assert fill(fm) == 0  # no alignment was launched


def test_multi_on_the_repeat_reads():
    """class F513's reads inside the repeat (two loci of distinct scores each), with reads of one locus and of none"""
    cs = lc.case("F513")
    pick = cs.of_kind("rep_") + cs.of_kind("exact")[:2] + cs.of_kind("rev")[:2] + cs.of_kind("random")[:1]
    reads, off = flat_of([cs.items[r].x for r in pick])
    cands, nh, _, _ = lc.candidates("F513")
    sub = [cands[2 * r + k] for r in pick for k in (0, 1)]
    sub_nh = np.array([nh[2 * r + k] for r in pick for k in (0, 1)])
    K = 4
    exp = mo.expected(sub, sub_nh, len(pick), 3, K)
    assert sum(e[4] >= 2 for e in exp) >= 4
    with open_index() as fm:
        d = dev("multi", fm, cs, K=K, reads=reads, off=off)
        assert d["status"] == 0 and fill(fm) == cs.fill, hex(fill(fm))
        check_multi(d["hits"], d["strand"], d["multi"], d["ops"], exp, K, d["stride"])
        untouched_outside_slots(d["hits"], d["ops"], d["stride"])
    counted("F513", "multi", len(pick))
