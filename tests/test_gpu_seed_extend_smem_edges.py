"""SMEM-seeded seed-and-extend (`bg_seed_extend_smem_batch[_dev]`, csrc/seed_smem.hip) at the edges of its proposal stage: reads
whose suffix-array rows are set by construction (tests/smem_edges.py: 0 .. 1024 rows per read at max_smems x max_occ = 64 x 16
and 32 x 32, every row a start of its own or 16 .. 32 starts of 32 .. 64 equal keys, the rows split between the halves of T$R$,
a read cut at max_smems; reads at the first and last bases of T and hanging over them; proposals pad / 2 and pad / 2 + 1 apart,
chains of them, equal and near starts across the strands), heavy reads between ordinary ones and next to the pass boundaries of
the device flavour.  Every hit field, the strand, both counts and the winner's operations against the CPU statement
(tests/smem_seed_oracle.py), the counts against the restatement of tests/smem_edges.py as well; on the 32-bit and the 64-bit
index layout, with a raw and a sampled suffix array, forward, reverse and both strands, host and device flavours."""
import functools

import numpy as np
import pytest
import torch

import fmd_cases as fc
import oracle_py as orc
import smem_edges as se
import smem_seed_oracle as sso
from rust_bio_amd import _lib
from rust_bio_amd.bwt import Occ
from rust_bio_amd.fmindex import FMIndex
from rust_bio_amd.pairwise import Scoring
from rust_bio_amd.pipeline import SmemSeedParams, attach_text, seed_extend_smem_arrays, seed_extend_smem_dev
from rust_bio_amd.suffix_array import RawSuffixArray, SampledSuffixArray

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPS_CAP = -9
CANARY = 0xA5  # no operation kind has this value
SCORES = (-5, -1, 1, -1)
SC = Scoring.from_scores(*SCORES)
F, R, BOTH = sso.STRAND_FORWARD, sso.STRAND_REVERSE, sso.STRAND_BOTH
LAYOUTS = [("narrow", 0), ("narrow", 8), ("wide", 0), ("wide", 8)]


@pytest.fixture(scope="module", params=LAYOUTS, ids=[f"{w}-sa{s}" for w, s in LAYOUTS])
def fm(request):
    """the FMD index over T$R$ in one layout: 64-bit (fm_wide_from = 1, proposals sorted as uint64 keys) or 32-bit; raw or
    sampled suffix array"""
    c = se.corpus()
    wide, sampled = request.param
    ctx = _lib.Context(0)
    if wide == "wide":
        ctx.set_option("fm_wide_from", 1)
        ctx.set_option("fm_wide_sb_shift", 2)
    f = FMIndex(c.bwt, c.less, Occ(c.bwt, 3, fc.ALPHA), ctx=ctx)
    if sampled:
        SampledSuffixArray(c.sa, c.text, c.bwt, sampled, fmindex=f)
    else:
        RawSuffixArray(c.sa, f)
    attach_text(f, c.text)
    yield f
    f.close()
    ctx.close()


@functools.lru_cache(maxsize=None)
def oracle(name, strands=BOTH, pad=25):
    """(the statement's result, `expected` of it, the restatement) of a batch, once per parameter set"""
    c = se.corpus()
    res = sso.candidates(orc, c.ofmd, c.sa, c.fwd, orc.make_scoring(*SCORES), *c.reads[name], strands=strands, **c.params(name, pad))
    return res, sso.expected(res), c.restate(name, pad, strands)


def check(name, strands, pad, hits, strand, ops, what):
    res, want, rs = oracle(name, strands, pad)
    assert (hits["n_seed_hits"] == [d["n_seed_hits"] for d in rs]).all(), what
    assert (hits["n_candidates"] == [d["n_candidates"] for d in rs]).all(), what
    sso.compare(hits, strand, ops, want, what)
    return res, want


def host_call(fm, name, strands=BOTH, pad=25, allow_truncated=True):
    c = se.corpus()
    return seed_extend_smem_arrays(fm, SC, *c.reads[name], SmemSeedParams(**c.params(name, pad)), strands=strands,
                                   allow_truncated=allow_truncated)


def dev_call(fm, name, strands=BOTH, pad=25, chunk=0):
    """the device flavour with every output, operation slots at the minimum stride and a canary behind them, in passes of `chunk`
    reads (0: one pass): (hits, strand, ops, totals).  A batch with a read cut at max_smems answers every read and says so."""
    c = se.corpus()
    buf, off = c.reads[name]
    n, max_len = len(off) - 1, int(np.diff(off).max())
    stride = 2 * max_len + 2 * pad + 4
    d_reads = torch.from_numpy(buf.copy()).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.full((n * 96,), 0x5A, dtype=torch.uint8, device=DEV)
    d_strand = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
    d_ops = torch.full((n * stride + 4096,), CANARY, dtype=torch.uint8, device=DEV)
    tot = np.zeros(2, dtype=np.uint64)
    status = 0
    fm.ctx.set_option("seed_chunk_reads", chunk)
    try:
        seed_extend_smem_dev(fm, SC, n, d_reads.data_ptr(), d_off.data_ptr(), max_len, d_hits.data_ptr(), d_strand.data_ptr(),
                             d_ops.data_ptr(), stride, SmemSeedParams(**c.params(name, pad)), strands, torch.cuda.current_stream().cuda_stream,
                             tot)
    except _lib.BiogpuError as e:
        status = e.status
    finally:
        torch.cuda.synchronize()
        fm.ctx.set_option("seed_chunk_reads", 0)
    assert status == (OPS_CAP if any(x.get("truncated") for x in c.cases[name]) else 0)
    hits, ops = d_hits.cpu().numpy().view(_lib.SEED_HIT_DTYPE), d_ops.cpu().numpy()
    # operations only at [ops_off, ops_off + n_ops) of each read, ending exactly at (r + 1) * stride
    n_ops = hits["aln"]["n_ops"].astype(np.int64)
    assert (hits["aln"]["ops_off"].astype(np.int64) == (np.arange(n) + 1) * stride - n_ops).all()
    mask = np.ones(len(ops), bool)
    for r in range(n):
        mask[(r + 1) * stride - n_ops[r]:(r + 1) * stride] = False
    assert (ops[mask] == CANARY).all()
    return hits, d_strand.cpu().numpy(), ops, tot


@pytest.mark.parametrize("strands", [F, R, BOTH], ids=["forward", "reverse", "both"])
@pytest.mark.parametrize("name", list(se.SHAPES))
def test_count_cases_host_flavour(fm, name, strands):
    """0 .. 1024 rows per read: the rank-by-broadcast path up to 64, the LDS sort of 128 .. 1024 keys, the compaction of equal
    keys across its blocks of 64, the strand bit's boundary anywhere in the sorted list, reads at the ends of T"""
    hits, strand, ops = host_call(fm, name, strands)
    res, want = check(name, strands, 25, hits, strand, ops, (name, strands))
    c = se.corpus()
    nh = np.array([d["nh"] for d in c.restate(name)])
    assert set(se.NH_VALUES) <= set(nh.tolist()) and (nh == 1024).sum() >= 6
    if strands == BOTH:
        assert hits["n_candidates"].max() == 1024 and ((hits["n_seed_hits"] > hits["n_candidates"]) & (hits["n_candidates"] == 0)).sum() >= 4
    # a read with more than max_smems records: the call says so unless told that this is expected
    if strands == BOTH:
        with pytest.raises(_lib.BiogpuError) as e:
            host_call(fm, name, strands, allow_truncated=False)
        assert e.value.status == OPS_CAP


@pytest.mark.parametrize("strands,chunk", [(F, 0), (R, 0), (BOTH, 0), (BOTH, se.CHUNK), (R, se.CHUNK), (BOTH, 1)],
                         ids=["forward", "reverse", "both", "both-passes", "reverse-passes", "both-single-read-passes"])
@pytest.mark.parametrize("name", list(se.SHAPES))
def test_count_cases_device_flavour(fm, name, strands, chunk):
    """the same in one pass, in passes of CHUNK reads (a pass boundary directly before one 1024-row read and directly after
    another, a third at the end of a short last pass) and with every read a pass of its own; the totals over the passes"""
    hits, strand, ops, tot = dev_call(fm, name, strands, chunk=chunk)
    res, want = check(name, strands, 25, hits, strand, ops, (name, strands, chunk))
    assert int(tot[0]) == res["rows"] and int(tot[1]) == sum(w[2] for w in want)


@pytest.mark.parametrize("pad", se.PADS)
def test_merge_cases(fm, pad):
    """proposals pad / 2 and pad / 2 + 1 apart, chains (a start is compared with the last one kept), equal and near starts
    across the strands (never merged), a read that is its own reverse complement; pad 25, 24, 1 and 0"""
    for strands in (BOTH, F, R):
        hits, strand, ops = host_call(fm, "merge", strands, pad, allow_truncated=False)
        check("merge", strands, pad, hits, strand, ops, (pad, strands))
    for chunk in (0, 1):
        hits, strand, ops, tot = dev_call(fm, "merge", BOTH, pad, chunk)
        res, want = check("merge", BOTH, pad, hits, strand, ops, (pad, chunk))
        assert int(tot[0]) == res["rows"] and int(tot[1]) == sum(w[2] for w in want)
    kinds = [x["kind"] for x in se.corpus().cases["merge"]]
    for r, k in enumerate(kinds):
        if k in ("palindrome", "strands_equal", "strands_5_apart"):
            assert hits["n_candidates"][r] == 2, (pad, r, k)
        if k == "palindrome":
            assert strand[r] == sso.HIT_FORWARD and hits["aln"]["score"][r] == 60
