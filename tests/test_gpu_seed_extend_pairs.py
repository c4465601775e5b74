"""Read pairs in seed-and-extend (`bg_seed_extend_pairs_batch[_dev]`) against a CPU statement of the rule (tests/pair_oracle.py):
every candidate of every (mate, strand) restated on the oracle's own calls (backward_search_batch, the suffix array,
align_batch semiglobal), pinned to the oracle's composition, then the pair rule of include/biogpu.h.  Every hit field, the
reported hits' complete operations, strand, span, n_proper and proper, read by read and pair by pair."""
import numpy as np
import pytest
import torch

import oracle_py as orc
import pair_oracle as po
from rust_bio_amd import _lib, synth
from rust_bio_amd.alphabets import dna
from rust_bio_amd.bwt import Occ, bwt, less
from rust_bio_amd.fmindex import FMIndex
from rust_bio_amd.pairwise import MIN_SCORE, Scoring
from rust_bio_amd.pipeline import (PairParams, SeedParams, attach_text, seed_extend_pairs_arrays, seed_extend_pairs_dev,
                                   seed_extend_strands_arrays, seed_extend_strands_dev)
from rust_bio_amd.suffix_array import RawSuffixArray, SampledSuffixArray, suffix_array
from test_gpu_pipeline import ALPHA, build
from test_gpu_seed_extend_strands import oracle_strands

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID_ARG, OUT_OF_ALPHABET = -1, -7
HIT_FORWARD, HIT_REVERSE, HIT_NONE = _lib.HIT_FORWARD, _lib.HIT_REVERSE, _lib.HIT_NONE
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
SC = (-5, -1, 1, -1)


def flat_of(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.ascontiguousarray(np.concatenate(seqs)), off


def mates_at(g, s, frag, L, seed, swap, sub=0.04):
    """pairs from fragments text[s .. s + frag): mate 1 its first L bases, mate 2 the revcomp of its last L, swapped where
    `swap`; mutated like the bench reads.  Returns (reads uint8[2n, L], origin[2n], rev[2n])."""
    org = np.stack([s, s + frag - L], axis=1)
    rev = np.zeros_like(org, dtype=bool)
    rev[:, 1] = True
    org[swap], rev[swap] = org[swap][:, ::-1], rev[swap][:, ::-1]
    org, rev = org.reshape(-1), rev.reshape(-1)
    refs = np.stack([g[o:o + L] for o in org])
    for k in np.nonzero(rev)[0]:
        refs[k] = np.frombuffer(dna.revcomp(refs[k].tobytes()), np.uint8)
    reads, _ = synth.mutate_fixed(refs, seed, sub, 0.005, 0.005)
    return reads, org, rev


def make_case(n_text=200_000, n_pairs=500, L=150, ragged=False):
    """synth.read_pairs on a genome with a repeat, then: 10 pairs with an unmappable mate 2, 10 chimeric pairs"""
    g = synth.random_dna(n_text, seed=31).copy()
    g[50_000:50_400] = g[10_000:10_400]
    text = np.append(g, np.uint8(ord("$")))
    reads, org, rev = synth.read_pairs(text, n_pairs, L, seed=12, sub=0.04, ins=0.005, dele=0.005)
    R = reads.reshape(-1, L).copy()
    R[2 * np.arange(n_pairs - 10, n_pairs) + 1] = synth.random_dna(10 * L, seed=5).reshape(10, L)
    R[2 * np.arange(n_pairs - 20, n_pairs - 10) + 1] = R[2 * np.arange(0, 10) + 1]  # mate 2 of another pair
    seqs = list(R)
    if ragged:
        lens = np.random.default_rng(3).integers(15, L + 1, size=2 * n_pairs)
        lens[:200] = L
        seqs = [R[r, :lens[r]] for r in range(2 * n_pairs)]
    flat, off = flat_of(seqs)
    return g, text, flat, off, org, rev


def oracle_pairs(b, ls, sa, text, n_text, reads, off, pp, scores=SC, **kw):
    """(expected reads, expected pairs, the candidates of the virtual reads)"""
    occ = orc.Occ(b, 64, ALPHA)
    vr, voff = po.virtual_reads(reads, off)
    cands, nh = po.candidates(orc, b, ls, occ, sa, text, n_text, orc.make_scoring(*scores), vr, voff, **kw)
    er, ep = po.expected(cands, nh, (len(off) - 1) // 2, pp.min_span, pp.max_span, pp.pen_unpaired)
    return er, ep, cands


def check(hits, strand, pairs, ops, er, ep):
    """the call's outputs against the expectation: every field, the reported hits' complete operations"""
    for r, (st, c, nc, nsh) in enumerate(er):
        h = hits[r]
        assert strand[r] == st, r
        assert h["n_candidates"] == nc and h["n_seed_hits"] == nsh, r
        if c is None:
            assert h["aln"]["score"] == MIN_SCORE and h["ref_start"] == NONE and h["window_start"] == NONE, r
            continue
        for f in ("score", "xstart", "xend", "ystart", "yend", "xlen", "ylen", "n_ops"):
            assert int(h["aln"][f]) == int(c["rec"][f]), (r, f)
        assert h["aln"]["mode"] == 2
        assert (int(h["window_start"]), int(h["ref_start"]), int(h["ref_end"])) == (c["wlo"], c["ref_start"], c["ref_end"]), r
        k, o = int(h["aln"]["n_ops"]), int(h["aln"]["ops_off"])
        assert (ops[o:o + k] == c["ops"]).all(), r
    for p, (proper, span, n_proper) in enumerate(ep):
        assert (int(pairs["proper"][p]), int(pairs["span"][p]), int(pairs["n_proper"][p])) == (int(proper), span, n_proper), p
    assert (pairs["reserved"] == 0).all()


def dev_call(fm, reads, off, max_len, prm=None, pp=None, scores=SC, strand=True, ops=True):
    """the device flavour: (hits, strand, pairs, ops slots, ops stride, totals)"""
    prm = prm or SeedParams()
    R = len(off) - 1
    stride = 2 * max_len + 2 * prm.pad + 4
    d_reads = torch.from_numpy(reads).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.zeros(R * 96, dtype=torch.uint8, device=DEV)
    d_strand = torch.full((R,), 77, dtype=torch.uint8, device=DEV)
    d_pairs = torch.full((max(R // 2, 1) * 16,), 0x55, dtype=torch.uint8, device=DEV)
    d_ops = torch.zeros(R * stride, dtype=torch.uint8, device=DEV)
    tot = np.zeros(2, dtype=np.uint64)
    seed_extend_pairs_dev(fm, Scoring.from_scores(*scores), R // 2, d_reads.data_ptr(), d_off.data_ptr(), max_len, d_hits.data_ptr(),
                          d_pairs.data_ptr(), d_strand.data_ptr() if strand else 0, d_ops.data_ptr() if ops else 0, stride if ops else 0,
                          prm, pp, torch.cuda.current_stream().cuda_stream, tot)
    torch.cuda.synchronize()
    return (d_hits.cpu().numpy().view(_lib.SEED_HIT_DTYPE), d_strand.cpu().numpy(), d_pairs.cpu().numpy().view(_lib.PAIR_HIT_DTYPE)[:R // 2],
            d_ops.cpu().numpy(), stride, tot)


def strands_dev(fm, reads, off, max_len, prm=None):
    prm = prm or SeedParams()
    R = len(off) - 1
    stride = 2 * max_len + 2 * prm.pad + 4
    d_reads = torch.from_numpy(reads).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.zeros(R * 96, dtype=torch.uint8, device=DEV)
    d_strand = torch.full((R,), 77, dtype=torch.uint8, device=DEV)
    d_ops = torch.zeros(R * stride, dtype=torch.uint8, device=DEV)
    tot = np.zeros(2, dtype=np.uint64)
    seed_extend_strands_dev(fm, Scoring.from_scores(*SC), R, d_reads.data_ptr(), d_off.data_ptr(), max_len, d_hits.data_ptr(),
                            d_strand.data_ptr(), d_ops.data_ptr(), stride, prm, _lib.STRAND_BOTH, torch.cuda.current_stream().cuda_stream,
                            tot)
    torch.cuda.synchronize()
    return d_hits.cpu().numpy().view(_lib.SEED_HIT_DTYPE), d_strand.cpu().numpy(), d_ops.cpu().numpy(), tot


@pytest.mark.parametrize("sampled", [0, 8])
@pytest.mark.parametrize("ragged", [False, True])
def test_pairs_match_the_oracle(sampled, ragged):
    g, text, reads, off, org, rev = make_case(ragged=ragged)
    sa, b, ls, fm = build(text, sampled)
    attach_text(fm, text)
    pp = PairParams(0, 1000, 17)
    er, ep, cands = oracle_pairs(b, ls, sa, text, len(g), reads, off, pp)
    # the restatement, pinned: its per-read best on both strands is the oracle's composition joined over the strands
    ohits, ostrand, _, _ = oracle_strands(b, ls, sa, text, len(g), reads, off)
    for r in range(len(off) - 1):
        pk = po.strand_best(cands[2 * r], cands[2 * r + 1])
        assert (HIT_NONE if pk is None else pk[0]) == ostrand[r], r
        assert len(cands[2 * r]) + len(cands[2 * r + 1]) == ohits["n_candidates"][r], r
        if pk is not None:
            c = cands[2 * r + pk[0]][pk[1]]
            assert (c["score"], c["ref_start"], c["ref_end"]) == (ohits["aln"]["score"][r], ohits["ref_start"][r], ohits["ref_end"][r]), r
    hits, strand, pairs, ops = seed_extend_pairs_arrays(fm, Scoring.from_scores(*SC), reads, off, pair_params=pp)
    check(hits, strand, pairs, ops, er, ep)
    dh, ds, dp, dops, stride, tot = dev_call(fm, reads, off, int(np.diff(off).max()), pp=pp)
    check(dh, ds, dp, dops, er, ep)
    R = len(off) - 1
    assert (dh["aln"]["ops_off"] == (np.arange(R) + 1) * stride - dh["aln"]["n_ops"]).all()
    assert int(tot[0]) == int(ohits["n_seed_hits"].sum()) and int(tot[1]) == int(ohits["n_candidates"].sum())
    proper = pairs["proper"].astype(bool)
    if not ragged:
        assert proper[:-20].mean() > 0.9 and not proper[-10:].any()
        home = np.abs(hits["ref_start"].astype(np.int64) - org) <= 8
        both = (home[0::2] & home[1::2])[:-20]
        assert both.mean() > 0.9
        # a proper pair's mates are on opposite strands, and its span is the fragment's
        assert (strand[0::2][proper] != strand[1::2][proper]).all()
        frag = np.maximum(org[0::2], org[1::2]) + 150 - np.minimum(org[0::2], org[1::2])
        ok = proper[:-20] & both
        assert (np.abs(pairs["span"][:-20][ok].astype(np.int64) - frag[:-20][ok]) <= 16).mean() > 0.95


def test_repeats_are_resolved_by_the_partner_mate():
    """a 1.2 kb segment duplicated and a 400 bp segment planted 60 times: with one mate inside a copy and the other in unique
    sequence, the unique partner settles the copy; the strands call places most repeat mates at the first copy"""
    n_text, L = 400_000, 150
    g = synth.random_dna(n_text, seed=61).copy()
    g[300_000:301_200] = g[20_000:21_200]
    unit = g[40_000:40_400].copy()
    planted = 50_000 + np.arange(60) * 4_000
    for p0 in planted:
        g[p0:p0 + 400] = unit
    text = np.append(g, np.uint8(ord("$")))
    rng = np.random.default_rng(8)
    # (fragment start, length, is the repeat mate mate 1 (in the copy) or not)
    dup = np.concatenate([20_000 + rng.integers(950, 1051, size=30), 300_000 + rng.integers(950, 1051, size=30)])
    rep = np.concatenate([planted, [40_000]]) + rng.integers(150, 251, size=61)
    s = np.concatenate([dup, rep, rep[:40]])
    frag = np.full(len(s), 400)
    frag[-40:] = 300  # both mates inside a planted copy: 61 x 61 candidates per orientation
    s[-40:] = np.concatenate([planted, [40_000]])[:40] + rng.integers(0, 101, size=40)
    swap = rng.integers(0, 2, size=len(s)).astype(bool)
    R, org, rev = mates_at(g, s, frag, L, 91, swap)
    reads, off = flat_of(list(R))
    sa, b, ls, fm = build(text, 0)
    attach_text(fm, text)
    prm = SeedParams(20, 10, 64, 25)
    pp = PairParams(0, 1000, 17)
    hits, strand, pairs, ops = seed_extend_pairs_arrays(fm, Scoring.from_scores(*SC), reads, off, params=prm, pair_params=pp)
    er, ep, cands = oracle_pairs(b, ls, sa, text, n_text, reads, off, pp, seed_len=20, stride=10, max_occ=64, pad=25)
    check(hits, strand, pairs, ops, er, ep)
    n1 = len(dup) + len(rep)
    home = np.abs(hits["ref_start"].astype(np.int64) - org) <= 8
    assert (home[0::2] & home[1::2])[:n1].mean() >= 0.95
    assert max(len(c) for c in cands) >= 60 and (pairs["n_proper"][n1:] >= 60).mean() > 0.9
    in_copy = np.where(swap[:n1], 1, 0) + 2 * np.arange(n1)  # the repeat mate of each pair
    sh, ss, _ = seed_extend_strands_arrays(fm, Scoring.from_scores(*SC), reads, off, params=prm)
    shome = np.abs(sh["ref_start"].astype(np.int64) - org) <= 8
    assert shome[in_copy].mean() < 0.6
    assert (hits["ref_start"][in_copy] != sh["ref_start"][in_copy]).any()


def test_improper_pairs_fall_back_to_the_strands_call():
    """spans outside the range, chimeric pairs and pairs with an unmappable mate: never proper, and hits, strand, operation
    slots and totals bit for bit those of the strands call on the same reads"""
    n_text, L = 200_000, 150
    g = synth.random_dna(n_text, seed=71).copy()
    text = np.append(g, np.uint8(ord("$")))
    rng = np.random.default_rng(4)
    s = rng.integers(0, n_text - 1_200, size=300)
    frag = np.concatenate([rng.integers(900, 1_100, size=150), rng.integers(300, 500, size=150)])
    R, org, rev = mates_at(g, s, frag, L, 92, rng.integers(0, 2, size=300).astype(bool))
    R = R.copy()
    R[2 * np.arange(150, 220) + 1] = R[2 * np.arange(0, 70) + 1]   # chimeric: mate 2 of an unrelated pair
    R[2 * np.arange(220, 300) + 1] = synth.random_dna(80 * L, seed=6).reshape(80, L)  # an unmappable mate 2
    reads, off = flat_of(list(R))
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    pp = PairParams(300, 600, 17)
    hits, strand, pairs, ops, stride, tot = dev_call(fm, reads, off, L, pp=pp)
    sh, ss, sops, stot = strands_dev(fm, reads, off, L)
    assert not pairs["proper"].any() and (pairs["span"] == 0).all()
    assert hits.view(np.uint8).tobytes() == sh.view(np.uint8).tobytes()
    assert (strand == ss).all() and ops.tobytes() == sops.tobytes() and (tot == stot).all()
    assert (ss[2 * np.arange(220, 300) + 1] == HIT_NONE).mean() > 0.9
    er, ep, _ = oracle_pairs(b, ls, sa, text, n_text, reads, off, pp)
    check(hits, strand, pairs, ops, er, ep)


def test_pen_unpaired_at_its_edge():
    """mate 2 drawn from a distant copy of its locus; the copy next to mate 1 differs in k bases: the proper pair gives up
    d = best1 + best2 - pair_sum > 0.  pen_unpaired = d: proper; d - 1: not"""
    n_text, L = 200_000, 150
    g = synth.random_dna(n_text, seed=81).copy()
    rng = np.random.default_rng(5)
    s = 10_000 + np.arange(40) * 2_000
    frag = np.full(40, 400)
    far = 120_000 + np.arange(40) * 2_000
    for k, (a, f) in enumerate(zip(s, far)):
        near = a + 400 - L
        g[f:f + L] = g[near:near + L]
        for q in rng.choice(np.arange(30, L - 30), size=1 + k % 4, replace=False):  # 1..4 differences in the near copy
            g[near + q] = ord("A") if g[near + q] != ord("A") else ord("C")
    text = np.append(g, np.uint8(ord("$")))
    org = np.stack([s, far], axis=1).reshape(-1)
    refs = np.stack([g[o:o + L] for o in org])
    refs[1::2] = [np.frombuffer(dna.revcomp(x.tobytes()), np.uint8) for x in refs[1::2]]
    reads, off = flat_of(list(refs))
    sa, b, ls, fm = build(text, 0)
    attach_text(fm, text)
    er, ep, cands = oracle_pairs(b, ls, sa, text, n_text, reads, off, PairParams(0, 1000, 10**6))
    d = {}
    for p in range(40):
        assert ep[p][0]  # proper with an unlimited pen_unpaired
        pair_sum = sum(c["score"] for _, c, _, _ in er[2 * p:2 * p + 2])
        o1 = po.strand_best(cands[4 * p], cands[4 * p + 1])
        o2 = po.strand_best(cands[4 * p + 2], cands[4 * p + 3])
        own = cands[4 * p + o1[0]][o1[1]]["score"] + cands[4 * p + 2 + o2[0]][o2[1]]["score"]
        d.setdefault(own - pair_sum, []).append(p)
    assert len([k for k in d if k > 0]) >= 2
    for dd, ps in d.items():
        if dd <= 0:
            continue
        for pen, want in ((dd, 1), (dd - 1, 0)):
            pp = PairParams(0, 1000, pen)
            hits, strand, pairs, ops = seed_extend_pairs_arrays(fm, Scoring.from_scores(*SC), reads, off, pair_params=pp)
            assert (pairs["proper"][ps] == want).all(), (dd, pen)
            er2, ep2, _ = oracle_pairs(b, ls, sa, text, n_text, reads, off, pp)
            check(hits, strand, pairs, ops, er2, ep2)


def test_span_at_its_edges():
    g, text, reads, off, org, rev = make_case(n_text=120_000, n_pairs=200)
    sa, b, ls, fm = build(text, 4)
    attach_text(fm, text)
    hits, strand, pairs, ops = seed_extend_pairs_arrays(fm, Scoring.from_scores(*SC), reads, off, pair_params=PairParams(0, 1000, 17))
    p = int(np.nonzero(pairs["proper"])[0][0])
    S = int(pairs["span"][p])
    for lo, hi, want in ((S, S, 1), (S + 1, 10_000, 0), (0, S - 1, 0)):
        pp = PairParams(lo, hi, 17)
        hits, strand, pairs2, ops = seed_extend_pairs_arrays(fm, Scoring.from_scores(*SC), reads, off, pair_params=pp)
        er, ep, _ = oracle_pairs(b, ls, sa, text, len(g), reads, off, pp)
        check(hits, strand, pairs2, ops, er, ep)
        assert pairs2["proper"][p] == want, (lo, hi)
        if want:
            assert int(pairs2["span"][p]) == S


@pytest.mark.parametrize("chunk", [1, 6, 7, 0])
def test_passes_never_split_a_pair(chunk):
    g, text, reads, off, _, _ = make_case(n_text=120_000, n_pairs=101)
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    want = dev_call(fm, reads, off, 150)
    fm.ctx.set_option("seed_chunk_reads", chunk)
    try:
        got = dev_call(fm, reads, off, 150)
        hh, hs, hp, hops = seed_extend_pairs_arrays(fm, Scoring.from_scores(*SC), reads, off)
    finally:
        fm.ctx.set_option("seed_chunk_reads", 0)
    for a, b_ in zip(got, want):
        assert np.asarray(a).tobytes() == np.asarray(b_).tobytes()
    R = len(off) - 1
    assert (got[0]["aln"]["ops_off"] == (np.arange(R) + 1) * got[4] - got[0]["aln"]["n_ops"]).all()
    assert (hp.tobytes() == got[2].tobytes()) and (hs == got[1]).all()


def test_arguments():
    g, text, reads, off, _, _ = make_case(n_text=60_000, n_pairs=50, L=100)
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    sc = Scoring.from_scores(*SC)
    for bad in (PairParams(501, 500, 0), PairParams(0, 500, -1)):
        with pytest.raises(_lib.BiogpuError) as e:
            seed_extend_pairs_arrays(fm, sc, reads, off, pair_params=bad)
        assert e.value.status == INVALID_ARG
        with pytest.raises(_lib.BiogpuError) as e:
            dev_call(fm, reads, off, 100, pp=bad)
        assert e.value.status == INVALID_ARG
    L = _lib.lib()
    pc, pp = SeedParams().to_c(), PairParams().to_c()
    c_sc = sc.to_c()
    hits = np.zeros(100, dtype=_lib.SEED_HIT_DTYPE)
    pairs = np.zeros(50, dtype=_lib.PAIR_HIT_DTYPE)
    import ctypes as C
    used = C.c_uint64(0)
    assert L.bg_seed_extend_pairs_batch(fm.h, C.byref(c_sc), C.byref(pc), C.byref(pp), 50, reads.ctypes.data, off.ctypes.data,
                                        hits.ctypes.data, None, None, None, 0, C.byref(used)) == INVALID_ARG  # no pairs
    assert L.bg_seed_extend_pairs_batch(fm.h, C.byref(c_sc), C.byref(pc), C.byref(pp), 50, reads.ctypes.data, off.ctypes.data,
                                        None, None, pairs.ctypes.data, None, 0, C.byref(used)) == INVALID_ARG  # no hits
    assert L.bg_seed_extend_pairs_batch(fm.h, C.byref(c_sc), C.byref(pc), None, 50, reads.ctypes.data, off.ctypes.data,
                                        hits.ctypes.data, None, pairs.ctypes.data, None, 0, C.byref(used)) == INVALID_ARG
    d_reads = torch.from_numpy(reads).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.zeros(100 * 96, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.BiogpuError) as e:  # no pairs
        seed_extend_pairs_dev(fm, sc, 50, d_reads.data_ptr(), d_off.data_ptr(), 100, d_hits.data_ptr(), 0)
    assert e.value.status == INVALID_ARG
    # none at all
    assert L.bg_seed_extend_pairs_batch(fm.h, C.byref(c_sc), C.byref(pc), C.byref(pp), 0, reads.ctypes.data, off.ctypes.data,
                                        None, None, pairs.ctypes.data, None, 0, C.byref(used)) == 0
    # strand and operations are optional; the result is the same
    hits2, strand2, pairs2, _ = seed_extend_pairs_arrays(fm, sc, reads, off, want_ops=False)
    dh, _, dp, _, _, _ = dev_call(fm, reads, off, 100, strand=False, ops=False)
    assert (dh["ref_start"] == hits2["ref_start"]).all() and dp.tobytes() == pairs2.tobytes()


def test_seed_outside_the_alphabet_answers_every_pair():
    g, text, reads, off, _, _ = make_case(n_text=60_000, n_pairs=100, L=150)
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    reads = reads.copy()
    reads[5 * 150 + 37] = ord("X")  # read 5 = mate 2 of pair 2
    sc = Scoring.from_scores(*SC)
    with pytest.raises(_lib.AlphabetError):
        seed_extend_pairs_arrays(fm, sc, reads, off)
    hits, strand, pairs, _ = seed_extend_pairs_arrays(fm, sc, reads, off, allow_out_of_alphabet=True)
    clean = np.where(np.arange(len(reads)) == 5 * 150 + 37, ord("A"), reads).astype(np.uint8)
    chits, cstrand, cpairs, _ = seed_extend_pairs_arrays(fm, sc, clean, off)
    keep = np.arange(200) // 2 != 2
    for f in ("n_candidates", "ref_start", "ref_end"):
        assert (hits[f][keep] == chits[f][keep]).all()
    assert (strand[keep] == cstrand[keep]).all()
    assert (pairs[np.arange(100) != 2].tobytes() == cpairs[np.arange(100) != 2].tobytes())
    assert hits["aln"]["score"][5] > MIN_SCORE


def test_wide_layout_with_n_runs():
    """the 64-bit index layout (fm_wide_from = 1: proposals sorted as uint64), raw and sampled suffix arrays, N runs"""
    g, text, reads, off, _, _ = make_case(n_text=120_000, n_pairs=300)
    text = text.copy()
    text[30_000:30_040] = ord("N")
    text[np.random.default_rng(2).integers(0, 119_000, size=20)] = ord("N")
    reads = reads.copy()
    for r in range(0, 500, 7):
        reads[int(off[r]) + 60:int(off[r]) + 64] = ord("N")
    sa = suffix_array(text)
    b = bwt(text, sa)
    ls = less(b, ALPHA)
    pp = PairParams(0, 1000, 17)
    er, ep, _ = oracle_pairs(b, ls, sa, text, len(text) - 1, reads, off, pp)
    for sampled in (0, 8):
        ctx = _lib.Context(0)
        ctx.set_option("fm_wide_from", 1)
        ctx.set_option("fm_wide_sb_shift", 2)
        fm = FMIndex(b, ls, Occ(b, 64, ALPHA), ctx=ctx)
        if sampled:
            SampledSuffixArray(sa, text, b, sampled, fmindex=fm)
        else:
            RawSuffixArray(sa, fm)
        attach_text(fm, text)
        hits, strand, pairs, ops = seed_extend_pairs_arrays(fm, Scoring.from_scores(*SC), reads, off, pair_params=pp)
        check(hits, strand, pairs, ops, er, ep)
        assert pairs["proper"][:-20].mean() > 0.85
        fm.close()


def test_read_pairs_from_genome_mirrors_synth():
    g = synth.random_dna(80_000, seed=3)
    text = np.append(g, np.uint8(ord("$")))
    from rust_bio_amd import synth_gpu
    r, o, rv = synth.read_pairs(text, 3000, 150, seed=7, chunk=1000)
    r2, o2, rv2 = synth_gpu.read_pairs_from_genome(torch.from_numpy(text).to(DEV), 3000, 150, seed=7, chunk=1000)
    assert (r == r2.cpu().numpy()).all() and (o == o2.cpu().numpy()).all() and (rv == rv2.cpu().numpy()).all()
