"""Runner-up loci and MAPQ in seed-and-extend (`bg_seed_extend_multi_batch[_dev]`) against a CPU statement of the rule
(tests/multi_oracle.py): every candidate of every (read, strand) restated on the oracle's own calls by pair_oracle.candidates, then
the multi rule of include/biogpu.h.  Every field of every slot, the complete operations of every reported hit, strand, the
multi records, the unused slots and the reserved bytes, read by read; slot 0 against the strands call.

The main case (`make_case`) under `multi_oracle` alone, K = 4, both strands, of 680 reads:
  fixed-length reads   n_loci >= 2: 269, n_loci >= 3: 115, 0 < mapq < cap: 109, loci != plain top K: 76
  ragged reads         n_loci >= 2: 232, n_loci >= 3: 84, 0 < mapq < cap: 85, loci != plain top K: 59
(the floors the test asserts are the ones the feature was specified with: 100, 20, 20 and 10)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import multi_oracle as mo
import oracle_py as orc
from rust_bio_amd import _lib, synth
from rust_bio_amd.alphabets import dna
from rust_bio_amd.bwt import Occ, bwt, less
from rust_bio_amd.fmindex import FMIndex
from rust_bio_amd.pairwise import MIN_SCORE, Scoring
from rust_bio_amd.pipeline import (MultiParams, SeedParams, attach_text, seed_extend_multi_arrays, seed_extend_multi_dev,
                                   seed_extend_strands_arrays)
from rust_bio_amd.suffix_array import RawSuffixArray, SampledSuffixArray, suffix_array
from test_gpu_pipeline import ALPHA, build
from test_gpu_seed_extend_strands import dev_call as strands_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID_ARG, OUT_OF_ALPHABET = -1, -7
HIT_FORWARD, HIT_REVERSE, HIT_NONE = _lib.HIT_FORWARD, _lib.HIT_REVERSE, _lib.HIT_NONE
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
INT32_MIN = -2**31
SC = (-5, -1, 1, -1)
L = 150
# the planted repeats of make_case: (name, length, the text offsets of the copies)
TWO, THREE, PALI, TANDEM = (20_000, 150_000), (40_000, 100_000, 200_000), 250_000, 270_000
REP = 600


def rc(a):
    return np.frombuffer(dna.revcomp(a.tobytes()), np.uint8)


def flat_of(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.ascontiguousarray(np.concatenate(seqs)), off


@functools.lru_cache(maxsize=None)
def make_case(ragged=False):
    """A 300 kbp genome with: an exact 2-copy repeat (600 bp); a 3-copy repeat whose second copy differs from the first in every
    50th base and whose third in every 25th, so the three score 2 x (differences under the read) apart; a 400 bp palindrome
    (X revcomp(X): it maps on both strands at one place); a tandem run (a 40 bp unit 15 times).  Reads of 150 bases mutated like
    the bench reads, every second one turned to the other strand: 120 from the 2-copy repeat, 120 from the 3-copy one, 40 from
    the palindrome, 40 from the tandem run, 320 from unique sequence, 40 unmappable.  Returns (g, text, reads, off, kind[R]) with
    kind in "two", "three", "pali", "tandem", "unique", "none"."""
    n_text = 300_000
    g = synth.random_dna(n_text, seed=41).copy()
    g[TWO[1]:TWO[1] + REP] = g[TWO[0]:TWO[0] + REP]
    for k, at in enumerate(THREE[1:]):
        g[at:at + REP] = g[THREE[0]:THREE[0] + REP]
        for q in range(7 + 3 * k, REP, 50 if k == 0 else 25):
            g[at + q] = ord("A") if g[at + q] != ord("A") else ord("C")
    x = g[PALI:PALI + 200].copy()
    g[PALI:PALI + 400] = np.concatenate([x, rc(x)])
    g[TANDEM:TANDEM + 600] = np.tile(g[TANDEM:TANDEM + 40], 15)
    text = np.append(g, np.uint8(ord("$")))
    rng = np.random.default_rng(17)
    starts, kind = [], []

    def add(name, n, lo, hi):
        starts.extend(int(s) for s in rng.integers(lo, hi, size=n))
        kind.extend([name] * n)
    for at in TWO:
        add("two", 60, at + 30, at + REP - L - 30)  # the whole window inside the copy: both copies align alike
    for at in THREE:
        add("three", 40, at + 30, at + REP - L - 30)
    add("pali", 40, PALI + 100, PALI + 151)  # centred: the read and its revcomp cover the same bases
    add("tandem", 40, TANDEM + 30, TANDEM + 600 - L - 30)
    planted = [(a, a + REP) for a in TWO + THREE] + [(PALI, PALI + 400), (TANDEM, TANDEM + 600)]
    while kind.count("unique") < 320:
        s = int(rng.integers(0, n_text - L))
        if all(s + L + 30 < a or s > e + 30 for a, e in planted):
            starts.append(s)
            kind.append("unique")
    refs = np.stack([g[s:s + L] for s in starts])
    reads, _ = synth.mutate_fixed(refs, 78, 0.04, 0.005, 0.005)
    reads = np.concatenate([reads, synth.random_dna(40 * L, seed=6).reshape(40, L)])
    kind += ["none"] * 40
    R = len(kind)
    for r in range(1, R, 2):
        reads[r] = rc(reads[r])
    order = np.random.default_rng(5).permutation(R)  # every kind in every pass and wavefront
    reads, kind = reads[order], np.array(kind)[order]
    seqs = list(reads)
    if ragged:
        lens = np.random.default_rng(3).integers(15, L + 1, size=R)
        lens[:300] = L
        seqs = [reads[r, :lens[r]] for r in range(R)]
    flat, off = flat_of(seqs)
    return g, text, flat, off, kind


def index_arrays(text):
    sa = suffix_array(text)
    b = bwt(text, sa)
    return sa, b, less(b, ALPHA)


def oracle_cands(b, ls, sa, text, n_text, reads, off, scores=SC, **kw):
    """the candidates and seed hits of the virtual reads (read, revcomp) x n"""
    vr, voff = mo.virtual_reads(reads, off)
    return mo.candidates(orc, b, ls, orc.Occ(b, 64, ALPHA), sa, text, n_text, orc.make_scoring(*scores), vr, voff, **kw)


def for_strands(cands, nh, strands):
    """the virtual reads' lists as multi_oracle.expected wants them for `strands`"""
    if strands == 3:
        return cands, nh
    return cands[strands - 1::2], nh[strands - 1::2]


@functools.lru_cache(maxsize=None)
def main_oracle(ragged):
    g, text, reads, off, kind = make_case(ragged)
    sa, b, ls = index_arrays(text)
    return oracle_cands(b, ls, sa, text, len(g), reads, off)


def vacuity_counts(cands, nh, n, K=4, cap=60):
    """what the main case exercises, from multi_oracle alone: reads with n_loci >= 2, with n_loci >= 3, with 0 < mapq < cap, and
    reads whose loci differ from the plain top K by score"""
    exp = mo.expected(cands, nh, n, 3, K, INT32_MIN, cap)
    differ = 0
    for r in range(n):
        picks = mo.multi_rule(cands[2 * r], cands[2 * r + 1], K, INT32_MIN, cap)[0]
        differ += picks != mo.top_k(cands[2 * r], cands[2 * r + 1], K)
    return (sum(e[4] >= 2 for e in exp), sum(e[4] >= 3 for e in exp), sum(0 < e[5] < cap for e in exp), differ)


def check(hits, strand, multi, ops, exp, K, stride=None):
    """the call's outputs against the expectation: every field of every slot, the reported hits' complete operations, the records.
    `stride`: the device flavour's operation slots; None: the host flavour's compacted operations.  Returns the reads compared."""
    hits, strand = hits.reshape(-1, K), strand.reshape(-1, K)
    assert len(hits) == len(exp) == len(multi)
    used = 0
    for r, (slots, nc, nsh, sub, n_loci, mapq) in enumerate(exp):
        m = multi[r]
        assert (int(m["sub_score"]), int(m["n_loci"]), int(m["n_reported"]), int(m["mapq"])) == (sub, n_loci, min(n_loci, K), mapq), r
        for k, (st, c) in enumerate(slots):
            h = hits[r, k]
            assert strand[r, k] == st, (r, k)
            assert h["n_candidates"] == nc and h["n_seed_hits"] == nsh, (r, k)
            if stride is None:
                assert int(h["aln"]["ops_off"]) == used, (r, k)
            else:
                assert int(h["aln"]["ops_off"]) == (r * K + k + 1) * stride - int(h["aln"]["n_ops"]), (r, k)
            if c is None:
                assert h["aln"]["score"] == MIN_SCORE and h["aln"]["n_ops"] == 0, (r, k)
                assert h["ref_start"] == NONE and h["ref_end"] == NONE and h["window_start"] == NONE, (r, k)
                continue
            for f in ("score", "xstart", "xend", "ystart", "yend", "xlen", "ylen", "n_ops"):
                assert int(h["aln"][f]) == int(c["rec"][f]), (r, k, f)
            assert h["aln"]["mode"] == 2 and h["aln"]["status"] == 0
            assert (int(h["window_start"]), int(h["ref_start"]), int(h["ref_end"])) == (c["wlo"], c["ref_start"], c["ref_end"]), (r, k)
            n, o = int(h["aln"]["n_ops"]), int(h["aln"]["ops_off"])
            assert (ops[o:o + n] == c["ops"]).all(), (r, k)
            used += n
    assert (multi["reserved"] == 0).all()
    if stride is None:
        assert used == len(ops)
    return len(exp)


def dev_call(fm, reads, off, max_len, mp, prm=None, strands=3, scores=SC, strand=True, ops=True):
    """the device flavour: (hits, strand, multi, ops slots, ops stride, totals)"""
    prm = prm or SeedParams()
    R, K = len(off) - 1, mp.max_hits
    stride = 2 * max_len + 2 * prm.pad + 4
    d_reads = torch.from_numpy(reads).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.full((R * K * 96,), 0x33, dtype=torch.uint8, device=DEV)
    d_strand = torch.full((R * K,), 77, dtype=torch.uint8, device=DEV)
    d_multi = torch.full((max(R, 1) * 16,), 0x55, dtype=torch.uint8, device=DEV)
    d_ops = torch.zeros(R * K * stride, dtype=torch.uint8, device=DEV)
    tot = np.zeros(2, dtype=np.uint64)
    seed_extend_multi_dev(fm, Scoring.from_scores(*scores), R, d_reads.data_ptr(), d_off.data_ptr(), max_len, d_hits.data_ptr(),
                          d_multi.data_ptr(), d_strand.data_ptr() if strand else 0, d_ops.data_ptr() if ops else 0, stride if ops else 0,
                          prm, mp, strands, torch.cuda.current_stream().cuda_stream, tot)
    torch.cuda.synchronize()
    return (d_hits.cpu().numpy().view(_lib.SEED_HIT_DTYPE), d_strand.cpu().numpy(), d_multi.cpu().numpy().view(_lib.MULTI_HIT_DTYPE)[:R],
            d_ops.cpu().numpy(), stride, tot)


def slot0_equals_strands(fm, reads, off, max_len, strands, K, prm=None):
    """slot 0 of the multi call (min_score = INT32_MIN) against the strands call, host and device flavours: every field but the
    slot-dependent ops_off, the strand, the complete operations, the totals"""
    sc = Scoring.from_scores(*SC)
    mp = MultiParams(K, INT32_MIN, 60)
    sh, ss, sops = seed_extend_strands_arrays(fm, sc, reads, off, params=prm, strands=strands)
    mh, ms, mm, mops = seed_extend_multi_arrays(fm, sc, reads, off, params=prm, multi_params=mp, strands=strands)
    dsh, dss, dsops, stride, stot = strands_dev(fm, reads, off, max_len, prm=prm, strands=strands)
    dmh, dms, dmm, dmops, mstride, mtot = dev_call(fm, reads, off, max_len, mp, prm=prm, strands=strands)
    assert stride == mstride and (stot == mtot).all()
    dmh, dms = dmh.reshape(-1, K), dms.reshape(-1, K)
    for want, wstrand, wops, got, gstrand, gops in ((sh, ss, sops, mh, ms, mops), (dsh, dss, dsops, dmh, dms, dmops)):
        a, b_ = want.copy(), got[:, 0].copy()
        if K == 1:
            assert (a["aln"]["ops_off"] == b_["aln"]["ops_off"]).all()
        a["aln"]["ops_off"] = b_["aln"]["ops_off"] = 0
        assert a.tobytes() == b_.tobytes()
        assert (wstrand == gstrand[:, 0]).all()
        for r in range(len(want)):
            n = int(want["aln"]["n_ops"][r])
            wo, go = int(want["aln"]["ops_off"][r]), int(got["aln"]["ops_off"][r, 0])
            assert (wops[wo:wo + n] == gops[go:go + n]).all(), r
    assert mm.tobytes() == dmm.tobytes()


@pytest.mark.parametrize("sampled", [0, 8])
@pytest.mark.parametrize("ragged", [False, True])
def test_multi_matches_the_oracle(sampled, ragged):
    g, text, reads, off, kind = make_case(ragged)
    R, max_len = len(off) - 1, int(np.diff(off).max())
    cands, nh = main_oracle(ragged)
    # the case is not vacuous (the counts are in the module docstring)
    n2, n3, mid, differ = vacuity_counts(cands, nh, R)
    assert n2 >= 100 and n3 >= 20 and mid >= 20 and differ >= 10, (n2, n3, mid, differ)
    sa, b, ls, fm = build(text, sampled)
    attach_text(fm, text)
    sc = Scoring.from_scores(*SC)
    compared = 0
    for strands in (1, 2, 3):
        cs, ns = for_strands(cands, nh, strands)
        for K in (1, 2, 4, 8):
            cap = 60 if K != 2 else 254
            mp = MultiParams(K, INT32_MIN, cap)
            exp = mo.expected(cs, ns, R, strands, K, INT32_MIN, cap)
            hits, strand, multi, ops = seed_extend_multi_arrays(fm, sc, reads, off, multi_params=mp, strands=strands)
            compared += check(hits, strand, multi, ops, exp, K)
            dh, ds, dm, dops, stride, tot = dev_call(fm, reads, off, max_len, mp, strands=strands)
            compared += check(dh, ds, dm, dops, exp, K, stride)
            assert int(tot[0]) == int(sum(ns)) and int(tot[1]) == sum(len(c) for c in cs)
        slot0_equals_strands(fm, reads, off, max_len, strands, 4)
    slot0_equals_strands(fm, reads, off, max_len, 3, 1)
    assert compared == 3 * 4 * 2 * R  # no read left out
    # min_score takes candidates out of the loci and of the runner-up
    mp = MultiParams(4, 120, 60)
    exp = mo.expected(cands, nh, R, 3, 4, 120, 60)
    hits, strand, multi, ops = seed_extend_multi_arrays(fm, sc, reads, off, multi_params=mp)
    check(hits, strand, multi, ops, exp, 4)
    full = mo.expected(cands, nh, R, 3, 4)
    lifted = sum(f[4] >= 2 and f[5] < 60 and e[4] == 1 and e[5] == 60 for e, f in zip(exp, full))  # the runner-up went: MAPQ at the cap
    assert sum(e[4] for e in exp) < sum(e[4] for e in full) and lifted >= 10, lifted
    if not ragged:
        # what a user reads off the result: the exact 2-copy reads have MAPQ 0 and their two loci at the two copies; reads from
        # unique sequence have the cap (a read whose every seed holds a mutation has no candidate: it is unmapped, MAPQ 0)
        mp = MultiParams(4, INT32_MIN, 60)
        hits, strand, multi, ops = seed_extend_multi_arrays(fm, sc, reads, off, multi_params=mp)
        mapped = hits["n_candidates"][:, 0] > 0
        two = (kind == "two") & mapped
        assert (multi["mapq"][kind == "two"] == 0).all() and (multi["n_reported"][two] >= 2).all()
        assert two.sum() >= 0.95 * (kind == "two").sum()
        at = np.sort(hits["ref_start"][two][:, :2].astype(np.int64), axis=1)
        assert (np.abs(at[:, 1] - at[:, 0] - (TWO[1] - TWO[0])) <= 8).all()
        assert (at[:, 0] >= TWO[0]).all() and (at[:, 0] < TWO[0] + REP).all()
        unique = (kind == "unique") & mapped
        assert (multi["mapq"][unique] == 60).all() and unique.sum() >= 0.95 * (kind == "unique").sum()
        assert (multi["mapq"][kind == "none"] == 0).mean() > 0.9
        three = multi["mapq"][kind == "three"]
        assert ((three > 0) & (three < 60)).mean() > 0.85
        assert (multi["n_loci"][kind == "pali"] == 1).mean() > 0.9
    fm.close()


@pytest.mark.parametrize("chunk", [1, 7, 64, 0])
def test_slots_hold_across_passes(chunk):
    g, text, reads, off, kind = make_case(False)
    n = 203
    reads, off = reads[:int(off[n])], off[:n + 1]
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    mp = MultiParams(4, INT32_MIN, 60)
    want = dev_call(fm, reads, off, L, mp)
    wh = seed_extend_multi_arrays(fm, Scoring.from_scores(*SC), reads, off, multi_params=mp)
    fm.ctx.set_option("seed_chunk_reads", chunk)
    try:
        got = dev_call(fm, reads, off, L, mp)
        gh = seed_extend_multi_arrays(fm, Scoring.from_scores(*SC), reads, off, multi_params=mp)
    finally:
        fm.ctx.set_option("seed_chunk_reads", 0)
    for a, b_ in list(zip(got, want)) + list(zip(gh, wh)):
        assert np.asarray(a).tobytes() == np.asarray(b_).tobytes()
    cands, nh = main_oracle(False)
    exp = mo.expected(cands[:2 * n], nh[:2 * n], n, 3, 4)
    check(got[0], got[1], got[2], got[3], exp, 4, got[4])
    check(gh[0], gh[1], gh[2], gh[3], exp, 4)
    fm.close()


def test_wide_layout_with_n_runs():
    """the 64-bit index layout (fm_wide_from = 1: proposals sorted as uint64), raw and sampled suffix arrays, N runs"""
    g, text, reads, off, kind = make_case(False)
    text = text.copy()
    text[30_000:30_040] = ord("N")
    text[np.random.default_rng(2).integers(0, 299_000, size=20)] = ord("N")
    reads = reads.copy()
    for r in range(0, len(off) - 1, 7):
        reads[int(off[r]) + 60:int(off[r]) + 64] = ord("N")
    sa, b, ls = index_arrays(text)
    cands, nh = oracle_cands(b, ls, sa, text, len(text) - 1, reads, off)
    R = len(off) - 1
    mp = MultiParams(4, INT32_MIN, 60)
    exp = mo.expected(cands, nh, R, 3, 4)
    assert sum(e[4] >= 2 for e in exp) >= 100
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
        hits, strand, multi, ops = seed_extend_multi_arrays(fm, Scoring.from_scores(*SC), reads, off, multi_params=mp)
        check(hits, strand, multi, ops, exp, 4)
        dh, ds, dm, dops, stride, tot = dev_call(fm, reads, off, L, mp)
        check(dh, ds, dm, dops, exp, 4, stride)
        fm.close()


def many_candidates_case():
    """15 families of 10-mers, each planted 58 times on either strand of a 400 kbp genome, and a read that is one 10-mer of
    each family: with seed_len = stride = 10 and max_occ = 64 every seed of the read and of its revcomp votes at some 58 places
    (over 1536 candidates: lanes own up to 128 and every mask dword is in use); a 400 bp unit planted 30 times gives reads with
    more than 16"""
    n_text = 400_000
    g = synth.random_dna(n_text, seed=51).copy()
    rng = np.random.default_rng(9)
    fam = synth.random_dna(150, seed=52).copy()
    places = rng.permutation(np.arange(200, n_text - 400, 220))[:15 * 116 + 30]
    for f in range(15):
        seg = fam[10 * f:10 * f + 10]
        for k in range(116):
            p = int(places[f * 116 + k]) + int(rng.integers(0, 40))
            g[p:p + 10] = seg if k < 58 else rc(seg)
    unit = synth.random_dna(400, seed=53)
    unit_at = places[15 * 116:]
    for p in unit_at:
        g[int(p) - 100:int(p) + 300] = unit
    text = np.append(g, np.uint8(ord("$")))
    refs = np.stack([unit[s:s + L] for s in (0, 40, 97, 200, 250)])
    urd, _ = synth.mutate_fixed(refs, 79, 0.04, 0.005, 0.005)
    urd[1::2] = [rc(x) for x in urd[1::2]]
    uniq = np.stack([g[s:s + L] for s in (1_000, 90_000)])
    reads, off = flat_of([fam] + list(urd) + list(uniq) + [rc(fam)])
    return g, text, reads, off


def test_many_candidates_per_lane():
    g, text, reads, off = many_candidates_case()
    prm = SeedParams(10, 10, 64, 25)
    sa, b, ls, fm = build(text, 0)
    attach_text(fm, text)
    cands, nh = oracle_cands(b, ls, sa, text, len(g), reads, off, seed_len=10, stride=10, max_occ=64, pad=25)
    R = len(off) - 1
    per_read = [len(cands[2 * r]) + len(cands[2 * r + 1]) for r in range(R)]
    assert per_read[0] > 1536 and per_read[-1] > 1536 and min(per_read[1:6]) > 16 and max(per_read[1:6]) < 200
    for K, min_score in ((8, INT32_MIN), (1, INT32_MIN), (4, -60)):
        mp = MultiParams(K, min_score, 60)
        exp = mo.expected(cands, nh, R, 3, K, min_score, 60)
        hits, strand, multi, ops = seed_extend_multi_arrays(fm, Scoring.from_scores(*SC), reads, off, params=prm, multi_params=mp)
        check(hits, strand, multi, ops, exp, K)
        dh, ds, dm, dops, stride, tot = dev_call(fm, reads, off, L, mp, prm=prm)
        check(dh, ds, dm, dops, exp, K, stride)
    assert exp[0][4] >= 2
    slot0_equals_strands(fm, reads, off, L, 3, 8, prm=prm)
    fm.close()


def test_arguments():
    g, text, reads, off, kind = make_case(False)
    n = 60
    reads, off = reads[:int(off[n])], off[:n + 1]
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    sc = Scoring.from_scores(*SC)
    for bad in (MultiParams(0, 0, 60), MultiParams(9, 0, 60), MultiParams(4, 0, 255)):
        with pytest.raises(_lib.BiogpuError) as e:
            seed_extend_multi_arrays(fm, sc, reads, off, multi_params=bad)
        assert e.value.status == INVALID_ARG
        with pytest.raises(_lib.BiogpuError) as e:
            dev_call(fm, reads, off, L, bad)
        assert e.value.status == INVALID_ARG
    for strands in (0, 4):
        with pytest.raises(_lib.BiogpuError) as e:
            seed_extend_multi_arrays(fm, sc, reads, off, strands=strands)
        assert e.value.status == INVALID_ARG
    lib = _lib.lib()
    pc, mpc, c_sc = SeedParams().to_c(), MultiParams(2).to_c(), sc.to_c()
    hits = np.zeros(2 * n, dtype=_lib.SEED_HIT_DTYPE)
    multi = np.zeros(n, dtype=_lib.MULTI_HIT_DTYPE)
    used = C.c_uint64(0)

    def host(mp, hits_p, multi_p, n_reads=n):
        return lib.bg_seed_extend_multi_batch(fm.h, C.byref(c_sc), C.byref(pc), mp, 3, n_reads, reads.ctypes.data, off.ctypes.data, hits_p,
                                              None, multi_p, None, 0, C.byref(used))
    assert host(None, hits.ctypes.data, multi.ctypes.data) == INVALID_ARG            # no parameters
    assert host(C.byref(mpc), hits.ctypes.data, None) == INVALID_ARG                 # no records
    assert host(C.byref(mpc), None, multi.ctypes.data) == INVALID_ARG                # no hits
    assert host(C.byref(mpc), None, multi.ctypes.data, 0) == 0                       # none at all
    assert host(C.byref(mpc), hits.ctypes.data, multi.ctypes.data) == 0              # strand and operations are optional
    d_reads = torch.from_numpy(reads).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.zeros(2 * n * 96, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.BiogpuError) as e:  # no records
        seed_extend_multi_dev(fm, sc, n, d_reads.data_ptr(), d_off.data_ptr(), L, d_hits.data_ptr(), 0, multi_params=MultiParams(2))
    assert e.value.status == INVALID_ARG
    d_multi = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    d_ops = torch.zeros(2 * n * 100, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.BiogpuError):  # a stride below the minimum
        seed_extend_multi_dev(fm, sc, n, d_reads.data_ptr(), d_off.data_ptr(), L, d_hits.data_ptr(), d_multi.data_ptr(), 0, d_ops.data_ptr(),
                              100, multi_params=MultiParams(2))
    # without strand and operations the result is the same
    mp = MultiParams(2, INT32_MIN, 60)
    h1, s1, m1, _ = seed_extend_multi_arrays(fm, sc, reads, off, multi_params=mp)
    h2, _, m2, none = seed_extend_multi_arrays(fm, sc, reads, off, multi_params=mp, want_ops=False)
    dh, _, dm, _, _, _ = dev_call(fm, reads, off, L, mp, strand=False, ops=False)
    assert none is None and m1.tobytes() == m2.tobytes() == dm.tobytes()
    for f in ("ref_start", "ref_end", "window_start", "n_candidates"):
        assert (h1[f] == h2[f]).all() and (h1[f].reshape(-1) == dh[f]).all()
    assert (multi["n_loci"] == m1["n_loci"]).all() and (hits["ref_start"].reshape(n, 2) == h1["ref_start"]).all()
    fm.close()


def test_seed_outside_the_alphabet_answers_every_read():
    g, text, reads, off, kind = make_case(False)
    n = 100
    reads, off = reads[:int(off[n])].copy(), off[:n + 1]
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    reads[5 * L + 37] = ord("X")
    sc = Scoring.from_scores(*SC)
    mp = MultiParams(2, INT32_MIN, 60)
    with pytest.raises(_lib.AlphabetError):
        seed_extend_multi_arrays(fm, sc, reads, off, multi_params=mp)
    hits, strand, multi, _ = seed_extend_multi_arrays(fm, sc, reads, off, multi_params=mp, allow_out_of_alphabet=True)
    clean = np.where(np.arange(len(reads)) == 5 * L + 37, ord("A"), reads).astype(np.uint8)
    chits, cstrand, cmulti, _ = seed_extend_multi_arrays(fm, sc, clean, off, multi_params=mp)
    keep = np.arange(n) != 5
    for f in ("n_candidates", "ref_start", "ref_end"):
        assert (hits[f][keep] == chits[f][keep]).all()
    assert (strand[keep] == cstrand[keep]).all() and multi[keep].tobytes() == cmulti[keep].tobytes()
    if kind[5] != "none":
        assert hits["aln"]["score"][5, 0] > MIN_SCORE
    fm.close()
