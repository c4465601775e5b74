"""Seed-and-extend on both strands (`bg_seed_extend_strands_batch[_dev]`, `bg_revcomp_batch_dev`) against the oracle's
composition (oracle/pipeline.cpp, the same one test_gpu_pipeline.py holds the single-strand call to): run once on the reads
and once on their `dna::revcomp`, joined per read by the rule of include/biogpu.h — the highest score wins, the forward
strand on an equal score; counts are sums.  Scores, coordinates, counts, strand and the winner's complete operation list,
read by read."""
import numpy as np
import pytest
import torch

import oracle_py as orc
from rust_bio_amd import _lib, synth
from rust_bio_amd.alphabets import dna
from rust_bio_amd.bwt import Occ, bwt, less
from rust_bio_amd.fmindex import FMIndex
from rust_bio_amd.pairwise import MIN_SCORE, Scoring
from rust_bio_amd.pipeline import (SeedParams, attach_text, revcomp_dev, seed_extend_arrays, seed_extend_dev,
                                   seed_extend_strands_arrays, seed_extend_strands_dev)
from rust_bio_amd.suffix_array import SampledSuffixArray, suffix_array
from test_gpu_pipeline import ALPHA, build, compare, make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID_ARG = -1
HIT_FORWARD, HIT_REVERSE, HIT_NONE = _lib.HIT_FORWARD, _lib.HIT_REVERSE, _lib.HIT_NONE
SC = (-5, -1, 1, -1)


def revcomp_reads(reads, off):
    """dna::revcomp of every read, at the same offsets"""
    out = np.empty_like(reads)
    for r in range(len(off) - 1):
        a, e = int(off[r]), int(off[r + 1])
        out[a:e] = dna.revcomp(reads[a:e])
    return out


def half_reversed(reads, off, n_keep_tail=50):
    """every odd read but the unmappable tail turned into its reverse complement: the other strand of the same locus"""
    R = len(off) - 1
    rev = (np.arange(R) % 2 == 1) & (np.arange(R) < R - n_keep_tail)
    rc = revcomp_reads(reads, off)
    out = reads.copy()
    for r in np.nonzero(rev)[0]:
        out[int(off[r]):int(off[r + 1])] = rc[int(off[r]):int(off[r + 1])]
    return out, rev


def oracle_strands(b, ls, sa, text, n_text, reads, off, strands=3, **kw):
    """the oracle's composition on the reads and on their revcomps, joined: (hits, strand, ops, ops stride)"""
    occ = orc.Occ(b, 64, ALPHA)
    sc = orc.make_scoring(*kw.pop("scores", SC))
    fh, fops, stride = orc.seed_extend_batch(b, ls, occ, sa, text, n_text, sc, reads, off, threads=8, **kw)
    rh, rops, _ = orc.seed_extend_batch(b, ls, occ, sa, text, n_text, sc, revcomp_reads(reads, off), off, threads=8, **kw)
    n = len(off) - 1
    if strands == 1:
        return fh, np.where(fh["aln"]["score"] > MIN_SCORE, HIT_FORWARD, HIT_NONE).astype(np.uint8), fops, stride
    if strands == 2:
        return rh, np.where(rh["aln"]["score"] > MIN_SCORE, HIT_REVERSE, HIT_NONE).astype(np.uint8), rops, stride
    rev = rh["aln"]["score"] > fh["aln"]["score"]  # forward on an equal score (and where neither has a candidate)
    hits = np.where(rev, rh, fh)
    hits["n_candidates"] = fh["n_candidates"] + rh["n_candidates"]
    hits["n_seed_hits"] = fh["n_seed_hits"] + rh["n_seed_hits"]
    ops = np.where(rev[:, None], rops.reshape(n, stride), fops.reshape(n, stride)).reshape(-1)
    strand = np.where(rev, HIT_REVERSE, np.where(fh["aln"]["score"] > MIN_SCORE, HIT_FORWARD, HIT_NONE)).astype(np.uint8)
    return hits, strand, ops, stride


def dev_call(fm, reads, off, max_len, prm=None, strands=3, scores=SC):
    """the device flavour with every optional output: (hits, strand, ops slots, ops stride, totals)"""
    prm = prm or SeedParams()
    R = len(off) - 1
    stride = 2 * max_len + 2 * prm.pad + 4
    d_reads = torch.from_numpy(reads).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.zeros(R * 96, dtype=torch.uint8, device=DEV)
    d_strand = torch.full((R,), 77, dtype=torch.uint8, device=DEV)
    d_ops = torch.zeros(R * stride, dtype=torch.uint8, device=DEV)
    tot = np.zeros(2, dtype=np.uint64)
    seed_extend_strands_dev(fm, Scoring.from_scores(*scores), R, d_reads.data_ptr(), d_off.data_ptr(), max_len, d_hits.data_ptr(),
                            d_strand.data_ptr(), d_ops.data_ptr(), stride, prm, strands, torch.cuda.current_stream().cuda_stream, tot)
    torch.cuda.synchronize()
    return d_hits.cpu().numpy().view(_lib.SEED_HIT_DTYPE), d_strand.cpu().numpy(), d_ops.cpu().numpy(), stride, tot


@pytest.mark.parametrize("sampled", [0, 8])
@pytest.mark.parametrize("ragged", [False, True])
def test_both_strands_match_the_joined_oracle(sampled, ragged):
    g, text, reads, off, starts = make_case(ragged=ragged)
    reads, rev = half_reversed(reads, off)
    sa, b, ls, fm = build(text, sampled)
    attach_text(fm, text)
    hits, strand, ops = seed_extend_strands_arrays(fm, Scoring.from_scores(*SC), reads, off)
    ohits, ostrand, oops, ostride = oracle_strands(b, ls, sa, text, len(g), reads, off)
    mapped = compare(hits, ops, ohits, oops, ostride)
    assert (strand == ostrand).all()
    assert ((strand == HIT_NONE) == ~mapped).all()
    if not ragged:
        mappable = np.arange(len(rev)) < len(rev) - 50
        assert mapped[mappable].mean() > 0.95 and not mapped[~mappable].any()
        want = np.where(rev, HIT_REVERSE, HIT_FORWARD)
        home = (np.abs(hits["ref_start"].astype(np.int64) - starts) <= 8) & (strand == want) & mapped
        assert home[mappable].mean() > 0.9  # at the origin, on the strand the read was drawn from
        # the reverse winners' alignments are of revcomp(read): the whole read, forward text coordinates
        assert (hits["aln"]["xlen"][rev & mapped] == 150).all()
        # the forward-only call leaves the other strand's reads (about half) unmapped
        fwd, _ = seed_extend_arrays(fm, Scoring.from_scores(*SC), reads, off)
        fmapped = fwd["aln"]["score"] > MIN_SCORE
        assert fmapped[rev].mean() < 0.1 and fmapped[mappable & ~rev].mean() > 0.95
        assert 0.4 < fmapped[mappable].mean() < 0.6


def test_one_strand_at_a_time():
    """strands = 1 is bg_seed_extend_batch_dev bit for bit (hits, operation slots, totals); strands = 2 on the reads is the
    same call on their revcomps"""
    g, text, reads, off, _ = make_case(n_text=120_000, R=900, L=120)
    reads, rev = half_reversed(reads, off)
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    R, L, prm = len(off) - 1, 120, SeedParams()
    stride = 2 * L + 2 * prm.pad + 4

    def single(rd):
        d_reads = torch.from_numpy(rd).to(DEV)
        d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
        d_hits = torch.zeros(R * 96, dtype=torch.uint8, device=DEV)
        d_ops = torch.zeros(R * stride, dtype=torch.uint8, device=DEV)
        tot = np.zeros(2, dtype=np.uint64)
        seed_extend_dev(fm, Scoring.from_scores(*SC), R, d_reads.data_ptr(), d_off.data_ptr(), L, d_hits.data_ptr(), d_ops.data_ptr(),
                        stride, prm, torch.cuda.current_stream().cuda_stream, tot)
        torch.cuda.synchronize()
        return d_hits.cpu().numpy(), d_ops.cpu().numpy(), tot

    for strands, rd, code in ((1, reads, HIT_FORWARD), (2, revcomp_reads(reads, off), HIT_REVERSE)):
        want_hits, want_ops, want_tot = single(rd)
        hits, strand, ops, s2, tot = dev_call(fm, reads, off, L, prm, strands)
        assert s2 == stride
        assert hits.view(np.uint8).tobytes() == want_hits.tobytes(), strands
        assert ops.tobytes() == want_ops.tobytes(), strands
        assert (tot == want_tot).all(), strands
        mapped = hits["aln"]["score"] > MIN_SCORE
        assert (strand == np.where(mapped, code, HIT_NONE)).all()
        # the host flavour agrees
        hh, hs, _ = seed_extend_strands_arrays(fm, Scoring.from_scores(*SC), reads, off, strands=strands)
        assert (hh["ref_start"] == hits["ref_start"]).all() and (hs == strand).all()
    # the reverse strand alone maps the reversed reads
    assert (strand[rev & (np.arange(R) < R - 50)] == HIT_REVERSE).mean() > 0.9


def test_equal_scores_on_both_strands_go_to_the_forward_strand():
    """a genome that holds a segment and, elsewhere, its reverse complement: an exact read of the segment scores the same
    on both strands (forward at the segment, reverse at the copy) and the forward strand wins"""
    n_text, L = 80_000, 100
    g = synth.random_dna(n_text, seed=51).copy()
    g[50_000:50_400] = dna.revcomp(g[10_000:10_400])
    text = np.append(g, np.uint8(ord("$")))
    starts = 10_000 + np.arange(60) * 5
    reads = np.ascontiguousarray(np.stack([g[s:s + L] for s in starts]).reshape(-1))
    off = np.arange(61, dtype=np.uint64) * np.uint64(L)
    sa, b, ls, fm = build(text, 4)
    attach_text(fm, text)
    hits, strand, ops = seed_extend_strands_arrays(fm, Scoring.from_scores(*SC), reads, off)
    ohits, ostrand, oops, ostride = oracle_strands(b, ls, sa, text, n_text, reads, off)
    compare(hits, ops, ohits, oops, ostride)
    assert (strand == HIT_FORWARD).all() and (ostrand == HIT_FORWARD).all()
    assert (hits["aln"]["score"] == L).all() and (hits["ref_start"] == starts).all()
    assert (hits["n_candidates"] >= 2).all()  # one placement per strand was aligned
    # the reverse strand alone finds the copy, with the same score
    rh, rs, _ = seed_extend_strands_arrays(fm, Scoring.from_scores(*SC), reads, off, strands=2)
    assert (rs == HIT_REVERSE).all() and (rh["aln"]["score"] == L).all()
    assert (rh["ref_start"] == 50_400 - (starts - 10_000) - L).all()


@pytest.mark.parametrize("chunk", [0, 256, 999])
def test_device_flavour_slots_totals_and_passes(chunk):
    """right-aligned operation slots of the caller's buffer, totals summed over both strands, and passes (seed_chunk_reads
    counts the caller's reads: a pass boundary inside the batch)"""
    g, text, reads, off, _ = make_case(n_text=120_000, R=1500, L=150)
    reads, _ = half_reversed(reads, off)
    sa, b, ls, fm = build(text, 8)
    d_text = torch.from_numpy(text).to(DEV)
    attach_text(fm, d_text=d_text)
    ohits, ostrand, oops, ostride = oracle_strands(b, ls, sa, text, len(g), reads, off)
    fm.ctx.set_option("seed_chunk_reads", chunk)
    try:
        hits, strand, ops, stride, tot = dev_call(fm, reads, off, 150)
    finally:
        fm.ctx.set_option("seed_chunk_reads", 0)
    R = len(off) - 1
    assert (hits["aln"]["ops_off"] == (np.arange(R) + 1) * stride - hits["aln"]["n_ops"]).all()
    compare(hits, ops, ohits, oops, ostride)
    assert (strand == ostrand).all()
    assert int(tot[0]) == int(ohits["n_seed_hits"].sum()) and int(tot[1]) == int(ohits["n_candidates"].sum())


def test_other_parameters_and_scoring():
    g, text, reads, off, _ = make_case(n_text=120_000, R=700, L=100, ragged=True)
    reads, _ = half_reversed(reads, off)
    sa, b, ls, fm = build(text, 4)
    attach_text(fm, text)
    prm = SeedParams(seed_len=16, stride=7, max_occ=4, pad=12)
    hits, strand, ops, _, _ = dev_call(fm, reads, off, 100, prm, 3, scores=(-4, -2, 2, -3))
    ohits, ostrand, oops, ostride = oracle_strands(b, ls, sa, text, len(g), reads, off, seed_len=16, stride=7, max_occ=4, pad=12,
                                                   scores=(-4, -2, 2, -3))
    compare(hits, ops, ohits, oops, ostride)
    assert (strand == ostrand).all()


def test_wide_layout_with_n_runs():
    """the 64-bit index layout (ctx option fm_wide_from = 1; proposals sorted as uint64), raw and sampled suffix arrays, N runs
    in the text and in the reads (N is its own complement)"""
    from rust_bio_amd.suffix_array import RawSuffixArray
    g, text, reads, off, _ = make_case(n_text=120_000, R=800)
    text = text.copy()
    text[30_000:30_040] = ord("N")
    text[np.random.default_rng(2).integers(0, 119_000, size=20)] = ord("N")
    reads, _ = half_reversed(reads, off)
    reads = reads.copy()
    for r in range(0, 700, 7):  # a run of N inside some reads
        reads[int(off[r]) + 60:int(off[r]) + 64] = ord("N")
    sa = suffix_array(text)
    b = bwt(text, sa)
    ls = less(b, ALPHA)
    ohits, ostrand, oops, ostride = oracle_strands(b, ls, sa, text, len(text) - 1, reads, off)
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
        hits, strand, ops = seed_extend_strands_arrays(fm, Scoring.from_scores(*SC), reads, off)
        mapped = compare(hits, ops, ohits, oops, ostride)
        assert (strand == ostrand).all()
        assert mapped[:-50].mean() > 0.9
        fm.close()


def test_seed_outside_the_alphabet_is_reported_on_both_strands():
    g, text, reads, off, _ = make_case(n_text=60_000, R=200, L=100)
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    reads = reads.copy()
    reads[5 * 100 + 37] = ord("X")  # read 5 (X is its own complement: a seed on each strand covers it)
    sc = Scoring.from_scores(*SC)
    with pytest.raises(_lib.AlphabetError):
        seed_extend_strands_arrays(fm, sc, reads, off)
    hits, strand, _ = seed_extend_strands_arrays(fm, sc, reads, off, allow_out_of_alphabet=True)
    clean = np.where(np.arange(len(reads)) == 5 * 100 + 37, ord("A"), reads).astype(np.uint8)
    chits, cstrand, _ = seed_extend_strands_arrays(fm, sc, clean, off)
    keep = np.arange(200) != 5
    for f in ("n_candidates", "ref_start", "ref_end"):
        assert (hits[f][keep] == chits[f][keep]).all()
    assert (strand[keep] == cstrand[keep]).all()
    assert hits["aln"]["score"][5] > MIN_SCORE and strand[5] == HIT_FORWARD


def test_arguments():
    g, text, reads, off, _ = make_case(n_text=60_000, R=100, L=80)
    sa = suffix_array(text)
    b = bwt(text, sa)
    ls = less(b, ALPHA)
    bare = FMIndex(b, ls, Occ(b, 64, ALPHA))
    with pytest.raises(_lib.BiogpuError):  # no text, no suffix array
        seed_extend_strands_arrays(bare, Scoring.from_scores(*SC), reads, off)
    _, _, _, fm = build(text, 8)
    with pytest.raises(_lib.BiogpuError):  # a suffix array but no text
        seed_extend_strands_arrays(fm, Scoring.from_scores(*SC), reads, off)
    attach_text(fm, text)
    for bad in (0, 4):
        with pytest.raises(_lib.BiogpuError) as e:
            seed_extend_strands_arrays(fm, Scoring.from_scores(*SC), reads, off, strands=bad)
        assert e.value.status == INVALID_ARG
        with pytest.raises(_lib.BiogpuError) as e:
            dev_call(fm, reads, off, 80, strands=bad)
        assert e.value.status == INVALID_ARG
    # the strand array is optional
    hits, strand, _ = seed_extend_strands_arrays(fm, Scoring.from_scores(*SC), reads, off)
    R = len(off) - 1
    d_reads = torch.from_numpy(reads).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.zeros(R * 96, dtype=torch.uint8, device=DEV)
    seed_extend_strands_dev(fm, Scoring.from_scores(*SC), R, d_reads.data_ptr(), d_off.data_ptr(), 80, d_hits.data_ptr(),
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dh = d_hits.cpu().numpy().view(_lib.SEED_HIT_DTYPE)
    assert (dh["ref_start"] == hits["ref_start"]).all() and (dh["aln"]["score"] == hits["aln"]["score"]).all()


def test_revcomp_batch_dev_against_dna_revcomp():
    rng = np.random.default_rng(9)
    seqs = [np.arange(256, dtype=np.uint8), np.zeros(0, np.uint8), np.array([ord("A")], np.uint8), np.zeros(0, np.uint8),
            rng.integers(0, 256, size=65535).astype(np.uint8), np.array([ord("$")], np.uint8)]
    seqs += [np.frombuffer(b"ACGTNacgtnRYSWKMBDHV"[:k], np.uint8) for k in range(21)]
    seqs += [rng.choice(np.frombuffer(b"ACGTNacgtn", np.uint8), size=int(rng.integers(0, 300))) for _ in range(500)]
    flat, off = _lib.concat([s.tobytes() for s in seqs])
    d_in = torch.from_numpy(flat.copy()).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_out = torch.full_like(d_in, 7)
    revcomp_dev(len(seqs), d_in.data_ptr(), d_off.data_ptr(), d_out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    for i, s in enumerate(seqs):
        assert out[int(off[i]):int(off[i + 1])].tobytes() == dna.revcomp(s.tobytes()), i
    assert (d_in.cpu().numpy() == flat).all()
