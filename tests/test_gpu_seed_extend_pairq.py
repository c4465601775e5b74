"""A mapping quality for each mate of a read pair (`bg_seed_extend_pairs_mapq_batch[_dev]`) against the CPU statement of the
rule (tests/pairq_oracle.py) on the candidates of tests/pair_oracle.py: every field of every bg_multi_hit_t, the paired call's
outputs byte for byte, the multi call's records where the pair is not proper, and the SAM lines that carry the result.

The case (`make_case`): the pairs generator's genome with its far repeat (400 bases at 10 000 copied to 50 000) and a near repeat
(the 150 bases at 120 000 copied to 120 300, inside max_span of a partner), 440 pairs drawn anywhere, 20 pairs with a mate on a
copy of the near repeat, 20 with a mate inside a copy of the far repeat, 10 more of those made chimeric (mate 2 of another
pair) and 10 whose mate 2 is unmappable, half of them with mate 1 on the near repeat.  `test_the_case_meets_every_class` counts,
from the oracle alone, the mates of each class of pairq_oracle.CLASS_NAMES and asserts at least 5 in each."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import pairq_oracle as qo
from rust_bio_amd import _lib, sam, synth
from rust_bio_amd.pairwise import MIN_SCORE, Scoring
from rust_bio_amd.pipeline import (MultiParams, PairParams, PairQualityParams, SeedParams, attach_text, seed_extend_multi_dev,
                                   seed_extend_pairs_mapq_arrays, seed_extend_pairs_mapq_dev)
from test_gpu_pipeline import build
from test_gpu_sam_emit import Batch, cut, fastq_text, fields, split, tag
from test_gpu_seed_extend_pairs import SC, dev_call, flat_of, mates_at, oracle_pairs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID_ARG = -1
L = 150
PP = PairParams(0, 1000, 17)
N_PAIRS = 500


def make_case(ragged=False):
    """(genome, text, reads, offsets): see the module docstring.  `ragged` shortens the 440 pairs drawn anywhere (not the first
    100 reads) to 15 .. 150 bases; the planted pairs keep their length, so the classes stay met."""
    g = synth.random_dna(200_000, seed=31).copy()
    g[50_000:50_400] = g[10_000:10_400]
    g[120_300:120_450] = g[120_000:120_150]
    text = np.append(g, np.uint8(ord("$")))
    rng = np.random.default_rng(17)
    bulk, _, _ = synth.read_pairs(text, 440, L, seed=12, sub=0.04, ins=0.005, dele=0.005)
    # a mate on a copy of the near repeat: the reverse mate on the first copy (its partner 250 before it), or the forward mate on
    # the second copy (its partner 250 behind it); either way both copies lie inside max_span of the partner
    s_near = np.concatenate([120_000 + rng.integers(0, 8, size=10) - 250, 120_300 + rng.integers(0, 8, size=10)])
    near, _, _ = mates_at(g, s_near, np.full(20, 400), L, 95, np.zeros(20, bool))
    # mate 1 inside a copy of the far repeat, mate 2 behind it in unique sequence
    s_far = np.concatenate([10_000 + rng.integers(150, 250, size=15), 50_000 + rng.integers(150, 250, size=15)])
    far, _, _ = mates_at(g, s_far, np.full(30, 400), L, 96, np.zeros(30, bool))
    # pairs that lose mate 2: mate 1 in unique sequence, or on the second copy of the near repeat
    s_lone = np.concatenate([150_000 + 1_000 * np.arange(5), 120_300 + rng.integers(0, 8, size=5)])
    lone, _, _ = mates_at(g, s_lone, np.full(10, 400), L, 97, np.zeros(10, bool))
    R = np.concatenate([bulk.reshape(-1, L), near, far, lone]).copy()
    assert len(R) == 2 * N_PAIRS
    R[2 * np.arange(N_PAIRS - 10, N_PAIRS) + 1] = synth.random_dna(10 * L, seed=5).reshape(10, L)  # unmappable mate 2
    R[2 * np.arange(N_PAIRS - 20, N_PAIRS - 10) + 1] = R[2 * np.arange(0, 10) + 1]                # chimeric: mate 2 of another pair
    seqs = list(R)
    if ragged:
        lens = rng.integers(15, L + 1, size=2 * N_PAIRS)
        lens[:100] = L
        lens[880:] = L
        seqs = [R[r, :lens[r]] for r in range(2 * N_PAIRS)]
    flat, off = flat_of(seqs)
    return g, text, flat, off


@functools.lru_cache(maxsize=None)
def case(ragged=False, sampled=8):
    """the case, its index and the candidates of its virtual reads (the oracle's)"""
    g, text, reads, off = make_case(ragged)
    sa, b, ls, fm = build(text, sampled)
    attach_text(fm, text)
    _, _, cands = oracle_pairs(b, ls, sa, text, len(g), reads, off, PP)
    return g, text, reads, off, fm, cands


def expectation(cands, n_pairs, qp, pp=PP):
    recs, classes = qo.expected(cands, None, n_pairs, pp.min_span, pp.max_span, pp.pen_unpaired, qp.min_score, qp.mapq_cap)
    return recs, np.array(classes)


def check_records(multi, recs):
    """every field of every record against the oracle"""
    assert len(multi) == len(recs)
    for r, (sub, n_loci, n_rep, mapq) in enumerate(recs):
        m = multi[r]
        assert (int(m["sub_score"]), int(m["n_loci"]), int(m["n_reported"]), int(m["mapq"])) == (sub, n_loci, n_rep, mapq), r
    assert (multi["reserved"] == 0).all()


def pairq_dev(fm, reads, off, max_len, qp, pp=PP, prm=None, stream=None, strand=True, ops=True):
    """the device flavour into buffers filled with a pattern: (hits, strand, pairs, ops slots, stride, totals, multi)"""
    prm = prm or SeedParams()
    R = len(off) - 1
    stride = 2 * max_len + 2 * prm.pad + 4
    d_reads = torch.from_numpy(reads).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    # (hits and operation slots start as dev_call's do: the comparison with the paired call is over whole buffers)
    d_hits = torch.zeros(max(R, 1) * 96, dtype=torch.uint8, device=DEV)
    d_strand = torch.full((max(R, 1),), 77, dtype=torch.uint8, device=DEV)
    d_pairs = torch.full((max(R // 2, 1) * 16,), 0x55, dtype=torch.uint8, device=DEV)
    d_multi = torch.full((max(R, 1) * 16,), 0xA5, dtype=torch.uint8, device=DEV)
    d_ops = torch.zeros(max(R, 1) * stride, dtype=torch.uint8, device=DEV)
    tot = np.zeros(2, dtype=np.uint64)
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        seed_extend_pairs_mapq_dev(fm, Scoring.from_scores(*SC), R // 2, d_reads.data_ptr(), d_off.data_ptr(), max_len, d_hits.data_ptr(),
                                   d_pairs.data_ptr(), d_multi.data_ptr(), d_strand.data_ptr() if strand else 0,
                                   d_ops.data_ptr() if ops else 0, stride if ops else 0, prm, pp, qp, st.cuda_stream, tot)
    torch.cuda.synchronize()
    return (d_hits.cpu().numpy().view(_lib.SEED_HIT_DTYPE)[:R], d_strand.cpu().numpy()[:R],
            d_pairs.cpu().numpy().view(_lib.PAIR_HIT_DTYPE)[:R // 2], d_ops.cpu().numpy(), stride, tot,
            d_multi.cpu().numpy().view(_lib.MULTI_HIT_DTYPE)[:R])


def multi_k1_dev(fm, reads, off, max_len, qp):
    """bg_seed_extend_multi_batch_dev at K = 1 on both strands: the records"""
    R = len(off) - 1
    d_reads = torch.from_numpy(reads).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.zeros(R * 96, dtype=torch.uint8, device=DEV)
    d_multi = torch.full((R * 16,), 0x5A, dtype=torch.uint8, device=DEV)
    seed_extend_multi_dev(fm, Scoring.from_scores(*SC), R, d_reads.data_ptr(), d_off.data_ptr(), max_len, d_hits.data_ptr(),
                          d_multi.data_ptr(), multi_params=MultiParams(1, qp.min_score, qp.mapq_cap), strands=_lib.STRAND_BOTH,
                          stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_multi.cpu().numpy().view(_lib.MULTI_HIT_DTYPE)


def test_the_case_meets_every_class():
    """counted from the oracle alone, before anything of the library's is compared"""
    for ragged in (False, True):
        g, text, reads, off, fm, cands = case(ragged)
        for qp in (PairQualityParams(), PairQualityParams(60, 60)):
            recs, classes = expectation(cands, N_PAIRS, qp)
            counts = np.bincount(classes, minlength=6)
            print("ragged" if ragged else "fixed", "min_score", qp.min_score, dict(zip(qo.CLASS_NAMES, counts.tolist())))
            assert (counts >= 5).all(), counts
            mapq = np.array([r[3] for r in recs])
            assert ((mapq > 0) & (mapq < qp.mapq_cap)).sum() >= 5 and (mapq == 0).sum() >= 5 and (mapq == qp.mapq_cap).sum() >= 5


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("min_score,cap", [(-2**31, 60), (60, 60), (100, 254), (-2**31, 0)])
def test_records_match_the_oracle_and_the_paired_call(ragged, min_score, cap):
    g, text, reads, off, fm, cands = case(ragged)
    qp = PairQualityParams(min_score, cap)
    recs, classes = expectation(cands, N_PAIRS, qp)
    got = pairq_dev(fm, reads, off, L, qp)
    check_records(got[6], recs)
    # hits, strand, pairs, every operation byte and the totals are the paired call's
    want = dev_call(fm, reads, off, L, pp=PP)
    for a, b_ in zip(got[:6], want):
        assert np.asarray(a).tobytes() == np.asarray(b_).tobytes()
    # the records of pairs that are not proper are the multi call's at K = 1 on both strands
    single = np.repeat(got[2]["proper"] == 0, 2)
    assert single.sum() >= 40
    m1 = multi_k1_dev(fm, reads, off, L, qp)
    assert got[6][single].tobytes() == m1[single].tobytes()
    assert (np.isin(classes[single], (qo.SINGLE_RUNNER_UP, qo.SINGLE_UNIQUE, qo.NO_CANDIDATES))).all()
    # the host flavour: the same records, the paired call's hits with compacted operations
    hh, hs, hp, hm, hops = seed_extend_pairs_mapq_arrays(fm, Scoring.from_scores(*SC), reads, off, pair_params=PP, quality_params=qp)
    assert hm.tobytes() == got[6].tobytes() and hp.tobytes() == got[2].tobytes() and (hs == got[1]).all()
    for f in ("window_start", "ref_start", "ref_end", "n_candidates", "n_seed_hits"):
        assert (hh[f] == got[0][f]).all(), f
    assert (hh["aln"]["score"] == got[0]["aln"]["score"]).all()
    n_ops = hh["aln"]["n_ops"].astype(np.int64)
    assert (hh["aln"]["ops_off"] == np.cumsum(n_ops) - n_ops).all() and len(hops) == int(n_ops.sum())
    for r in range(0, len(hh), 7):
        o, k, do = int(hh["aln"]["ops_off"][r]), int(n_ops[r]), int(got[0]["aln"]["ops_off"][r])
        assert (hops[o:o + k] == got[3][do:do + k]).all(), r


def test_a_unique_partner_settles_a_repeat_mate():
    """what the call is for: a mate on the near repeat gets MAPQ 0 (both copies pair with the partner), a mate in the far repeat a
    MAPQ of about cap * pen_unpaired / score next to its unique partner, and the same read mapped alone gets 0"""
    g, text, reads, off, fm, cands = case()
    qp = PairQualityParams(-2**31, 60)
    got = pairq_dev(fm, reads, off, L, qp)
    multi, pairs = got[6], got[2]
    near = multi[880:920].reshape(20, 2)
    rep = np.concatenate([near[:10, 1], near[10:, 0]])  # the mate on a copy: the reverse mate of the first 10, the forward one after
    # (a read starts up to 7 bases into its copy, so its last bases differ at the other copy: a few points of score)
    assert (pairs["proper"][440:460] == 1).mean() >= 0.9 and ((rep["n_loci"] == 2) & (rep["mapq"] <= 10)).mean() >= 0.9
    far = multi[920:960:2]
    assert (far["n_loci"] == 2).mean() > 0.9
    two = far["n_loci"] == 2
    assert ((far["mapq"][two] > 0) & (far["mapq"][two] < 20)).mean() > 0.9
    alone = multi_k1_dev(fm, reads, off, L, qp)[920:960:2]
    assert (alone["mapq"][two] <= 5).mean() > 0.9
    partner = multi[921:960:2]
    assert (partner["mapq"] == 60).mean() > 0.9


@pytest.mark.parametrize("chunk", [2, 14, 0])
def test_passes_streams_and_none_at_all(chunk):
    g, text, reads, off, fm, cands = case(True)
    n = 2 * 130
    sub_reads, sub_off = reads[int(off[740]):int(off[740 + n])].copy(), (off[740:740 + n + 1] - off[740]).astype(np.uint64)
    qp = PairQualityParams(40, 60)
    recs, _ = expectation(cands[2 * 740:2 * (740 + n)], n // 2, qp)
    want = pairq_dev(fm, sub_reads, sub_off, L, qp)
    check_records(want[6], recs)
    fm.ctx.set_option("seed_chunk_reads", chunk)
    try:
        got = pairq_dev(fm, sub_reads, sub_off, L, qp)
        side = torch.cuda.Stream()
        got2 = pairq_dev(fm, sub_reads, sub_off, L, qp, stream=side)
    finally:
        fm.ctx.set_option("seed_chunk_reads", 0)
    for a, b_, c_ in zip(got, want, got2):
        assert np.asarray(a).tobytes() == np.asarray(b_).tobytes() == np.asarray(c_).tobytes()
    # strand and operations are optional; the records are the same
    bare = pairq_dev(fm, sub_reads, sub_off, L, qp, strand=False, ops=False)
    assert bare[6].tobytes() == want[6].tobytes() and bare[2].tobytes() == want[2].tobytes()
    # no pairs: nothing is written, totals are zeroed
    none = pairq_dev(fm, sub_reads[:0], sub_off[:1], L, qp)
    assert (none[5] == 0).all()


def test_arguments():
    g, text, reads, off, fm, cands = case()
    sc = Scoring.from_scores(*SC)
    with pytest.raises(_lib.BiogpuError) as e:
        seed_extend_pairs_mapq_arrays(fm, sc, reads, off, quality_params=PairQualityParams(0, 255))
    assert e.value.status == INVALID_ARG
    with pytest.raises(_lib.BiogpuError) as e:
        pairq_dev(fm, reads, off, L, PairQualityParams(0, 255))
    assert e.value.status == INVALID_ARG
    pairq_dev(fm, reads[:int(off[20])], off[:21], L, PairQualityParams(0, 254))
    for bad in (PairParams(501, 500, 0), PairParams(0, 500, -1)):  # the paired call's own checks stay
        with pytest.raises(_lib.BiogpuError) as e:
            pairq_dev(fm, reads, off, L, PairQualityParams(), pp=bad)
        assert e.value.status == INVALID_ARG
    lib = _lib.lib()
    c_sc, pc, pp, qp = sc.to_c(), SeedParams().to_c(), PP.to_c(), PairQualityParams().to_c()
    n = len(off) - 1
    hits = np.zeros(n, dtype=_lib.SEED_HIT_DTYPE)
    pairs = np.zeros(n // 2, dtype=_lib.PAIR_HIT_DTYPE)
    multi = np.zeros(n, dtype=_lib.MULTI_HIT_DTYPE)
    used = C.c_uint64(0)

    def host(qp_ref, multi_ptr, pairs_ptr=pairs.ctypes.data, n_pairs=n // 2):
        return lib.bg_seed_extend_pairs_mapq_batch(fm.h, C.byref(c_sc), C.byref(pc), C.byref(pp), qp_ref, n_pairs, reads.ctypes.data,
                                                   off.ctypes.data, hits.ctypes.data, None, pairs_ptr, multi_ptr, None, 0, C.byref(used))
    assert host(None, multi.ctypes.data) == INVALID_ARG   # no parameters
    assert host(C.byref(qp), None) == INVALID_ARG         # no records
    assert host(C.byref(qp), multi.ctypes.data, pairs_ptr=None) == INVALID_ARG
    assert host(C.byref(qp), None, n_pairs=0) == INVALID_ARG
    assert host(C.byref(qp), multi.ctypes.data, n_pairs=0) == 0
    d_reads = torch.from_numpy(reads).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.zeros(n * 96, dtype=torch.uint8, device=DEV)
    d_pairs = torch.zeros(n * 8, dtype=torch.uint8, device=DEV)
    d_multi = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)

    def dev(qp_ref, multi_ptr):
        return lib.bg_seed_extend_pairs_mapq_batch_dev(fm.h, C.byref(c_sc), C.byref(pc), C.byref(pp), qp_ref, n // 2, d_reads.data_ptr(),
                                                       d_off.data_ptr(), L, d_hits.data_ptr(), None, d_pairs.data_ptr(), multi_ptr, None, 0,
                                                       None, None)
    assert dev(None, d_multi.data_ptr()) == INVALID_ARG
    assert dev(C.byref(qp), None) == INVALID_ARG
    assert dev(C.byref(qp), d_multi.data_ptr()) == 0
    torch.cuda.synchronize()


def test_sam_lines_carry_the_records():
    """bg_sam_emit_batch_dev with BG_SAM_PAIRED and the new records as its multi argument"""
    g, _, reads, off = make_case()
    text, entries = cut(g, (70_000, 140_000))
    seqs = split(reads, off)
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    B = Batch(fm, entries, text, fastq_text(seqs, [b"frag%d/%d" % (r // 2, r % 2 + 1) for r in range(len(seqs))], seed=2), len(seqs))
    cap = 60
    qp = PairQualityParams(-2**31, cap)
    d_hits, d_strand, d_ops, stride = B.device_slots(1)
    d_pairs = torch.zeros(B.n // 2 * 16, dtype=torch.uint8, device=DEV)
    d_multi = torch.full((B.n * 16,), 0xA5, dtype=torch.uint8, device=DEV)
    seed_extend_pairs_mapq_dev(fm, Scoring.from_scores(*SC), B.n // 2, B.d_seq.data_ptr(), B.d_seq_off.data_ptr(), B.max_len,
                               d_hits.data_ptr(), d_pairs.data_ptr(), d_multi.data_ptr(), d_strand.data_ptr(), d_ops.data_ptr(), stride,
                               pair_params=PP, quality_params=qp, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    multi = d_multi.cpu().numpy().view(_lib.MULTI_HIT_DTYPE)
    flags = sam.SAM_PAIRED | sam.SAM_TAG_NM | sam.SAM_TAG_MD
    out, o = B.emit_dev(flags, 1, d_hits, d_strand, d_ops, d_multi=d_multi, d_pairs=d_pairs)
    plain, po_ = B.emit_dev(flags, 1, d_hits, d_strand, d_ops, d_pairs=d_pairs)
    between = xs = 0
    for r in range(B.n):
        f, f0 = fields(out[int(o[r]):int(o[r + 1])]), fields(plain[int(po_[r]):int(po_[r + 1])])
        placed = not int(f[1]) & 0x4
        assert int(f[4]) == (int(multi["mapq"][r]) if placed else 0), r
        assert f0[4] == (b"255" if placed else b"0"), r
        between += 0 < int(f[4]) < cap
        has_xs = [t for t in f[11:] if t.startswith(b"XS:i:")]
        if placed and int(multi["sub_score"][r]) != MIN_SCORE:
            assert has_xs == [b"XS:i:%d" % int(multi["sub_score"][r])], r
            xs += 1
        else:
            assert not has_xs, r
        assert f[:4] + f[5:11] + [t for t in f[11:] if not t.startswith(b"XS:i:")] == f0[:4] + f0[5:], r
    print("SAM case: lines with 0 < MAPQ < cap:", between, "with XS:", xs)
    assert between >= 1 and xs >= 5
    assert tag(out[int(o[0]):int(o[1])], b"AS:i:") is not None
    fm.close()
