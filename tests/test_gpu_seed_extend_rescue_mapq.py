"""Mate rescue with a mapping quality per mate (`bg_seed_extend_pairs_rescue_mapq_batch[_dev]`) against the CPU statement of the
rule (tests/rescueq_oracle.py): every field of every bg_multi_hit_t, every other output against the rescue call byte for byte,
the records of pairs that were not rescued against the pairs-mapq call, and the SAM lines that carry the result.

The case (`make_case`), on the rescue tests' genome (a 400 bp repeat at 10 000 and 50 000) with two more planted copies:
  A  fragments in unique sequence, mate 2 seed-broken                       -> anchor / no alternative, rescued / no alternative
  B  mate 1 inside the second repeat copy, seed-broken mate 2 beside it     -> anchor / seeded alternative (its rescue fails)
  C  fragments of exactly 400 bp on a repeat copy, mate 2 seed-broken       -> anchor / alternative with its own accepted rescue,
                                                                               rescued / alternative through that rescue (mapq 0)
  D  mate 2 an exact copy of text[80 000 .. 80 150), whose seed-broken copy lies beside mate 1 at 120 250
                                                                            -> rescued / seeded alternative, judged through (b)
  E  mate 1 exact at 90 000, 15 substitutions on its copy at 130 000 beside the seed-broken mate 2: the chosen anchor is rank 1 and
     scores 30 less than the far one, pen_unpaired is 25                    -> anchor / S2 > S1 (clamped)
  F  pairs with a proper seeded combination, G pairs with a random mate 2 (rescue alignments run, none accepted): rescued = 0.
`test_the_case_meets_every_class` counts the mates of each class from the oracle alone."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle_py as orc
import pair_oracle as po
import rescue_cases as rc
import rescueq_oracle as rq
from rescue_cases import L, MIN_SCORE, SC, flat_of, other_base, planted_pairs, seed_broken
from rust_bio_amd import _lib, sam, synth
from rust_bio_amd.alphabets import dna
from rust_bio_amd.pairwise import Scoring
from rust_bio_amd.pairwise import MIN_SCORE as BG_MIN_SCORE
from rust_bio_amd.pipeline import (PairParams, PairQualityParams, RescueParams, SeedParams, attach_text,
                                   seed_extend_pairs_rescue_mapq_arrays, seed_extend_pairs_rescue_mapq_dev)
from test_gpu_pipeline import ALPHA, build
from test_gpu_sam_emit import Batch, fastq_text, fields, split
from test_gpu_seed_extend_pairq import check_records, pairq_dev
from test_gpu_seed_extend_rescue import dev_call as rescue_dev_call
from test_gpu_seed_extend_rescue import nothing_case, stride_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID_ARG, TOO_LARGE, OPS_CAP = -1, -8, -9
PP = PairParams(0, 1000, 25)
RP = RescueParams(4, MIN_SCORE)
QPS = [(-2**31, 60), (60, 60), (100, 254), (-2**31, 0)]


def revcomp(x):
    return np.frombuffer(dna.revcomp(np.ascontiguousarray(x).tobytes()), np.uint8)


def make_case(ragged=False):
    """(genome, text, reads, offsets): see the module docstring.  `ragged` cuts the reads of group A to 12 .. 150 bases; the
    other groups keep their length, so the classes stay met."""
    g, _ = rc.genome()
    g[120_250:120_400] = seed_broken(g[80_000:80_150])  # D
    g[130_000:130_150] = g[90_000:90_150]               # E
    g[130_060:130_075] = other_base(g[130_060:130_075])
    text = np.append(g, np.uint8(ord("$")))
    rng = np.random.default_rng(41)
    seqs = []
    # A
    s = rng.integers(60_000, 78_000, size=24)
    a, _, _ = planted_pairs(g, s, np.full(24, 400), np.arange(24) % 2 == 1, (np.arange(24) // 2) % 2 == 1, seed=2)
    if ragged:
        lens = rng.integers(12, L + 1, size=48)
        lens[:8] = L
        a = [r[:lens[k]] for k, r in enumerate(a)]
    seqs += a
    # B
    seqs += planted_pairs(g, 50_150 + rng.integers(0, 101, size=8), np.full(8, 400), np.arange(8) % 2 == 1)[0]
    # C
    seqs += planted_pairs(g, np.array([10_000] * 4 + [50_000] * 4), np.full(8, 400), np.arange(8) % 2 == 1, np.arange(8) % 4 >= 2, seed=3)[0]
    # D
    for k in range(6):
        pair = [g[120_000 + 7 * k:120_150 + 7 * k].copy(), revcomp(g[80_000:80_150])]
        seqs += pair[::-1] if k % 2 else pair
    # E
    for k in range(6):
        pair = [g[90_000:90_150].copy(), revcomp(seed_broken(g[130_250 + k:130_400 + k]))]
        seqs += pair[::-1] if k % 2 else pair
    # F, G
    seqs += planted_pairs(g, rng.integers(140_000, 190_000, size=6), np.full(6, 400), np.arange(6) % 2 == 1, break_mate2=False)[0]
    lone = planted_pairs(g, rng.integers(140_000, 190_000, size=4), np.full(4, 400), np.zeros(4, bool))[0]
    for k in range(4):
        lone[2 * k + 1] = synth.random_dna(L, seed=70 + k).copy()
    seqs += lone
    flat, off = flat_of(seqs)
    return g, text, flat, off


@functools.lru_cache(maxsize=None)
def case(ragged=False):
    """the case, its index with a raw and a sampled suffix array, the candidates of its virtual reads and the rescue alignments
    (the oracle's)"""
    g, text, reads, off = make_case(ragged)
    sa, b, ls, fm_raw = build(text, 0)
    fm_sampled = build(text, 8)[3]
    for fm in (fm_raw, fm_sampled):
        attach_text(fm, text)
    vr, voff = po.virtual_reads(reads, off)
    sc = orc.make_scoring(*SC)
    cands, _ = po.candidates(orc, b, ls, orc.Occ(b, 64, ALPHA), sa, text, len(g), sc, vr, voff)
    n_pairs = (len(off) - 1) // 2
    aligned = rq.expected(orc, sc, cands, voff, vr, text, len(g), n_pairs, PP.min_span, PP.max_span, PP.pen_unpaired, RP.max_anchors,
                          RP.min_score)[3]
    return g, text, reads, off, (fm_raw, fm_sampled), (cands, voff, vr, aligned)


def expectation(c, qp):
    """(records, classes, rescued) of the case c under qp"""
    g, text, reads, off, _, (cands, voff, vr, aligned) = c
    recs, classes, rescued, _ = rq.expected(None, None, cands, voff, vr, text, len(g), (len(off) - 1) // 2, PP.min_span, PP.max_span,
                                            PP.pen_unpaired, RP.max_anchors, RP.min_score, qp.min_score, qp.mapq_cap, aligned)
    return recs, np.array(classes), rescued


def rq_dev(fm, reads, off, max_len, qp, pp=PP, rp=RP, prm=None, stream=None, strand=True, ops=True, totals=True, stride=None, null=()):
    """the device flavour into buffers filled with the pattern of the rescue tests' dev_call: (hits, strand, pairs, rescued, ops slots,
    stride, totals, multi, status).  `null` names the pointers to pass as null; an error status is returned, not raised."""
    prm = prm or SeedParams()
    R = len(off) - 1
    stride = stride_of(max_len, prm, pp) if stride is None else stride
    d_reads = torch.from_numpy(reads if len(reads) else np.zeros(16, np.uint8)).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.zeros(max(R, 1) * 96, dtype=torch.uint8, device=DEV)
    d_strand = torch.full((max(R, 1),), 77, dtype=torch.uint8, device=DEV)
    d_pairs = torch.full((max(R // 2, 1) * 16,), 0x55, dtype=torch.uint8, device=DEV)
    d_resc = torch.full((max(R // 2, 1),), 0x55, dtype=torch.uint8, device=DEV)
    d_multi = torch.full((max(R, 1) * 16,), 0xA5, dtype=torch.uint8, device=DEV)
    d_ops = torch.zeros(max(R, 1) * stride, dtype=torch.uint8, device=DEV)
    tot = np.full(4, 99, dtype=np.uint64)
    st = stream if stream is not None else torch.cuda.current_stream()
    status = 0
    with torch.cuda.stream(st):
        try:
            seed_extend_pairs_rescue_mapq_dev(fm, Scoring.from_scores(*SC), R // 2, d_reads.data_ptr(), d_off.data_ptr(), max_len,
                                              d_hits.data_ptr(), 0 if "pairs" in null else d_pairs.data_ptr(),
                                              0 if "rescued" in null else d_resc.data_ptr(), 0 if "multi" in null else d_multi.data_ptr(),
                                              d_strand.data_ptr() if strand else 0, d_ops.data_ptr() if ops else 0, stride if ops else 0,
                                              prm, pp, rp, qp, st.cuda_stream, tot if totals else None)
        except _lib.BiogpuError as e:
            status = e.status
    torch.cuda.synchronize()
    return (d_hits.cpu().numpy().view(_lib.SEED_HIT_DTYPE)[:R], d_strand.cpu().numpy()[:R],
            d_pairs.cpu().numpy().view(_lib.PAIR_HIT_DTYPE)[:R // 2], d_resc.cpu().numpy()[:R // 2], d_ops.cpu().numpy(), stride, tot,
            d_multi.cpu().numpy().view(_lib.MULTI_HIT_DTYPE)[:R], status)


def untouched(out, n_reads):
    """every buffer of rq_dev still holds its pattern"""
    hits, strand, pairs, resc, ops, _, tot, multi, _ = out
    return (not hits.view(np.uint8).any() and (strand == 77).all() and (pairs.view(np.uint8) == 0x55).all() and (resc == 0x55).all()
            and not ops.any() and (tot == 99).all() and (multi.view(np.uint8) == 0xA5).all())


def test_the_case_meets_every_class():
    """counted from the oracle alone, before anything of the library's is compared"""
    for ragged in (False, True):
        c = case(ragged)
        for qp in (PairQualityParams(), PairQualityParams(60, 60)):
            recs, classes, rescued = expectation(c, qp)
            counts = np.bincount(classes, minlength=13)
            print("ragged" if ragged else "fixed", "min_score", qp.min_score, dict(zip(rq.CLASS_NAMES, counts.tolist())))
            assert (counts[list(rq.RESCUED_CLASSES)] >= 5).all(), counts
            assert (rescued == 0).sum() >= 8 and (rescued == 1).sum() >= 10 and (rescued == 2).sum() >= 10
            in_rescued = np.repeat(rescued != 0, 2)
            mapq = np.array([r[3] for r in recs])[in_rescued]
            assert ((mapq > 0) & (mapq < qp.mapq_cap)).sum() >= 5 and (mapq == 0).sum() >= 5 and (mapq == qp.mapq_cap).sum() >= 5


@pytest.mark.parametrize("ragged,sampled", [(False, 0), (True, 1)])
@pytest.mark.parametrize("min_score,cap", QPS)
def test_records_match_the_oracle_and_the_rescue_call(ragged, sampled, min_score, cap):
    c = case(ragged)
    g, text, reads, off = c[:4]
    fm = c[4][sampled]
    qp = PairQualityParams(min_score, cap)
    recs, classes, rescued = expectation(c, qp)
    got = rq_dev(fm, reads, off, L, qp)
    assert got[8] == 0 and (got[3] == rescued).all()
    check_records(got[7], recs)
    # hits, strand, pairs, rescued, every operation byte and the four totals are the rescue call's
    want = rescue_dev_call(fm, reads, off, L, pp=PP, rp=RP)
    assert want[5] == got[5]
    for k, (a, b_) in enumerate(zip(got[:7], want)):
        assert np.asarray(a).tobytes() == np.asarray(b_).tobytes(), k
    # the records of the pairs that were not rescued are the pairs-mapq call's
    single = np.repeat(got[3] == 0, 2)
    assert single.sum() >= 16
    pq = pairq_dev(fm, reads, off, L, qp, pp=PP)[6]
    assert got[7][single].tobytes() == pq[single].tobytes()
    assert (classes[single] < 6).all() and (classes[~single] >= 6).all()
    # the host flavour: the same records and bytes, the hits with compacted operations
    hh, hs, hp, hr, hm, hops = seed_extend_pairs_rescue_mapq_arrays(fm, Scoring.from_scores(*SC), reads, off, pair_params=PP,
                                                                    rescue_params=RP, quality_params=qp)
    assert hm.tobytes() == got[7].tobytes() and hp.tobytes() == got[2].tobytes() and (hs == got[1]).all() and (hr == got[3]).all()
    a, b_ = hh.copy(), got[0].copy()
    a["aln"]["ops_off"] = b_["aln"]["ops_off"] = 0
    assert a.tobytes() == b_.tobytes()
    n_ops = hh["aln"]["n_ops"].astype(np.int64)
    assert (hh["aln"]["ops_off"] == np.cumsum(n_ops) - n_ops).all() and len(hops) == int(n_ops.sum())
    for r in range(len(hh)):
        o, k, do = int(hh["aln"]["ops_off"][r]), int(n_ops[r]), int(got[0]["aln"]["ops_off"][r])
        assert (hops[o:o + k] == got[4][do:do + k]).all(), r


def test_what_the_rule_gives():
    """the planted groups, on the device's records: B costs the anchor's mate pen_unpaired, C gives both mates 0, D is judged through
    (b), E is clamped to 0; the rescued mates of A, B and E get the cap"""
    c = case()
    g, text, reads, off = c[:4]
    got = rq_dev(c[4][0], reads, off, L, PairQualityParams(-2**31, 60))
    multi, resc = got[7].reshape(-1, 2), got[3]
    assert (resc[:52] != 0).all() and (resc[52:] == 0).all()
    anchor = multi[np.arange(52), 2 - resc[:52].astype(int)]
    rescued = multi[np.arange(52), resc[:52].astype(int) - 1]
    assert (anchor["mapq"][:24] == 60).all() and (rescued["mapq"][:24] == 60).all() and (anchor["n_loci"][:24] == 1).all()
    assert (anchor["mapq"][24:32] == 60 * 25 // 150).all() and (anchor["sub_score"][24:32] == 150).all() and (rescued["mapq"][24:32] == 60).all()
    assert (anchor["mapq"][32:40] == 0).all() and (rescued["mapq"][32:40] == 0).all() and (rescued["n_loci"][32:40] == 2).all()
    assert (anchor["mapq"][40:46] == 60).all() and (rescued["sub_score"][40:46] == 150).all() and (rescued["mapq"][40:46] == 60 * 5 // 130).all()
    assert (anchor["mapq"][46:52] == 0).all() and (anchor["sub_score"][46:52] == 150).all() and (rescued["mapq"][46:52] == 60).all()


def test_nothing_to_rescue():
    """a pass that ends after R1's read-back has its records already: the pairs-mapq call's buffer whole"""
    g, text, reads, off, n_pairs = nothing_case()
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    pp, rp, qp = PairParams(0, 1000, 17), RescueParams(2, MIN_SCORE), PairQualityParams(40, 60)
    got = rq_dev(fm, reads, off, L, qp, pp=pp, rp=rp)
    assert got[8] == 0 and (got[3] == 0).all() and got[6][2] > 0 and got[6][3] == 0
    pq = pairq_dev(fm, reads, off, L, qp, pp=pp)
    assert got[7].tobytes() == pq[6].tobytes() and got[2].tobytes() == pq[2].tobytes()
    # pairs with a proper seeded combination alone: no rescue alignment in the whole call
    keep = np.nonzero(got[2]["n_proper"] > 0)[0][:64]
    seqs = []
    for p in keep:
        seqs += [reads[int(off[2 * p]):int(off[2 * p + 1])], reads[int(off[2 * p + 1]):int(off[2 * p + 2])]]
    sub, sub_off = flat_of(seqs)
    got = rq_dev(fm, sub, sub_off, L, qp, pp=pp, rp=rp)
    assert got[8] == 0 and got[6][2] == 0 and (got[3] == 0).all()
    assert got[7].tobytes() == pairq_dev(fm, sub, sub_off, L, qp, pp=pp)[6].tobytes()
    fm.close()


@pytest.mark.parametrize("chunk", [2, 6, 7, 0])
def test_passes_streams_and_optional_outputs(chunk):
    c = case(True)
    g, text, reads, off = c[:4]
    fm = c[4][1]
    qp = PairQualityParams(60, 60)
    recs, _, rescued = expectation(c, qp)
    want = rq_dev(fm, reads, off, L, qp)
    check_records(want[7], recs)
    fm.ctx.set_option("seed_chunk_reads", chunk)
    try:
        got = rq_dev(fm, reads, off, L, qp)
        got2 = rq_dev(fm, reads, off, L, qp, stream=torch.cuda.Stream())
        bare = rq_dev(fm, reads, off, L, qp, strand=False, ops=False, totals=False)
        none = rq_dev(fm, reads[:0], off[:1], L, qp)
    finally:
        fm.ctx.set_option("seed_chunk_reads", 0)
    for k, (a, b_, c_) in enumerate(zip(got[:8], want, got2)):
        assert np.asarray(a).tobytes() == np.asarray(b_).tobytes() == np.asarray(c_).tobytes(), k
    # strand, operations and totals are optional; the records are the same
    assert bare[8] == 0 and bare[7].tobytes() == want[7].tobytes() and bare[2].tobytes() == want[2].tobytes() and (bare[3] == want[3]).all()
    assert (bare[1] == 77).all() and not bare[4].any() and (bare[6] == 99).all()
    # no pairs: totals are zeroed, nothing else is written
    assert none[8] == 0 and [int(t) for t in none[6]] == [0, 0, 0, 0]


def test_arguments():
    c = case()
    g, text, reads, off = c[:4]
    fm = c[4][1]
    n = len(off) - 1
    qp = PairQualityParams()
    need = stride_of(L, SeedParams(), PP)
    for kw, status in ((dict(null=("multi",)), INVALID_ARG), (dict(null=("rescued",)), INVALID_ARG), (dict(null=("pairs",)), INVALID_ARG),
                       (dict(qp=PairQualityParams(0, 255)), INVALID_ARG), (dict(rp=RescueParams(0, 0)), INVALID_ARG),
                       (dict(rp=RescueParams(5, 0)), INVALID_ARG), (dict(pp=PairParams(501, 500, 0)), INVALID_ARG),
                       (dict(pp=PairParams(0, 65536, 25)), TOO_LARGE), (dict(stride=need - 1), OPS_CAP)):
        out = rq_dev(fm, reads, off, L, **{"qp": qp, **kw})
        assert out[8] == status, kw
        assert untouched(out, n), kw
    assert rq_dev(fm, reads, off, L, PairQualityParams(0, 254), stride=need)[8] == 0
    assert rq_dev(fm, reads, off, L, qp, rp=RescueParams(_lib.RESCUE_MAX_ANCHORS, 0))[8] == 0
    # null parameter structs, through the C ABI; the host flavour's own checks
    lib = _lib.lib()
    sc = Scoring.from_scores(*SC)
    c_sc, pc, pp, rp, cq = sc.to_c(), SeedParams().to_c(), PP.to_c(), RP.to_c(), qp.to_c()
    hits = np.zeros(n, dtype=_lib.SEED_HIT_DTYPE)
    pairs = np.full(n // 2 * 16, 0x55, np.uint8)
    resc = np.full(n // 2, 0x55, np.uint8)
    multi = np.full(n * 16, 0xA5, np.uint8)
    used = C.c_uint64(0)

    def host(rp_ref, qp_ref, hits_p=hits.ctypes.data, pairs_p=pairs.ctypes.data, resc_p=resc.ctypes.data, multi_p=multi.ctypes.data,
             n_pairs=n // 2):
        return lib.bg_seed_extend_pairs_rescue_mapq_batch(fm.h, C.byref(c_sc), C.byref(pc), C.byref(pp), rp_ref, qp_ref, n_pairs,
                                                          reads.ctypes.data, off.ctypes.data, hits_p, None, pairs_p, resc_p, multi_p, None, 0,
                                                          C.byref(used))
    assert host(None, C.byref(cq)) == INVALID_ARG
    assert host(C.byref(rp), None) == INVALID_ARG
    assert host(C.byref(rp), C.byref(cq), multi_p=None) == INVALID_ARG
    assert host(C.byref(rp), C.byref(cq), resc_p=None) == INVALID_ARG
    assert host(C.byref(rp), C.byref(cq), pairs_p=None) == INVALID_ARG
    assert host(C.byref(rp), C.byref(cq), hits_p=None) == INVALID_ARG
    assert host(C.byref(rp), C.byref(cq), multi_p=None, n_pairs=0) == INVALID_ARG
    assert host(C.byref(rp), C.byref(cq), hits_p=None, n_pairs=0) == 0
    assert not hits.view(np.uint8).any() and (pairs == 0x55).all() and (resc == 0x55).all() and (multi == 0xA5).all()
    d_reads = torch.from_numpy(reads).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.zeros(n * 96, dtype=torch.uint8, device=DEV)
    d_pairs = torch.zeros(n * 8, dtype=torch.uint8, device=DEV)
    d_resc = torch.zeros(n // 2, dtype=torch.uint8, device=DEV)
    d_multi = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)

    def dev(rp_ref, qp_ref):
        return lib.bg_seed_extend_pairs_rescue_mapq_batch_dev(fm.h, C.byref(c_sc), C.byref(pc), C.byref(pp), rp_ref, qp_ref, n // 2,
                                                              d_reads.data_ptr(), d_off.data_ptr(), L, d_hits.data_ptr(), None,
                                                              d_pairs.data_ptr(), d_resc.data_ptr(), d_multi.data_ptr(), None, 0, None, None)
    assert dev(None, C.byref(cq)) == INVALID_ARG
    assert dev(C.byref(rp), None) == INVALID_ARG
    torch.cuda.synchronize()
    assert not d_multi.any() and not d_hits.any()
    assert dev(C.byref(rp), C.byref(cq)) == 0
    torch.cuda.synchronize()
    with pytest.raises(_lib.BiogpuError) as e:
        seed_extend_pairs_rescue_mapq_arrays(fm, sc, reads, off, pair_params=PairParams(0, 65536, 25))
    assert e.value.status == TOO_LARGE
    with pytest.raises(_lib.BiogpuError) as e:
        seed_extend_pairs_rescue_mapq_arrays(fm, sc, reads, off, quality_params=PairQualityParams(0, 255))
    assert e.value.status == INVALID_ARG


def test_sam_lines_of_rescued_pairs_carry_the_records():
    """bg_sam_emit_batch_dev with BG_SAM_PAIRED and the new records as its multi argument, against tests/sam_oracle.py fed with
    the oracle's records; the same lines after the rescue call alone say 255"""
    c = case()
    g, text, reads, off = c[:4]
    fm = c[4][1]
    seqs = split(reads, off)
    n = len(seqs)
    B = Batch(fm, [(b"chr1", 0, len(g))], text, fastq_text(seqs, [b"frag%d/%d" % (r // 2, r % 2 + 1) for r in range(n)], seed=2), n)
    cap = 60
    qp = PairQualityParams(-2**31, cap)
    recs, _, rescued = expectation(c, qp)
    stride = stride_of(L, SeedParams(), PP)
    d_hits = torch.zeros(n * 96, dtype=torch.uint8, device=DEV)
    d_strand = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
    d_ops = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
    d_pairs = torch.zeros(n // 2 * 16, dtype=torch.uint8, device=DEV)
    d_resc = torch.zeros(n // 2, dtype=torch.uint8, device=DEV)
    d_multi = torch.full((n * 16,), 0xA5, dtype=torch.uint8, device=DEV)
    seed_extend_pairs_rescue_mapq_dev(fm, Scoring.from_scores(*SC), n // 2, B.d_seq.data_ptr(), B.d_seq_off.data_ptr(), B.max_len,
                                      d_hits.data_ptr(), d_pairs.data_ptr(), d_resc.data_ptr(), d_multi.data_ptr(), d_strand.data_ptr(),
                                      d_ops.data_ptr(), stride, pair_params=PP, rescue_params=RP, quality_params=qp,
                                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (d_resc.cpu().numpy() == rescued).all()
    want_multi = np.zeros(n, dtype=_lib.MULTI_HIT_DTYPE)
    for r, (sub, n_loci, n_rep, mapq) in enumerate(recs):
        want_multi[r]["sub_score"], want_multi[r]["n_loci"], want_multi[r]["n_reported"], want_multi[r]["mapq"] = sub, n_loci, n_rep, mapq
    flags = sam.SAM_PAIRED | sam.SAM_TAG_NM | sam.SAM_TAG_MD
    out, o = B.emit_dev(flags, 1, d_hits, d_strand, d_ops, d_multi=d_multi, d_pairs=d_pairs)
    lines = B.oracle(flags, 1, d_hits.cpu().numpy().view(_lib.SEED_HIT_DTYPE), d_strand.cpu().numpy(), d_ops.cpu().numpy(), want_multi,
                     d_pairs.cpu().numpy().view(_lib.PAIR_HIT_DTYPE))
    B.same(lines, (out, o))
    plain, po_ = B.emit_dev(flags, 1, d_hits, d_strand, d_ops, d_pairs=d_pairs)  # what the rescue call alone leads to
    between = xs = 0
    for p in np.nonzero(rescued)[0]:
        for r in (2 * p, 2 * p + 1):
            f, f0 = fields(out[int(o[r]):int(o[r + 1])]), fields(plain[int(po_[r]):int(po_[r + 1])])
            assert int(f[1]) & 0x2 and not int(f[1]) & 0x4, r
            assert int(f[4]) == recs[r][3] and f0[4] == b"255", r
            between += 0 < int(f[4]) < cap
            has_xs = [t for t in f[11:] if t.startswith(b"XS:i:")]
            if recs[r][0] != BG_MIN_SCORE:
                assert has_xs == [b"XS:i:%d" % recs[r][0]], r
                xs += 1
            else:
                assert not has_xs, r
            assert not [t for t in f0[11:] if t.startswith(b"XS:i:")], r
    assert between >= 5 and xs >= 20
