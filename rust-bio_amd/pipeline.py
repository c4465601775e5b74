"""Seed-and-extend read mapping (BASELINE configs[4]) — host mirror of `bg_seed_extend_batch[_dev]`.

The reference has no such function; callers compose it from `FMIndex::backward_search`, `Interval::occ` and
`Aligner::semiglobal` (/root/reference/src/lib.rs:129-165, benches/fmindex.rs:20-38).  The composition — which
seeds vote, hit -> proposed read start, per-read dedup, window gather, best-hit reduction, the winners'
operations — runs in HIP kernels behind the C ABI (rust-bio_amd/csrc/seed_extend.hip); its definition is in
include/biogpu.h (the tests hold a CPU statement of it).  The `_strands` calls map each read on the forward strand, on
the reverse strand (its `dna::revcomp`), or on both, and say which strand won.  The `_pairs` calls map interleaved mates of
paired-end reads and report the best proper FR pair where there is one; the `_pairs_rescue` calls also look for a mate without a
seeded candidate inside its partner's insert window; the `_pairs_mapq` calls add a MAPQ per mate, judged against the pair.  The
`_multi` calls report up to K loci per read that
do not touch, the runner-up's score and a MAPQ.  This module only marshals arguments."""
import ctypes as C

import numpy as np

from . import _lib
from .pairwise import MIN_SCORE  # noqa: F401  (score of an unmapped read)


class SeedParams:
    def __init__(self, seed_len=20, stride=10, max_occ=16, pad=25):
        self.seed_len, self.stride, self.max_occ, self.pad = seed_len, stride, max_occ, pad

    def to_c(self):
        return _lib.SeedParamsC(self.seed_len, self.stride, self.max_occ, self.pad)


class PairParams:
    """bg_pair_params_t: a proper pair's span (SAM |TLEN|) lies in min_span ..= max_span; it may give up pen_unpaired (>= 0)
    of score against the two mates' own bests."""

    def __init__(self, min_span=0, max_span=1000, pen_unpaired=17):
        self.min_span, self.max_span, self.pen_unpaired = min_span, max_span, pen_unpaired

    def to_c(self):
        return _lib.PAIR_PARAMS(self.min_span, self.max_span, self.pen_unpaired)


class RescueParams:
    """bg_rescue_params_t: max_anchors (A, 1 ..= 4) candidates of a mate, best first, in whose insert windows the other mate is
    sought; a rescued alignment scoring below min_score is discarded."""

    def __init__(self, max_anchors=2, min_score=0):
        self.max_anchors, self.min_score = max_anchors, min_score

    def to_c(self):
        return _lib.RESCUE_PARAMS(self.max_anchors, self.min_score)


class MultiParams:
    """bg_multi_params_t: max_hits (K, 1 ..= 8) loci reported per read; a candidate scoring below min_score is neither reported
    nor counted as a runner-up; mapq_cap (0 ..= 254) is the MAPQ of a read without a runner-up."""

    def __init__(self, max_hits=1, min_score=-2**31, mapq_cap=60):
        self.max_hits, self.min_score, self.mapq_cap = max_hits, min_score, mapq_cap

    def to_c(self):
        return _lib.MULTI_PARAMS(self.max_hits, self.min_score, self.mapq_cap)


class PairQualityParams:
    """bg_pairq_params_t: a candidate scoring below min_score is no alternative placement of a mate (and no runner-up); mapq_cap
    (0 ..= 254) is the MAPQ of a mate without an alternative."""

    def __init__(self, min_score=-2**31, mapq_cap=60):
        self.min_score, self.mapq_cap = min_score, mapq_cap

    def to_c(self):
        return _lib.PAIRQ_PARAMS(self.min_score, self.mapq_cap)


def attach_text(fm, text=None, d_text=None):
    """bg_fm_set_text (host bytes, copied) or bg_fm_set_text_dev (a uint8 cuda tensor, borrowed): all n bytes the
    index was built from, final sentinel included."""
    if d_text is not None:
        fm._text_keepalive = d_text
        _lib.check(_lib.lib().bg_fm_set_text_dev(fm.h, d_text.data_ptr(), d_text.numel()), "bg_fm_set_text_dev")
    else:
        t = _lib.as_u8(text)
        _lib.check(_lib.lib().bg_fm_set_text(fm.h, t.ctypes.data, len(t)), "bg_fm_set_text")


def seed_extend_arrays(fm, scoring, reads, read_off, params=None, want_ops=True, allow_out_of_alphabet=False):
    """Host-buffer batch: returns (hits: SEED_HIT_DTYPE[n], ops: uint8[], winners' operations back to back).
    A seed that reaches a byte outside the index's alphabet raises AlphabetError (the reference's backward_search
    panics there) unless allow_out_of_alphabet: such seeds simply do not vote."""
    params = params or SeedParams()
    rd = _lib.as_u8(reads)
    off = np.ascontiguousarray(read_off, dtype=np.uint64)
    n = len(off) - 1
    hits = np.zeros(n, dtype=_lib.SEED_HIT_DTYPE)
    cap = int(2 * off[-1] + (2 * params.pad + 4) * n) + 8 if want_ops else 0
    ops = np.zeros(max(cap, 1), dtype=np.uint8) if want_ops else None
    used = C.c_uint64(0)
    sc, pc = scoring.to_c(), params.to_c()
    rc = _lib.lib().bg_seed_extend_batch(fm.h, C.byref(sc), C.byref(pc), n, rd.ctypes.data, off.ctypes.data,
                                         hits.ctypes.data, ops.ctypes.data if want_ops else None, cap, C.byref(used))
    if not (rc == -7 and allow_out_of_alphabet):
        _lib.check(rc, "bg_seed_extend_batch")
    return hits, (ops[:used.value] if want_ops else None)


def seed_extend_dev(fm, scoring, n_reads, d_reads, d_read_off, max_read_len, d_hits, d_ops=0, ops_stride=0, params=None,
                    stream=0, totals=None):
    """Device-resident batch (pointers are ints); `totals`, if given, is a uint64[2] numpy array that receives
    (suffix-array rows resolved, candidates aligned)."""
    params = params or SeedParams()
    sc, pc = scoring.to_c(), params.to_c()
    _lib.check(_lib.lib().bg_seed_extend_batch_dev(fm.h, C.byref(sc), C.byref(pc), n_reads, d_reads, d_read_off, max_read_len,
                                                   d_hits, d_ops, ops_stride, totals.ctypes.data if totals is not None else None,
                                                   stream), "bg_seed_extend_batch_dev")


def seed_extend_strands_arrays(fm, scoring, reads, read_off, params=None, strands=_lib.STRAND_BOTH, want_ops=True,
                               allow_out_of_alphabet=False):
    """bg_seed_extend_strands_batch, host buffers: returns (hits: SEED_HIT_DTYPE[n], strand: uint8[n] of HIT_FORWARD /
    HIT_REVERSE / HIT_NONE, ops: the winners' operations back to back).  A reverse-strand winner's alignment and operations
    refer to revcomp(read) against the forward text.  Errors as seed_extend_arrays."""
    params = params or SeedParams()
    rd = _lib.as_u8(reads)
    off = np.ascontiguousarray(read_off, dtype=np.uint64)
    n = len(off) - 1
    hits = np.zeros(n, dtype=_lib.SEED_HIT_DTYPE)
    strand = np.zeros(max(n, 1), dtype=np.uint8)
    cap = int(2 * off[-1] + (2 * params.pad + 4) * n) + 8 if want_ops else 0
    ops = np.zeros(max(cap, 1), dtype=np.uint8) if want_ops else None
    used = C.c_uint64(0)
    sc, pc = scoring.to_c(), params.to_c()
    rc = _lib.lib().bg_seed_extend_strands_batch(fm.h, C.byref(sc), C.byref(pc), strands, n, rd.ctypes.data, off.ctypes.data,
                                                 hits.ctypes.data, strand.ctypes.data, ops.ctypes.data if want_ops else None, cap,
                                                 C.byref(used))
    if not (rc == -7 and allow_out_of_alphabet):
        _lib.check(rc, "bg_seed_extend_strands_batch")
    return hits, strand[:n], (ops[:used.value] if want_ops else None)


def seed_extend_strands_dev(fm, scoring, n_reads, d_reads, d_read_off, max_read_len, d_hits, d_strand=0, d_ops=0, ops_stride=0,
                            params=None, strands=_lib.STRAND_BOTH, stream=0, totals=None):
    """bg_seed_extend_strands_batch_dev (pointers are ints; d_strand / d_ops may be 0); `totals` as seed_extend_dev, summed
    over the strands that ran."""
    params = params or SeedParams()
    sc, pc = scoring.to_c(), params.to_c()
    _lib.check(_lib.lib().bg_seed_extend_strands_batch_dev(fm.h, C.byref(sc), C.byref(pc), strands, n_reads, d_reads, d_read_off,
                                                           max_read_len, d_hits, d_strand or None, d_ops or None, ops_stride,
                                                           totals.ctypes.data if totals is not None else None, stream),
               "bg_seed_extend_strands_batch_dev")


def seed_extend_pairs_arrays(fm, scoring, reads, read_off, params=None, pair_params=None, want_ops=True, allow_out_of_alphabet=False):
    """bg_seed_extend_pairs_batch, host buffers.  The reads are interleaved mates: read 2p is mate 1 of pair p, read 2p + 1 its
    mate 2 (an even count).  Returns (hits: SEED_HIT_DTYPE[2n], strand: uint8[2n], pairs: PAIR_HIT_DTYPE[n], ops: the reported
    hits' operations back to back).  Errors as seed_extend_arrays."""
    params = params or SeedParams()
    pair_params = pair_params or PairParams()
    rd = _lib.as_u8(reads)
    off = np.ascontiguousarray(read_off, dtype=np.uint64)
    n = len(off) - 1
    if n % 2:
        raise ValueError("seed_extend_pairs_arrays: an odd number of reads")
    hits = np.zeros(n, dtype=_lib.SEED_HIT_DTYPE)
    strand = np.zeros(max(n, 1), dtype=np.uint8)
    pairs = np.zeros(max(n // 2, 1), dtype=_lib.PAIR_HIT_DTYPE)
    cap = int(2 * off[-1] + (2 * params.pad + 4) * n) + 8 if want_ops else 0
    ops = np.zeros(max(cap, 1), dtype=np.uint8) if want_ops else None
    used = C.c_uint64(0)
    sc, pc, pp = scoring.to_c(), params.to_c(), pair_params.to_c()
    rc = _lib.lib().bg_seed_extend_pairs_batch(fm.h, C.byref(sc), C.byref(pc), C.byref(pp), n // 2, rd.ctypes.data, off.ctypes.data,
                                               hits.ctypes.data, strand.ctypes.data, pairs.ctypes.data,
                                               ops.ctypes.data if want_ops else None, cap, C.byref(used))
    if not (rc == -7 and allow_out_of_alphabet):
        _lib.check(rc, "bg_seed_extend_pairs_batch")
    return hits, strand[:n], pairs[:n // 2], (ops[:used.value] if want_ops else None)


def seed_extend_pairs_dev(fm, scoring, n_pairs, d_reads, d_read_off, max_read_len, d_hits, d_pairs, d_strand=0, d_ops=0, ops_stride=0,
                          params=None, pair_params=None, stream=0, totals=None):
    """bg_seed_extend_pairs_batch_dev (pointers are ints; 2 n_pairs interleaved mates, d_pairs: n_pairs bg_pair_hit_t; d_strand /
    d_ops may be 0); `totals` as seed_extend_dev, over both strands of every mate."""
    params = params or SeedParams()
    pair_params = pair_params or PairParams()
    sc, pc, pp = scoring.to_c(), params.to_c(), pair_params.to_c()
    _lib.check(_lib.lib().bg_seed_extend_pairs_batch_dev(fm.h, C.byref(sc), C.byref(pc), C.byref(pp), n_pairs, d_reads, d_read_off,
                                                         max_read_len, d_hits, d_strand or None, d_pairs or None, d_ops or None,
                                                         ops_stride, totals.ctypes.data if totals is not None else None, stream),
               "bg_seed_extend_pairs_batch_dev")


def seed_extend_pairs_mapq_arrays(fm, scoring, reads, read_off, params=None, pair_params=None, quality_params=None, want_ops=True,
                                  allow_out_of_alphabet=False):
    """bg_seed_extend_pairs_mapq_batch, host buffers: seed_extend_pairs_arrays plus a mapping quality per mate.  Returns (hits,
    strand, pairs, multi: MULTI_HIT_DTYPE[2n] — read r's MAPQ, its best alternative's score and n_loci —, ops)."""
    params = params or SeedParams()
    pair_params = pair_params or PairParams()
    quality_params = quality_params or PairQualityParams()
    rd = _lib.as_u8(reads)
    off = np.ascontiguousarray(read_off, dtype=np.uint64)
    n = len(off) - 1
    if n % 2:
        raise ValueError("seed_extend_pairs_mapq_arrays: an odd number of reads")
    hits = np.zeros(n, dtype=_lib.SEED_HIT_DTYPE)
    strand = np.zeros(max(n, 1), dtype=np.uint8)
    pairs = np.zeros(max(n // 2, 1), dtype=_lib.PAIR_HIT_DTYPE)
    multi = np.zeros(max(n, 1), dtype=_lib.MULTI_HIT_DTYPE)
    cap = int(2 * off[-1] + (2 * params.pad + 4) * n) + 8 if want_ops else 0
    ops = np.zeros(max(cap, 1), dtype=np.uint8) if want_ops else None
    used = C.c_uint64(0)
    sc, pc, pp, qp = scoring.to_c(), params.to_c(), pair_params.to_c(), quality_params.to_c()
    rc = _lib.lib().bg_seed_extend_pairs_mapq_batch(fm.h, C.byref(sc), C.byref(pc), C.byref(pp), C.byref(qp), n // 2, rd.ctypes.data,
                                                    off.ctypes.data, hits.ctypes.data, strand.ctypes.data, pairs.ctypes.data,
                                                    multi.ctypes.data, ops.ctypes.data if want_ops else None, cap, C.byref(used))
    if not (rc == -7 and allow_out_of_alphabet):
        _lib.check(rc, "bg_seed_extend_pairs_mapq_batch")
    return hits, strand[:n], pairs[:n // 2], multi[:n], (ops[:used.value] if want_ops else None)


def seed_extend_pairs_mapq_dev(fm, scoring, n_pairs, d_reads, d_read_off, max_read_len, d_hits, d_pairs, d_multi, d_strand=0, d_ops=0,
                               ops_stride=0, params=None, pair_params=None, quality_params=None, stream=0, totals=None):
    """bg_seed_extend_pairs_mapq_batch_dev (pointers are ints; as seed_extend_pairs_dev, plus d_multi: 2 n_pairs bg_multi_hit_t,
    which bg_sam_emit_batch_dev takes as its d_multi together with SAM_PAIRED)."""
    params = params or SeedParams()
    pair_params = pair_params or PairParams()
    quality_params = quality_params or PairQualityParams()
    sc, pc, pp, qp = scoring.to_c(), params.to_c(), pair_params.to_c(), quality_params.to_c()
    _lib.check(_lib.lib().bg_seed_extend_pairs_mapq_batch_dev(fm.h, C.byref(sc), C.byref(pc), C.byref(pp), C.byref(qp), n_pairs, d_reads,
                                                              d_read_off, max_read_len, d_hits, d_strand or None, d_pairs or None,
                                                              d_multi or None, d_ops or None, ops_stride,
                                                              totals.ctypes.data if totals is not None else None, stream),
               "bg_seed_extend_pairs_mapq_batch_dev")


def seed_extend_pairs_rescue_arrays(fm, scoring, reads, read_off, params=None, pair_params=None, rescue_params=None, want_ops=True,
                                    allow_out_of_alphabet=False):
    """bg_seed_extend_pairs_rescue_batch, host buffers: seed_extend_pairs_arrays plus mate rescue.  Returns (hits, strand, pairs,
    rescued: uint8[n] — 0, or 1 / 2: the mate that was placed inside its partner's insert window —, ops)."""
    params = params or SeedParams()
    pair_params = pair_params or PairParams()
    rescue_params = rescue_params or RescueParams()
    rd = _lib.as_u8(reads)
    off = np.ascontiguousarray(read_off, dtype=np.uint64)
    n = len(off) - 1
    if n % 2:
        raise ValueError("seed_extend_pairs_rescue_arrays: an odd number of reads")
    hits = np.zeros(n, dtype=_lib.SEED_HIT_DTYPE)
    strand = np.zeros(max(n, 1), dtype=np.uint8)
    pairs = np.zeros(max(n // 2, 1), dtype=_lib.PAIR_HIT_DTYPE)
    rescued = np.zeros(max(n // 2, 1), dtype=np.uint8)
    # a reported hit has at most read + window operations; a rescue window is up to max_span bytes
    cap = int(off[-1] + (max(int(np.diff(off).max(initial=0)) + 2 * params.pad, pair_params.max_span) + 4) * n) + 8 if want_ops else 0
    ops = np.zeros(max(cap, 1), dtype=np.uint8) if want_ops else None
    used = C.c_uint64(0)
    sc, pc, pp, rp = scoring.to_c(), params.to_c(), pair_params.to_c(), rescue_params.to_c()
    rc = _lib.lib().bg_seed_extend_pairs_rescue_batch(fm.h, C.byref(sc), C.byref(pc), C.byref(pp), C.byref(rp), n // 2, rd.ctypes.data,
                                                      off.ctypes.data, hits.ctypes.data, strand.ctypes.data, pairs.ctypes.data,
                                                      rescued.ctypes.data, ops.ctypes.data if want_ops else None, cap, C.byref(used))
    if not (rc == -7 and allow_out_of_alphabet):
        _lib.check(rc, "bg_seed_extend_pairs_rescue_batch")
    return hits, strand[:n], pairs[:n // 2], rescued[:n // 2], (ops[:used.value] if want_ops else None)


def seed_extend_pairs_rescue_dev(fm, scoring, n_pairs, d_reads, d_read_off, max_read_len, d_hits, d_pairs, d_rescued, d_strand=0, d_ops=0,
                                 ops_stride=0, params=None, pair_params=None, rescue_params=None, stream=0, totals=None):
    """bg_seed_extend_pairs_rescue_batch_dev (pointers are ints; as seed_extend_pairs_dev, plus d_rescued: n_pairs bytes;
    ops_stride >= max_read_len + max(max_read_len + 2 pad, max_span) + 4); `totals`, if given, is a uint64[4] numpy array that
    receives (suffix-array rows resolved, seeded candidates aligned, rescue alignments run, pairs rescued)."""
    params = params or SeedParams()
    pair_params = pair_params or PairParams()
    rescue_params = rescue_params or RescueParams()
    sc, pc, pp, rp = scoring.to_c(), params.to_c(), pair_params.to_c(), rescue_params.to_c()
    _lib.check(_lib.lib().bg_seed_extend_pairs_rescue_batch_dev(fm.h, C.byref(sc), C.byref(pc), C.byref(pp), C.byref(rp), n_pairs, d_reads,
                                                                d_read_off, max_read_len, d_hits, d_strand or None, d_pairs or None,
                                                                d_rescued or None, d_ops or None, ops_stride,
                                                                totals.ctypes.data if totals is not None else None, stream),
               "bg_seed_extend_pairs_rescue_batch_dev")


def seed_extend_pairs_rescue_mapq_arrays(fm, scoring, reads, read_off, params=None, pair_params=None, rescue_params=None,
                                         quality_params=None, want_ops=True, allow_out_of_alphabet=False):
    """bg_seed_extend_pairs_rescue_mapq_batch, host buffers: seed_extend_pairs_rescue_arrays plus a mapping quality per mate, the
    mates of rescued pairs included.  Returns (hits, strand, pairs, rescued, multi: MULTI_HIT_DTYPE[2n], ops)."""
    params = params or SeedParams()
    pair_params = pair_params or PairParams()
    rescue_params = rescue_params or RescueParams()
    quality_params = quality_params or PairQualityParams()
    rd = _lib.as_u8(reads)
    off = np.ascontiguousarray(read_off, dtype=np.uint64)
    n = len(off) - 1
    if n % 2:
        raise ValueError("seed_extend_pairs_rescue_mapq_arrays: an odd number of reads")
    hits = np.zeros(n, dtype=_lib.SEED_HIT_DTYPE)
    strand = np.zeros(max(n, 1), dtype=np.uint8)
    pairs = np.zeros(max(n // 2, 1), dtype=_lib.PAIR_HIT_DTYPE)
    rescued = np.zeros(max(n // 2, 1), dtype=np.uint8)
    multi = np.zeros(max(n, 1), dtype=_lib.MULTI_HIT_DTYPE)
    # a reported hit has at most read + window operations; a rescue window is up to max_span bytes
    cap = int(off[-1] + (max(int(np.diff(off).max(initial=0)) + 2 * params.pad, pair_params.max_span) + 4) * n) + 8 if want_ops else 0
    ops = np.zeros(max(cap, 1), dtype=np.uint8) if want_ops else None
    used = C.c_uint64(0)
    sc, pc, pp, rp, qp = scoring.to_c(), params.to_c(), pair_params.to_c(), rescue_params.to_c(), quality_params.to_c()
    rc = _lib.lib().bg_seed_extend_pairs_rescue_mapq_batch(fm.h, C.byref(sc), C.byref(pc), C.byref(pp), C.byref(rp), C.byref(qp), n // 2,
                                                           rd.ctypes.data, off.ctypes.data, hits.ctypes.data, strand.ctypes.data,
                                                           pairs.ctypes.data, rescued.ctypes.data, multi.ctypes.data,
                                                           ops.ctypes.data if want_ops else None, cap, C.byref(used))
    if not (rc == -7 and allow_out_of_alphabet):
        _lib.check(rc, "bg_seed_extend_pairs_rescue_mapq_batch")
    return hits, strand[:n], pairs[:n // 2], rescued[:n // 2], multi[:n], (ops[:used.value] if want_ops else None)


def seed_extend_pairs_rescue_mapq_dev(fm, scoring, n_pairs, d_reads, d_read_off, max_read_len, d_hits, d_pairs, d_rescued, d_multi,
                                      d_strand=0, d_ops=0, ops_stride=0, params=None, pair_params=None, rescue_params=None,
                                      quality_params=None, stream=0, totals=None):
    """bg_seed_extend_pairs_rescue_mapq_batch_dev (pointers are ints; as seed_extend_pairs_rescue_dev, plus d_multi: 2 n_pairs
    bg_multi_hit_t, which bg_sam_emit_batch_dev takes as its d_multi together with SAM_PAIRED); `totals` as
    seed_extend_pairs_rescue_dev."""
    params = params or SeedParams()
    pair_params = pair_params or PairParams()
    rescue_params = rescue_params or RescueParams()
    quality_params = quality_params or PairQualityParams()
    sc, pc, pp, rp, qp = scoring.to_c(), params.to_c(), pair_params.to_c(), rescue_params.to_c(), quality_params.to_c()
    _lib.check(_lib.lib().bg_seed_extend_pairs_rescue_mapq_batch_dev(fm.h, C.byref(sc), C.byref(pc), C.byref(pp), C.byref(rp), C.byref(qp),
                                                                     n_pairs, d_reads, d_read_off, max_read_len, d_hits, d_strand or None,
                                                                     d_pairs or None, d_rescued or None, d_multi or None, d_ops or None,
                                                                     ops_stride, totals.ctypes.data if totals is not None else None,
                                                                     stream),
               "bg_seed_extend_pairs_rescue_mapq_batch_dev")


def seed_extend_multi_arrays(fm, scoring, reads, read_off, params=None, multi_params=None, strands=_lib.STRAND_BOTH, want_ops=True,
                             allow_out_of_alphabet=False):
    """bg_seed_extend_multi_batch, host buffers.  With K = multi_params.max_hits, returns (hits: SEED_HIT_DTYPE[n, K], strand:
    uint8[n, K], multi: MULTI_HIT_DTYPE[n], ops: the reported hits' operations back to back in slot order): read r's loci are
    hits[r, :multi["n_reported"][r]], the best first; the other slots read like an unmapped read.  Errors as seed_extend_arrays."""
    params = params or SeedParams()
    multi_params = multi_params or MultiParams()
    rd = _lib.as_u8(reads)
    off = np.ascontiguousarray(read_off, dtype=np.uint64)
    n = len(off) - 1
    K = max(int(multi_params.max_hits), 1) if 0 < multi_params.max_hits <= _lib.SEED_MAX_HITS else 1  # (the call rejects the rest)
    hits = np.zeros((n, K), dtype=_lib.SEED_HIT_DTYPE)
    strand = np.zeros(max(n * K, 1), dtype=np.uint8)
    multi = np.zeros(max(n, 1), dtype=_lib.MULTI_HIT_DTYPE)
    cap = K * (int(2 * off[-1] + (2 * params.pad + 4) * n) + 8) if want_ops else 0
    ops = np.zeros(max(cap, 1), dtype=np.uint8) if want_ops else None
    used = C.c_uint64(0)
    sc, pc, mp = scoring.to_c(), params.to_c(), multi_params.to_c()
    rc = _lib.lib().bg_seed_extend_multi_batch(fm.h, C.byref(sc), C.byref(pc), C.byref(mp), strands, n, rd.ctypes.data, off.ctypes.data,
                                               hits.ctypes.data, strand.ctypes.data, multi.ctypes.data,
                                               ops.ctypes.data if want_ops else None, cap, C.byref(used))
    if not (rc == -7 and allow_out_of_alphabet):
        _lib.check(rc, "bg_seed_extend_multi_batch")
    return hits, strand[:n * K].reshape(n, K), multi[:n], (ops[:used.value] if want_ops else None)


def seed_extend_multi_dev(fm, scoring, n_reads, d_reads, d_read_off, max_read_len, d_hits, d_multi, d_strand=0, d_ops=0, ops_stride=0,
                          params=None, multi_params=None, strands=_lib.STRAND_BOTH, stream=0, totals=None):
    """bg_seed_extend_multi_batch_dev (pointers are ints; d_hits / d_strand / d_ops hold max_hits slots per read, slot K r + k,
    d_multi n_reads bg_multi_hit_t; d_strand / d_ops may be 0); `totals` as seed_extend_strands_dev."""
    params = params or SeedParams()
    multi_params = multi_params or MultiParams()
    sc, pc, mp = scoring.to_c(), params.to_c(), multi_params.to_c()
    _lib.check(_lib.lib().bg_seed_extend_multi_batch_dev(fm.h, C.byref(sc), C.byref(pc), C.byref(mp), strands, n_reads, d_reads,
                                                         d_read_off, max_read_len, d_hits, d_strand or None, d_multi or None,
                                                         d_ops or None, ops_stride, totals.ctypes.data if totals is not None else None,
                                                         stream),
               "bg_seed_extend_multi_batch_dev")


def revcomp_dev(n, d_in, d_off, d_out, ctx=None, stream=0):
    """bg_revcomp_batch_dev: d_out[d_off[i] .. d_off[i + 1]) = dna::revcomp of the same range of d_in, for i < n (pointers
    are ints; asynchronous on `stream`)."""
    ctx = ctx or _lib.default_context()
    _lib.check(_lib.lib().bg_revcomp_batch_dev(ctx.h, n, d_in, d_off, d_out, stream), "bg_revcomp_batch_dev")
