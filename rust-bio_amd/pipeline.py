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
do not touch, the runner-up's score and a MAPQ.  The `_smem` calls take an FMD index over T$R$ and seed both strands with the
SMEMs of each read (`FMDIndex::all_smems`) instead of fixed windows.  The `_tiered` calls take the same index, seed every read with
fixed windows searched once for both strands, and re-seed with SMEMs only the reads whose winner scores below a threshold.  This
module only marshals arguments."""
import ctypes as C

import numpy as np

from . import _lib
from .pairwise import MIN_SCORE  # noqa: F401  (score of an unmapped read)


class SeedParams:
    def __init__(self, seed_len=20, stride=10, max_occ=16, pad=25):
        self.seed_len, self.stride, self.max_occ, self.pad = seed_len, stride, max_occ, pad

    def to_c(self):
        return _lib.SeedParamsC(self.seed_len, self.stride, self.max_occ, self.pad)


class SmemSeedParams:
    """bg_smem_seed_params_t: the records of FMDIndex::all_smems(read, min_seed_len) seed the read; the first max_smems of a read
    are used, one whose interval holds more than max_occ rows does not vote; pad as SeedParams."""

    def __init__(self, min_seed_len=19, max_smems=16, max_occ=16, pad=25):
        self.min_seed_len, self.max_smems, self.max_occ, self.pad = min_seed_len, max_smems, max_occ, pad

    def to_c(self):
        return _lib.SMEM_SEED_PARAMS(self.min_seed_len, self.max_smems, self.max_occ, self.pad)


class TieredSeedParams:
    """bg_tiered_seed_params_t: `window` (a SeedParams) seeds every read on the FMD index, `smem` (a SmemSeedParams, the same pad)
    the reads whose tier-1 winner scores below reseed_below (MIN_SCORE: none, 2**31 - 1: all)."""

    def __init__(self, window=None, smem=None, reseed_below=MIN_SCORE):
        self.window, self.smem, self.reseed_below = window or SeedParams(), smem or SmemSeedParams(), reseed_below

    @property
    def pad(self):
        return max(self.window.pad, self.smem.pad)

    def to_c(self):
        return _lib.TIERED_SEED_PARAMS(self.window.to_c(), self.smem.to_c(), self.reseed_below)


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


_OUT_DTYPE = {"strand": np.uint8, "tier": np.uint8, "pairs": _lib.PAIR_HIT_DTYPE, "rescued": np.uint8, "multi": _lib.MULTI_HIT_DTYPE}


def _host_call(stem, fm, scoring, reads, read_off, *, params, want_ops, allow_out_of_alphabet, modes=(), outs=(), strands=None, K=None,
               max_span=None, allow_truncated=False):
    """The host-buffer call bg_<stem>_batch, behind the public function <stem>_arrays.  modes: the mode's parameter objects in the call's order; outs: the
    names of its output arrays after `hits`, in the call's order (keys of _OUT_DTYPE); strands: None for a call without that
    argument; K: slots per read of the multi call; max_span: of a rescue call, whose operation slots also hold a rescue window;
    allow_truncated: of the SMEM and tiered calls, whose status BG_ERR_OPS_CAP (-9) says that a read had more records than max_smems.
    Returns (hits, *outs, ops)."""
    name = f"bg_{stem}_batch"
    params = params or SeedParams()
    rd = _lib.as_u8(reads)
    off = np.ascontiguousarray(read_off, dtype=np.uint64)
    n = len(off) - 1
    if "pairs" in outs and n % 2:
        raise ValueError(f"{stem}_arrays: an odd number of reads")
    hits = np.zeros(n if K is None else (n, K), dtype=_lib.SEED_HIT_DTYPE)
    K = K or 1
    size = {"strand": n * K, "tier": n, "pairs": n // 2, "rescued": n // 2, "multi": n}
    arrays = [np.zeros(max(size[o], 1), dtype=_OUT_DTYPE[o]) for o in outs]
    if not want_ops:
        cap = 0
    elif max_span is None:
        cap = K * (int(2 * off[-1] + (2 * params.pad + 4) * n) + 8)
    else:
        # a reported hit has at most read + window operations; a rescue window is up to max_span bytes
        cap = int(off[-1] + (max(int(np.diff(off).max(initial=0)) + 2 * params.pad, max_span) + 4) * n) + 8
    ops = np.zeros(max(cap, 1), dtype=np.uint8) if want_ops else None
    used = C.c_uint64(0)
    structs = [scoring.to_c(), params.to_c()] + [m.to_c() for m in modes]
    rc = getattr(_lib.lib(), name)(fm.h, *map(C.byref, structs), *([] if strands is None else [strands]), n // 2 if "pairs" in outs else n,
                                   rd.ctypes.data, off.ctypes.data, hits.ctypes.data, *[a.ctypes.data for a in arrays],
                                   ops.ctypes.data if want_ops else None, cap, C.byref(used))
    if not (rc == -7 and allow_out_of_alphabet) and not (rc == -9 and allow_truncated):
        _lib.check(rc, name)
    return (hits, *[a[:size[o]] for a, o in zip(arrays, outs)], ops[:used.value] if want_ops else None)


def _dev_call(stem, fm, scoring, n, d_reads, d_read_off, max_read_len, *, d_hits, d_outs, d_ops, ops_stride, params, stream, totals,
              modes=(), strands=None):
    """The device-resident call bg_<stem>_batch_dev (pointers are ints, 0: absent); modes, strands as _host_call,
    d_outs: the output pointers after d_hits in the call's order."""
    name = f"bg_{stem}_batch_dev"
    structs = [scoring.to_c(), (params or SeedParams()).to_c()] + [m.to_c() for m in modes]
    _lib.check(getattr(_lib.lib(), name)(fm.h, *map(C.byref, structs), *([] if strands is None else [strands]), n, d_reads, d_read_off,
                                         max_read_len, d_hits, *[d or None for d in d_outs], d_ops or None, ops_stride,
                                         totals.ctypes.data if totals is not None else None, stream), name)


def seed_extend_arrays(fm, scoring, reads, read_off, params=None, want_ops=True, allow_out_of_alphabet=False):
    """Host-buffer batch: returns (hits: SEED_HIT_DTYPE[n], ops: uint8[], winners' operations back to back).
    A seed that reaches a byte outside the index's alphabet raises AlphabetError (the reference's backward_search
    panics there) unless allow_out_of_alphabet: such seeds simply do not vote."""
    return _host_call("seed_extend", fm, scoring, reads, read_off, params=params, want_ops=want_ops,
                      allow_out_of_alphabet=allow_out_of_alphabet)


def seed_extend_dev(fm, scoring, n_reads, d_reads, d_read_off, max_read_len, d_hits, d_ops=0, ops_stride=0, params=None,
                    stream=0, totals=None):
    """Device-resident batch (pointers are ints); `totals`, if given, is a uint64[2] numpy array that receives
    (suffix-array rows resolved, candidates aligned)."""
    _dev_call("seed_extend", fm, scoring, n_reads, d_reads, d_read_off, max_read_len, d_hits=d_hits, d_outs=[], d_ops=d_ops,
              ops_stride=ops_stride, params=params, stream=stream, totals=totals)


def seed_extend_strands_arrays(fm, scoring, reads, read_off, params=None, strands=_lib.STRAND_BOTH, want_ops=True,
                               allow_out_of_alphabet=False):
    """bg_seed_extend_strands_batch, host buffers: returns (hits: SEED_HIT_DTYPE[n], strand: uint8[n] of HIT_FORWARD /
    HIT_REVERSE / HIT_NONE, ops: the winners' operations back to back).  A reverse-strand winner's alignment and operations
    refer to revcomp(read) against the forward text.  Errors as seed_extend_arrays."""
    return _host_call("seed_extend_strands", fm, scoring, reads, read_off, params=params, want_ops=want_ops,
                      allow_out_of_alphabet=allow_out_of_alphabet, outs=["strand"], strands=strands)


def seed_extend_strands_dev(fm, scoring, n_reads, d_reads, d_read_off, max_read_len, d_hits, d_strand=0, d_ops=0, ops_stride=0,
                            params=None, strands=_lib.STRAND_BOTH, stream=0, totals=None):
    """bg_seed_extend_strands_batch_dev (pointers are ints; d_strand / d_ops may be 0); `totals` as seed_extend_dev, summed
    over the strands that ran."""
    _dev_call("seed_extend_strands", fm, scoring, n_reads, d_reads, d_read_off, max_read_len, d_hits=d_hits, d_outs=[d_strand], d_ops=d_ops,
              ops_stride=ops_stride, params=params, stream=stream, totals=totals, strands=strands)


def seed_extend_smem_arrays(fm, scoring, reads, read_off, params=None, strands=_lib.STRAND_BOTH, want_ops=True,
                            allow_out_of_alphabet=False, allow_truncated=False):
    """bg_seed_extend_smem_batch, host buffers: `fm` is an FMD index over T$R$ with all of T$R$ attached and a suffix array.
    Returns (hits, strand, ops) as seed_extend_strands_arrays, in coordinates of the forward text T.  A read on which the
    reference's all_smems panics raises AlphabetError unless allow_out_of_alphabet (it does not vote); a read with more than
    params.max_smems records raises BiogpuError (OPS_CAP) unless allow_truncated (its first max_smems records vote).  Every read
    is answered either way."""
    return _host_call("seed_extend_smem", fm, scoring, reads, read_off, params=params or SmemSeedParams(), want_ops=want_ops,
                      allow_out_of_alphabet=allow_out_of_alphabet, outs=["strand"], strands=strands, allow_truncated=allow_truncated)


def seed_extend_smem_dev(fm, scoring, n_reads, d_reads, d_read_off, max_read_len, d_hits, d_strand=0, d_ops=0, ops_stride=0,
                         params=None, strands=_lib.STRAND_BOTH, stream=0, totals=None):
    """bg_seed_extend_smem_batch_dev (pointers are ints; d_strand / d_ops may be 0); `totals`, if given, is a uint64[2] numpy
    array that receives (suffix-array rows resolved, candidates aligned).  Raises as seed_extend_smem_arrays without its switches;
    the slots are written before it does."""
    _dev_call("seed_extend_smem", fm, scoring, n_reads, d_reads, d_read_off, max_read_len, d_hits=d_hits, d_outs=[d_strand], d_ops=d_ops,
              ops_stride=ops_stride, params=params or SmemSeedParams(), stream=stream, totals=totals, strands=strands)


def seed_extend_tiered_arrays(fm, scoring, reads, read_off, params=None, strands=_lib.STRAND_BOTH, want_ops=True,
                              allow_out_of_alphabet=False, allow_truncated=False):
    """bg_seed_extend_tiered_batch, host buffers: `fm` as seed_extend_smem_arrays takes it.  Returns (hits, strand, tier: uint8[n]
    of TIER_NONE / TIER_FIRST / TIER_SECOND, ops), hits and ops as seed_extend_smem_arrays.  A window that reaches a byte outside
    the alphabet, or a re-seeded read on which all_smems panics, raises AlphabetError unless allow_out_of_alphabet; a re-seeded
    read with more than params.smem.max_smems records raises BiogpuError (OPS_CAP) unless allow_truncated.  Every read is answered
    either way."""
    return _host_call("seed_extend_tiered", fm, scoring, reads, read_off, params=params or TieredSeedParams(), want_ops=want_ops,
                      allow_out_of_alphabet=allow_out_of_alphabet, outs=["strand", "tier"], strands=strands,
                      allow_truncated=allow_truncated)


def seed_extend_tiered_dev(fm, scoring, n_reads, d_reads, d_read_off, max_read_len, d_hits, d_strand=0, d_tier=0, d_ops=0, ops_stride=0,
                           params=None, strands=_lib.STRAND_BOTH, stream=0, totals=None):
    """bg_seed_extend_tiered_batch_dev (pointers are ints; d_strand / d_tier / d_ops may be 0); `totals`, if given, is a uint64[3]
    numpy array that receives (suffix-array rows resolved, candidates aligned, reads re-seeded), the first two over both tiers.
    Raises as seed_extend_tiered_arrays without its switches; the slots are written before it does."""
    _dev_call("seed_extend_tiered", fm, scoring, n_reads, d_reads, d_read_off, max_read_len, d_hits=d_hits, d_outs=[d_strand, d_tier],
              d_ops=d_ops, ops_stride=ops_stride, params=params or TieredSeedParams(), stream=stream, totals=totals, strands=strands)


def seed_extend_pairs_arrays(fm, scoring, reads, read_off, params=None, pair_params=None, want_ops=True, allow_out_of_alphabet=False):
    """bg_seed_extend_pairs_batch, host buffers.  The reads are interleaved mates: read 2p is mate 1 of pair p, read 2p + 1 its
    mate 2 (an even count).  Returns (hits: SEED_HIT_DTYPE[2n], strand: uint8[2n], pairs: PAIR_HIT_DTYPE[n], ops: the reported
    hits' operations back to back).  Errors as seed_extend_arrays."""
    return _host_call("seed_extend_pairs", fm, scoring, reads, read_off, params=params, want_ops=want_ops,
                      allow_out_of_alphabet=allow_out_of_alphabet,
                      modes=[pair_params or PairParams()], outs=["strand", "pairs"])


def seed_extend_pairs_dev(fm, scoring, n_pairs, d_reads, d_read_off, max_read_len, d_hits, d_pairs, d_strand=0, d_ops=0, ops_stride=0,
                          params=None, pair_params=None, stream=0, totals=None):
    """bg_seed_extend_pairs_batch_dev (pointers are ints; 2 n_pairs interleaved mates, d_pairs: n_pairs bg_pair_hit_t; d_strand /
    d_ops may be 0); `totals` as seed_extend_dev, over both strands of every mate."""
    _dev_call("seed_extend_pairs", fm, scoring, n_pairs, d_reads, d_read_off, max_read_len, d_hits=d_hits, d_outs=[d_strand, d_pairs], d_ops=d_ops,
              ops_stride=ops_stride, params=params, stream=stream, totals=totals, modes=[pair_params or PairParams()])


def seed_extend_pairs_mapq_arrays(fm, scoring, reads, read_off, params=None, pair_params=None, quality_params=None, want_ops=True,
                                  allow_out_of_alphabet=False):
    """bg_seed_extend_pairs_mapq_batch, host buffers: seed_extend_pairs_arrays plus a mapping quality per mate.  Returns (hits,
    strand, pairs, multi: MULTI_HIT_DTYPE[2n] — read r's MAPQ, its best alternative's score and n_loci —, ops)."""
    return _host_call("seed_extend_pairs_mapq", fm, scoring, reads, read_off, params=params, want_ops=want_ops,
                      allow_out_of_alphabet=allow_out_of_alphabet,
                      modes=[pair_params or PairParams(), quality_params or PairQualityParams()], outs=["strand", "pairs", "multi"])


def seed_extend_pairs_mapq_dev(fm, scoring, n_pairs, d_reads, d_read_off, max_read_len, d_hits, d_pairs, d_multi, d_strand=0, d_ops=0,
                               ops_stride=0, params=None, pair_params=None, quality_params=None, stream=0, totals=None):
    """bg_seed_extend_pairs_mapq_batch_dev (pointers are ints; as seed_extend_pairs_dev, plus d_multi: 2 n_pairs bg_multi_hit_t,
    which bg_sam_emit_batch_dev takes as its d_multi together with SAM_PAIRED)."""
    _dev_call("seed_extend_pairs_mapq", fm, scoring, n_pairs, d_reads, d_read_off, max_read_len, d_hits=d_hits,
              d_outs=[d_strand, d_pairs, d_multi], d_ops=d_ops,
              ops_stride=ops_stride, params=params, stream=stream, totals=totals, modes=[pair_params or PairParams(), quality_params or PairQualityParams()])


def seed_extend_pairs_rescue_arrays(fm, scoring, reads, read_off, params=None, pair_params=None, rescue_params=None, want_ops=True,
                                    allow_out_of_alphabet=False):
    """bg_seed_extend_pairs_rescue_batch, host buffers: seed_extend_pairs_arrays plus mate rescue.  Returns (hits, strand, pairs,
    rescued: uint8[n] — 0, or 1 / 2: the mate that was placed inside its partner's insert window —, ops)."""
    pair_params = pair_params or PairParams()
    return _host_call("seed_extend_pairs_rescue", fm, scoring, reads, read_off, params=params, want_ops=want_ops,
                      allow_out_of_alphabet=allow_out_of_alphabet,
                      modes=[pair_params, rescue_params or RescueParams()], outs=["strand", "pairs", "rescued"],
                      max_span=pair_params.max_span)


def seed_extend_pairs_rescue_dev(fm, scoring, n_pairs, d_reads, d_read_off, max_read_len, d_hits, d_pairs, d_rescued, d_strand=0, d_ops=0,
                                 ops_stride=0, params=None, pair_params=None, rescue_params=None, stream=0, totals=None):
    """bg_seed_extend_pairs_rescue_batch_dev (pointers are ints; as seed_extend_pairs_dev, plus d_rescued: n_pairs bytes;
    ops_stride >= max_read_len + max(max_read_len + 2 pad, max_span) + 4); `totals`, if given, is a uint64[4] numpy array that
    receives (suffix-array rows resolved, seeded candidates aligned, rescue alignments run, pairs rescued)."""
    _dev_call("seed_extend_pairs_rescue", fm, scoring, n_pairs, d_reads, d_read_off, max_read_len, d_hits=d_hits,
              d_outs=[d_strand, d_pairs, d_rescued], d_ops=d_ops,
              ops_stride=ops_stride, params=params, stream=stream, totals=totals,
              modes=[pair_params or PairParams(), rescue_params or RescueParams()])


def seed_extend_pairs_rescue_mapq_arrays(fm, scoring, reads, read_off, params=None, pair_params=None, rescue_params=None,
                                         quality_params=None, want_ops=True, allow_out_of_alphabet=False):
    """bg_seed_extend_pairs_rescue_mapq_batch, host buffers: seed_extend_pairs_rescue_arrays plus a mapping quality per mate, the
    mates of rescued pairs included.  Returns (hits, strand, pairs, rescued, multi: MULTI_HIT_DTYPE[2n], ops)."""
    pair_params = pair_params or PairParams()
    return _host_call("seed_extend_pairs_rescue_mapq", fm, scoring, reads, read_off, params=params, want_ops=want_ops,
                      allow_out_of_alphabet=allow_out_of_alphabet,
                      modes=[pair_params, rescue_params or RescueParams(), quality_params or PairQualityParams()],
                      outs=["strand", "pairs", "rescued", "multi"], max_span=pair_params.max_span)


def seed_extend_pairs_rescue_mapq_dev(fm, scoring, n_pairs, d_reads, d_read_off, max_read_len, d_hits, d_pairs, d_rescued, d_multi,
                                      d_strand=0, d_ops=0, ops_stride=0, params=None, pair_params=None, rescue_params=None,
                                      quality_params=None, stream=0, totals=None):
    """bg_seed_extend_pairs_rescue_mapq_batch_dev (pointers are ints; as seed_extend_pairs_rescue_dev, plus d_multi: 2 n_pairs
    bg_multi_hit_t, which bg_sam_emit_batch_dev takes as its d_multi together with SAM_PAIRED); `totals` as
    seed_extend_pairs_rescue_dev."""
    _dev_call("seed_extend_pairs_rescue_mapq", fm, scoring, n_pairs, d_reads, d_read_off, max_read_len, d_hits=d_hits,
              d_outs=[d_strand, d_pairs, d_rescued, d_multi], d_ops=d_ops,
              ops_stride=ops_stride, params=params, stream=stream, totals=totals,
              modes=[pair_params or PairParams(), rescue_params or RescueParams(), quality_params or PairQualityParams()])


def seed_extend_multi_arrays(fm, scoring, reads, read_off, params=None, multi_params=None, strands=_lib.STRAND_BOTH, want_ops=True,
                             allow_out_of_alphabet=False):
    """bg_seed_extend_multi_batch, host buffers.  With K = multi_params.max_hits, returns (hits: SEED_HIT_DTYPE[n, K], strand:
    uint8[n, K], multi: MULTI_HIT_DTYPE[n], ops: the reported hits' operations back to back in slot order): read r's loci are
    hits[r, :multi["n_reported"][r]], the best first; the other slots read like an unmapped read.  Errors as seed_extend_arrays."""
    multi_params = multi_params or MultiParams()
    K = max(int(multi_params.max_hits), 1) if 0 < multi_params.max_hits <= _lib.SEED_MAX_HITS else 1  # (the call rejects the rest)
    hits, strand, multi, ops = _host_call("seed_extend_multi", fm, scoring, reads, read_off, params=params, want_ops=want_ops,
                      allow_out_of_alphabet=allow_out_of_alphabet, modes=[multi_params], outs=["strand", "multi"], strands=strands, K=K)
    return hits, strand.reshape(len(hits), K), multi, ops


def seed_extend_multi_dev(fm, scoring, n_reads, d_reads, d_read_off, max_read_len, d_hits, d_multi, d_strand=0, d_ops=0, ops_stride=0,
                          params=None, multi_params=None, strands=_lib.STRAND_BOTH, stream=0, totals=None):
    """bg_seed_extend_multi_batch_dev (pointers are ints; d_hits / d_strand / d_ops hold max_hits slots per read, slot K r + k,
    d_multi n_reads bg_multi_hit_t; d_strand / d_ops may be 0); `totals` as seed_extend_strands_dev."""
    _dev_call("seed_extend_multi", fm, scoring, n_reads, d_reads, d_read_off, max_read_len, d_hits=d_hits, d_outs=[d_strand, d_multi], d_ops=d_ops,
              ops_stride=ops_stride, params=params, stream=stream, totals=totals, modes=[multi_params or MultiParams()], strands=strands)


def revcomp_dev(n, d_in, d_off, d_out, ctx=None, stream=0):
    """bg_revcomp_batch_dev: d_out[d_off[i] .. d_off[i + 1]) = dna::revcomp of the same range of d_in, for i < n (pointers
    are ints; asynchronous on `stream`)."""
    ctx = ctx or _lib.default_context()
    _lib.check(_lib.lib().bg_revcomp_batch_dev(ctx.h, n, d_in, d_off, d_out, stream), "bg_revcomp_batch_dev")
