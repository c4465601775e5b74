"""`bio::pattern_matching::myers::Myers<u64>` and `MyersBuilder` (src/pattern_matching/myers/) on the device
(csrc/myers.hip), plus trimming of parsed FASTQ records by the hits (csrc/fastq_trim.hip; the rule is defined in
include/biogpu.h, rust-bio has no trimmer).

In scope: patterns of 1 to 64 symbols (`Myers`, DistType u8) and, block-based, of up to 1024 (`MyersLong`, the reference's
`myers::long::Myers<u64>`, DistType usize; csrc/myers_long.hip): `distance`, `find_all_end`, `find_best_end`, `find_all`, the
best hit's alignment with its path.  Out of scope: `Myers<u128>`, `find_all_lazy`.  The pattern's `peq` table
(simple.rs:55-74) is built here on the host; everything that walks a text runs on the GPU, one text or a batch."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (ALN_DTYPE, MIN_SCORE, MYERS_ENDS_ONLY, MYERS_LONG_MAX_M, MYERS_MAX_HITS, MYERS_PATTERN_DTYPE, TRIM_3P,  # noqa: F401
                   TRIM_5P)

OPS = ["Match", "Subst", "Del", "Ins"]


class Myers:
    """Myers::<u64>::new(pattern) (simple.rs:29-82)"""

    def __init__(self, pattern, ambigs=None, wildcards=None, ctx=None):
        pattern = bytes(pattern)
        if len(pattern) > 64:
            raise ValueError("Pattern too long")  # simple.rs:52
        if len(pattern) == 0:
            raise ValueError("Pattern is empty")  # simple.rs:53
        peq = [0] * 256
        for i, symbol in enumerate(pattern):  # simple.rs:57-68
            mask = 1 << i
            peq[symbol] |= mask
            for eq in (ambigs or {}).get(symbol, ()):
                peq[eq] |= mask
        for w in wildcards or ():  # simple.rs:70-74
            peq[w] = (1 << 64) - 1
        self.peq = np.array(peq, dtype=np.uint64)
        self.m = len(pattern)
        self._ctx = ctx

    # ---- one text -------------------------------------------------------------------------------------------------
    def _one(self, text):
        t = _lib.as_u8(text)
        return t, np.array([0, len(t)], dtype=np.uint64)

    def distance(self, text):
        """myers_impl.rs:163-181: the smallest distance over all end columns; 255 for an empty text"""
        t, off = self._one(text)
        aln, _ = best_batch([self], t, off, 255, ctx=self._ctx)
        return 255 if aln["score"][0] == MIN_SCORE else int(aln["score"][0])

    def find_best_end(self, text):
        """myers_impl.rs:199-207: (end, dist), the first end among equal distances; raises on an empty text (unwrap)"""
        t, off = self._one(text)
        aln, _ = best_batch([self], t, off, 255, ctx=self._ctx)
        if aln["score"][0] == MIN_SCORE:
            raise ValueError("find_best_end: no end column (empty text)")
        return int(aln["yend"][0]) - 1, int(aln["score"][0])

    def _all(self, text, max_dist, ends_only):
        t, off = self._one(text)
        aln, count = find_all_batch([self], t, off, max_dist, MYERS_MAX_HITS, ends_only, ctx=self._ctx)
        if count[0] > MYERS_MAX_HITS:
            raise _lib.BiogpuError(-8, f"{int(count[0])} hits in one text: more than the {MYERS_MAX_HITS} a job reports")
        return aln[:int(count[0])]

    def find_all_end(self, text, max_dist):
        """myers_impl.rs:185-195: [(end, dist)]"""
        return [(int(a["yend"]) - 1, int(a["score"])) for a in self._all(text, max_dist, True)]

    def find_all(self, text, max_dist):
        """myers_impl.rs:214-225, 482-494: [(start, end + 1, dist)]"""
        return [(int(a["ystart"]), int(a["yend"]), int(a["score"])) for a in self._all(text, max_dist, False)]

    def alignments(self, text, max_dist):
        """next_alignment at every hit (myers_impl.rs:400-406): the Alignment fields of update_aln (helpers.rs:83-99) as
        dicts; `operations` is None — the find-all call reports coordinates and distances only, a path exists for the best
        hit alone (best_alignment)"""
        return [_aln_dict(a, None) for a in self._all(text, max_dist, False)]

    def best_alignment(self, text, max_dist=255):
        """the hit find_all(text, max_dist).min_by_key(dist) returns, with its operations; None without a hit"""
        t, off = self._one(text)
        aln, ops = best_batch([self], t, off, max_dist, ops_stride=2 * self.m, ctx=self._ctx)
        if aln["score"][0] == MIN_SCORE:
            return None
        o = ops[int(aln["ops_off"][0]):int(aln["ops_off"][0]) + int(aln["n_ops"][0])]
        return _aln_dict(aln[0], [OPS[int(b)] for b in o])


class MyersLong(Myers):
    """myers::long::Myers::<u64>::new_ambig(pattern, ambigs, wildcards) (long.rs:57-122): `peq` is [blocks][256]"""

    def __init__(self, pattern, ambigs=None, wildcards=None, ctx=None):
        pattern = bytes(pattern)
        if len(pattern) == 0:
            raise ValueError("Pattern is empty")  # long.rs:83
        if len(pattern) > MYERS_LONG_MAX_M:
            raise ValueError(f"Pattern too long: more than the {MYERS_LONG_MAX_M} symbols the device variant takes")
        n_blocks = (len(pattern) + 63) // 64
        peq = [[0] * 256 for _ in range(n_blocks)]
        for i, symbol in enumerate(pattern):  # long.rs:88-103
            block, mask = peq[i // 64], 1 << (i % 64)
            block[symbol] |= mask
            for eq in (ambigs or {}).get(symbol, ()):
                block[eq] |= mask
        for block in peq:  # long.rs:105-109
            for w in wildcards or ():
                block[w] = (1 << 64) - 1
        self.peq = np.array(peq, dtype=np.uint64)
        self.m = len(pattern)
        self._ctx = ctx

    NO_DISTANCE = (1 << 64) - 1 - 64  # impl_myers!'s max_dist, usize::MAX - 64 (long.rs:586): distance() of an empty text

    def _max(self):
        return 0xFFFFFFFF

    def distance(self, text):
        """myers_impl.rs:163-181; usize::MAX - 64 for an empty text"""
        t, off = self._one(text)
        aln, _ = long_best_batch([self], t, off, self._max(), ctx=self._ctx)
        return self.NO_DISTANCE if aln["score"][0] == MIN_SCORE else int(aln["score"][0])

    def find_best_end(self, text):
        t, off = self._one(text)
        aln, _ = long_best_batch([self], t, off, self._max(), ctx=self._ctx)
        if aln["score"][0] == MIN_SCORE:
            raise ValueError("find_best_end: no end column (empty text)")
        return int(aln["yend"][0]) - 1, int(aln["score"][0])

    def _all(self, text, max_dist, ends_only):
        t, off = self._one(text)
        aln, count = long_find_all_batch([self], t, off, max_dist, MYERS_MAX_HITS, ends_only, ctx=self._ctx)
        if count[0] > MYERS_MAX_HITS:
            raise _lib.BiogpuError(-8, f"{int(count[0])} hits in one text: more than the {MYERS_MAX_HITS} a job reports")
        return aln[:int(count[0])]

    def best_alignment(self, text, max_dist=0xFFFFFFFF):
        t, off = self._one(text)
        aln, ops = long_best_batch([self], t, off, max_dist, ops_stride=2 * self.m, ctx=self._ctx)
        if aln["score"][0] == MIN_SCORE:
            return None
        o = ops[int(aln["ops_off"][0]):int(aln["ops_off"][0]) + int(aln["n_ops"][0])]
        return _aln_dict(aln[0], [OPS[int(b)] for b in o])


def _aln_dict(a, operations):
    return {"score": int(a["score"]), "xstart": int(a["xstart"]), "xend": int(a["xend"]), "xlen": int(a["xlen"]),
            "ystart": int(a["ystart"]), "yend": int(a["yend"]), "ylen": int(a["ylen"]), "mode": "Semiglobal", "operations": operations}


class MyersBuilder:
    """myers::MyersBuilder (builder.rs:50-165)"""

    def __init__(self):
        self._ambigs, self._wildcards = {}, []

    def ambig(self, byte, equivalents):  # builder.rs:84-92: repeated calls accumulate
        self._ambigs.setdefault(_byte(byte), []).extend(_byte(e) for e in _iter_bytes(equivalents))
        return self

    def text_wildcard(self, wildcard):  # builder.rs:115-118
        self._wildcards.append(_byte(wildcard))
        return self

    def build_64(self, pattern, ctx=None):  # builder.rs:122-129
        return Myers(pattern, self._ambigs, self._wildcards, ctx)

    def build_long_64(self, pattern, ctx=None):  # builder.rs:169-176
        return MyersLong(pattern, self._ambigs, self._wildcards, ctx)


def _byte(b):
    return b if isinstance(b, int) else bytes(b)[0] if not isinstance(b, str) else ord(b)


def _iter_bytes(e):
    return e.encode() if isinstance(e, str) else e


# ---- batches ---------------------------------------------------------------------------------------------------------
def patterns_array(patterns):
    """bg_myers_pattern_t[n_pat] of Myers objects (or an array already in that layout)"""
    if isinstance(patterns, np.ndarray) and patterns.dtype == MYERS_PATTERN_DTYPE:
        return np.ascontiguousarray(patterns)
    a = np.zeros(len(patterns), dtype=MYERS_PATTERN_DTYPE)
    for i, p in enumerate(patterns):
        a["peq"][i] = p.peq
        a["m"][i] = p.m
    return a


def _raise_unless(rc, where, allow=()):
    if rc != 0 and rc not in allow:
        _lib.check(rc, where)
    return rc


def best_batch(patterns, text, off, max_dist, ops_stride=None, ctx=None, allow_ops_cap=False):
    """bg_myers_best_batch over host arrays: (records[n_texts * n_pat], ops).  Job t * n_pat + p; its operations end at
    (job + 1) * ops_stride.  ops_stride None: no operations.  allow_ops_cap: a path that overflows its slot is reported
    in its record (status -9) instead of raising."""
    ctx = ctx or _lib.default_context()
    pats = patterns_array(patterns)
    text, off = _lib.as_u8(text), np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1
    aln = np.zeros(n * len(pats), dtype=ALN_DTYPE)
    ops = np.zeros(max(1, len(aln) * ops_stride), dtype=np.uint8) if ops_stride is not None else None
    rc = _lib.lib().bg_myers_best_batch(ctx.h, pats.ctypes.data, len(pats), int(max_dist), n, text.ctypes.data, off.ctypes.data,
                                        aln.ctypes.data, ops.ctypes.data if ops is not None else None, ops_stride or 0)
    _raise_unless(rc, "bg_myers_best_batch", (-9,) if allow_ops_cap else ())
    return aln, ops


def find_all_batch(patterns, text, off, max_dist, max_hits, ends_only=False, ctx=None):
    """bg_myers_find_all_batch over host arrays: (records[n_texts * n_pat * max_hits], count[n_texts * n_pat])"""
    ctx = ctx or _lib.default_context()
    pats = patterns_array(patterns)
    text, off = _lib.as_u8(text), np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1
    aln = np.zeros(n * len(pats) * max(0, min(int(max_hits), MYERS_MAX_HITS)), dtype=ALN_DTYPE)
    count = np.zeros(n * len(pats), dtype=np.uint32)
    _lib.check(_lib.lib().bg_myers_find_all_batch(ctx.h, pats.ctypes.data, len(pats), int(max_dist), int(max_hits),
                                                  MYERS_ENDS_ONLY if ends_only else 0, n, text.ctypes.data, off.ctypes.data,
                                                  aln.ctypes.data, count.ctypes.data), "bg_myers_find_all_batch")
    return aln, count


def best_batch_dev(patterns, d_text, d_off, max_dist, ops_stride=None, ctx=None, stream=0, allow_ops_cap=False, out=None):
    """bg_myers_best_batch_dev: d_text uint8, d_off int64 (n_texts + 1) torch tensors on the device.  Returns
    (d_aln uint8[n_jobs * 64], d_ops uint8[n_jobs * ops_stride] or None), left in HBM.  `out`: that pair from an earlier
    call of the same shape, to write into instead of allocating."""
    import torch
    ctx = ctx or _lib.default_context()
    pats = patterns_array(patterns)
    n = int(d_off.numel()) - 1
    if out is not None:
        d_aln, d_ops = out
    else:
        d_aln = torch.empty(n * len(pats) * 64, dtype=torch.uint8, device=d_text.device)
        d_ops = torch.empty(max(1, n * len(pats) * ops_stride), dtype=torch.uint8, device=d_text.device) if ops_stride is not None else None
    rc = _lib.lib().bg_myers_best_batch_dev(ctx.h, pats.ctypes.data, len(pats), int(max_dist), n, d_text.data_ptr(), d_off.data_ptr(),
                                            d_aln.data_ptr(), d_ops.data_ptr() if d_ops is not None else None, ops_stride or 0, stream)
    _raise_unless(rc, "bg_myers_best_batch_dev", (-9,) if allow_ops_cap else ())
    return d_aln, d_ops


def find_all_batch_dev(patterns, d_text, d_off, max_dist, max_hits, ends_only=False, ctx=None, stream=0, out=None):
    """bg_myers_find_all_batch_dev: (d_aln uint8[n_jobs * max_hits * 64], d_count int32[n_jobs]) in HBM; `out` as in
    best_batch_dev"""
    import torch
    ctx = ctx or _lib.default_context()
    pats = patterns_array(patterns)
    n = int(d_off.numel()) - 1
    if out is not None:
        d_aln, d_count = out
    else:
        d_aln = torch.empty(n * len(pats) * max(0, min(int(max_hits), MYERS_MAX_HITS)) * 64, dtype=torch.uint8, device=d_text.device)
        d_count = torch.empty(n * len(pats), dtype=torch.int32, device=d_text.device)
    _lib.check(_lib.lib().bg_myers_find_all_batch_dev(ctx.h, pats.ctypes.data, len(pats), int(max_dist), int(max_hits),
                                                      MYERS_ENDS_ONLY if ends_only else 0, n, d_text.data_ptr(), d_off.data_ptr(),
                                                      d_aln.data_ptr(), d_count.data_ptr(), stream), "bg_myers_find_all_batch_dev")
    return d_aln, d_count


# ---- batches of the block-based variant ------------------------------------------------------------------------------
def long_patterns_array(patterns):
    """(peq uint64[blocks * 256], blk_off uint64[n_pat + 1], m uint32[n_pat]) of MyersLong objects — or of Myers objects, whose
    one table is one block — or such a triple already"""
    if isinstance(patterns, tuple):
        peq, blk_off, m = patterns
        return (np.ascontiguousarray(peq, dtype=np.uint64).reshape(-1), np.ascontiguousarray(blk_off, dtype=np.uint64),
                np.ascontiguousarray(m, dtype=np.uint32))
    blocks = [np.asarray(p.peq, dtype=np.uint64).reshape(-1, 256) for p in patterns]
    blk_off = np.zeros(len(blocks) + 1, dtype=np.uint64)
    blk_off[1:] = np.cumsum([len(b) for b in blocks])
    peq = np.concatenate(blocks).reshape(-1) if blocks else np.zeros(0, dtype=np.uint64)
    return np.ascontiguousarray(peq), blk_off, np.array([p.m for p in patterns], dtype=np.uint32)


def _max_dist(max_dist):
    return max(0, min(int(max_dist), 0xFFFFFFFF))  # the call clamps to each pattern's m anyway


def long_best_batch(patterns, text, off, max_dist, ops_stride=None, ctx=None, allow_ops_cap=False):
    """bg_myers_long_best_batch over host arrays; arguments and results as best_batch"""
    ctx = ctx or _lib.default_context()
    peq, blk_off, m = long_patterns_array(patterns)
    text, off = _lib.as_u8(text), np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1
    aln = np.zeros(n * len(m), dtype=ALN_DTYPE)
    ops = np.zeros(max(1, len(aln) * ops_stride), dtype=np.uint8) if ops_stride is not None else None
    rc = _lib.lib().bg_myers_long_best_batch(ctx.h, peq.ctypes.data, blk_off.ctypes.data, m.ctypes.data, len(m), _max_dist(max_dist), n,
                                             text.ctypes.data, off.ctypes.data, aln.ctypes.data,
                                             ops.ctypes.data if ops is not None else None, ops_stride or 0)
    _raise_unless(rc, "bg_myers_long_best_batch", (-9,) if allow_ops_cap else ())
    return aln, ops


def long_find_all_batch(patterns, text, off, max_dist, max_hits, ends_only=False, ctx=None):
    """bg_myers_long_find_all_batch over host arrays; arguments and results as find_all_batch"""
    ctx = ctx or _lib.default_context()
    peq, blk_off, m = long_patterns_array(patterns)
    text, off = _lib.as_u8(text), np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1
    aln = np.zeros(n * len(m) * max(0, min(int(max_hits), MYERS_MAX_HITS)), dtype=ALN_DTYPE)
    count = np.zeros(n * len(m), dtype=np.uint32)
    _lib.check(_lib.lib().bg_myers_long_find_all_batch(ctx.h, peq.ctypes.data, blk_off.ctypes.data, m.ctypes.data, len(m),
                                                       _max_dist(max_dist), int(max_hits), MYERS_ENDS_ONLY if ends_only else 0, n,
                                                       text.ctypes.data, off.ctypes.data, aln.ctypes.data, count.ctypes.data),
               "bg_myers_long_find_all_batch")
    return aln, count


def long_best_batch_dev(patterns, d_text, d_off, max_dist, ops_stride=None, ctx=None, stream=0, allow_ops_cap=False, out=None):
    """bg_myers_long_best_batch_dev; arguments and results as best_batch_dev"""
    import torch
    ctx = ctx or _lib.default_context()
    peq, blk_off, m = long_patterns_array(patterns)
    n = int(d_off.numel()) - 1
    if out is not None:
        d_aln, d_ops = out
    else:
        d_aln = torch.empty(n * len(m) * 64, dtype=torch.uint8, device=d_text.device)
        d_ops = torch.empty(max(1, n * len(m) * ops_stride), dtype=torch.uint8, device=d_text.device) if ops_stride is not None else None
    rc = _lib.lib().bg_myers_long_best_batch_dev(ctx.h, peq.ctypes.data, blk_off.ctypes.data, m.ctypes.data, len(m), _max_dist(max_dist), n,
                                                 d_text.data_ptr(), d_off.data_ptr(), d_aln.data_ptr(),
                                                 d_ops.data_ptr() if d_ops is not None else None, ops_stride or 0, stream)
    _raise_unless(rc, "bg_myers_long_best_batch_dev", (-9,) if allow_ops_cap else ())
    return d_aln, d_ops


def long_find_all_batch_dev(patterns, d_text, d_off, max_dist, max_hits, ends_only=False, ctx=None, stream=0, out=None):
    """bg_myers_long_find_all_batch_dev; arguments and results as find_all_batch_dev"""
    import torch
    ctx = ctx or _lib.default_context()
    peq, blk_off, m = long_patterns_array(patterns)
    n = int(d_off.numel()) - 1
    if out is not None:
        d_aln, d_count = out
    else:
        d_aln = torch.empty(n * len(m) * max(0, min(int(max_hits), MYERS_MAX_HITS)) * 64, dtype=torch.uint8, device=d_text.device)
        d_count = torch.empty(n * len(m), dtype=torch.int32, device=d_text.device)
    _lib.check(_lib.lib().bg_myers_long_find_all_batch_dev(ctx.h, peq.ctypes.data, blk_off.ctypes.data, m.ctypes.data, len(m),
                                                           _max_dist(max_dist), int(max_hits), MYERS_ENDS_ONLY if ends_only else 0, n,
                                                           d_text.data_ptr(), d_off.data_ptr(), d_aln.data_ptr(), d_count.data_ptr(),
                                                           stream), "bg_myers_long_find_all_batch_dev")
    return d_aln, d_count


def records(d_aln):
    """a device record tensor of the calls above as a host array of bg_alignment_t"""
    return d_aln.cpu().numpy().view(ALN_DTYPE)


# ---- trimming --------------------------------------------------------------------------------------------------------
def trim(mode, hits, n_pat, recs, seq, seq_off, qual, qual_off, ctx=None):
    """bg_fastq_trim over host arrays (the columns of fastq.parse_arrays; hits: records of best_batch, read r's at
    r * n_pat).  Returns (recs, seq, seq_off, qual, qual_off) trimmed and compacted."""
    ctx = ctx or _lib.default_context()
    n = len(recs)
    hits = np.ascontiguousarray(hits, dtype=ALN_DTYPE)
    recs, seq, seq_off, qual, qual_off = _lib.fq_columns(recs, seq, seq_off, qual, qual_off)
    o_recs, o_seq, o_so, o_qual, o_qo = _lib.fq_host_outputs(n, n, seq, qual)
    tot = (C.c_uint64 * 2)()
    _lib.check(_lib.lib().bg_fastq_trim(ctx.h, n, int(mode), hits.ctypes.data, int(n_pat), recs.ctypes.data, seq.ctypes.data,
                                        seq_off.ctypes.data, qual.ctypes.data, qual_off.ctypes.data, o_recs.ctypes.data,
                                        o_seq.ctypes.data, o_so.ctypes.data, o_qual.ctypes.data, o_qo.ctypes.data, tot), "bg_fastq_trim")
    return o_recs, o_seq[:int(tot[0])], o_so, o_qual[:int(tot[1])], o_qo


def trim_dev(mode, d_hits, n_pat, n, d_recs, d_seq, d_seq_off, d_qual, d_qual_off, ctx=None, stream=0, want_totals=True, out=None):
    """bg_fastq_trim_dev on torch device tensors (the outputs of fastq.parse_dev and best_batch_dev).  Returns
    (d_recs, d_seq, d_seq_off, d_qual, d_qual_off, totals) — new tensors in HBM (never the inputs: the call does not work in
    place); totals = (sequence bytes, quality bytes) or None (then the call does not synchronise).  `out`: the five tensors of
    an earlier call of the same shape, to write into instead of allocating."""
    ctx = ctx or _lib.default_context()
    o_recs, o_seq, o_so, o_qual, o_qo = out[:5] if out is not None else _lib.fq_dev_outputs(n, n, d_seq, d_qual)
    tot = (C.c_uint64 * 2)()
    _lib.check(_lib.lib().bg_fastq_trim_dev(ctx.h, n, int(mode), d_hits.data_ptr(), int(n_pat), d_recs.data_ptr(), d_seq.data_ptr(),
                                            d_seq_off.data_ptr(), d_qual.data_ptr(), d_qual_off.data_ptr(), o_recs.data_ptr(),
                                            o_seq.data_ptr(), o_so.data_ptr(), o_qual.data_ptr(), o_qo.data_ptr(),
                                            tot if want_totals else None, stream), "bg_fastq_trim_dev")
    return o_recs, o_seq, o_so, o_qual, o_qo, ((int(tot[0]), int(tot[1])) if want_totals else None)
