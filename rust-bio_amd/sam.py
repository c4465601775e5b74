"""SAM records from seed-and-extend hits — host mirror of `bg_sam_header[_so]`, `bg_sam_emit[_dup]_batch[_dev]`, and of the calls
that turn the records into what the next tool takes: `bg_sam_markdup[_dev]` (a duplicate byte per read), `bg_sam_sort_keys[_dev]`
and `bg_sam_sort[_dev]` (the lines in coordinate order); `sorted_sam` chains them.

rust-bio has no SAM writer; the record is defined in include/biogpu.h from the SAM specification and formatted in HIP kernels
(rust-bio_amd/csrc/sam_emit.hip) out of what `fastq.parse_*` and the `pipeline.seed_extend_*` calls leave behind: FASTQ records,
hits, strands, operations and, where given, the multi and pair records.  This module only marshals arguments."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SAM_PAIRED, SAM_SECONDARY, SAM_SO_COORDINATE, SAM_SO_UNSORTED, SAM_TAG_MD, SAM_TAG_NM  # noqa: F401


class Contigs:
    """bg_sam_contig_t[]: the reference sequences inside the indexed text.  `entries`: (name, start, len) ascending in start."""

    def __init__(self, entries):
        self.table = np.zeros(len(entries), dtype=_lib.SAM_CONTIG_DTYPE)
        names = b""
        for c, (name, start, ln) in enumerate(entries):
            name = name.encode() if isinstance(name, str) else bytes(name)
            self.table[c] = (start, ln, len(names), len(name), 0)
            names += name
        self.names = np.frombuffer(names + b"\0", dtype=np.uint8).copy()  # (never empty: a buffer to point at)

    @classmethod
    def from_arrays(cls, table, names):
        """a table and names buffer that already have the layout (what `fasta.reference_arrays` returns)"""
        self = cls([])
        self.table = np.ascontiguousarray(table, dtype=_lib.SAM_CONTIG_DTYPE)
        self.names = np.concatenate([np.ascontiguousarray(names, dtype=np.uint8), np.zeros(1, np.uint8)])
        return self

    def __len__(self):
        return len(self.table)

    def name(self, c):
        o, n = int(self.table["name_off"][c]), int(self.table["name_len"][c])
        return self.names[o:o + n].tobytes()


class SamParams:
    """bg_sam_params_t: flags (SAM_PAIRED | SAM_SECONDARY | SAM_TAG_NM | SAM_TAG_MD) and max_hits, the K slots per read of
    hits / strand (1 after the strands and pairs calls)."""

    def __init__(self, flags=0, max_hits=1):
        self.flags, self.max_hits = flags, max_hits

    def to_c(self):
        return _lib.SAM_PARAMS(self.flags, self.max_hits)


class MarkdupParams:
    """bg_markdup_params_t: flags (SAM_PAIRED or 0), max_hits (K of hits / strand; only slot K r of read r takes part), the
    quality encoding's offset and the quality below which a symbol does not count towards a read's score."""

    def __init__(self, flags=0, max_hits=1, phred_offset=33, min_qual=15):
        self.flags, self.max_hits, self.phred_offset, self.min_qual = flags, max_hits, phred_offset, min_qual

    def to_c(self):
        p = np.zeros(1, dtype=_lib.MARKDUP_PARAMS_DTYPE)
        p[0] = (self.flags, self.max_hits, self.phred_offset, self.min_qual)
        return p


def header(contigs, sort_order=SAM_SO_UNSORTED):
    """bg_sam_header_so: the @HD, @SQ and @PG lines as bytes (host only); sort_order SAM_SO_UNSORTED (bg_sam_header's bytes) or
    SAM_SO_COORDINATE."""
    n = C.c_uint64(0)
    args = (contigs.table.ctypes.data, len(contigs), contigs.names.ctypes.data, sort_order)
    _lib.check(_lib.lib().bg_sam_header_so(*args, None, 0, C.byref(n)), "bg_sam_header_so")
    out = np.zeros(max(n.value, 1), dtype=np.uint8)
    _lib.check(_lib.lib().bg_sam_header_so(*args, out.ctypes.data, n.value, C.byref(n)), "bg_sam_header_so")
    return out[:n.value].tobytes()


def _ptr(a):
    return a.ctypes.data if a is not None else None


def markdup_arrays(params, contigs, parsed, hits, strand, ctx=None):
    """bg_sam_markdup, host buffers: `parsed` has recs and qual, hits / strand n_reads * K entries.  Returns
    (dup: uint8[n_reads], counts: [reads with an end, reads flagged, pairs flagged, fragments flagged by a pair's end])."""
    ctx = ctx or _lib.default_context()
    n = len(parsed.recs)
    hits = np.ascontiguousarray(hits).reshape(-1)
    strand = np.ascontiguousarray(strand, dtype=np.uint8).reshape(-1)
    qual = np.ascontiguousarray(parsed.qual) if len(parsed.qual) else np.zeros(1, np.uint8)
    recs = np.ascontiguousarray(parsed.recs)
    dup = np.zeros(max(n, 1), dtype=np.uint8)
    counts = np.zeros(4, dtype=np.uint64)
    pc = params.to_c()
    _lib.check(_lib.lib().bg_sam_markdup(ctx.h, pc.ctypes.data, n, contigs.table.ctypes.data, len(contigs), hits.ctypes.data, strand.ctypes.data,
                                         recs.ctypes.data, qual.ctypes.data, dup.ctypes.data, counts.ctypes.data), "bg_sam_markdup")
    return dup[:n], [int(c) for c in counts]


def markdup_dev(params, n_reads, d_contigs, n_contigs, d_hits, d_strand, d_recs, d_qual, d_dup, stream=0, ctx=None):
    """bg_sam_markdup_dev (pointers are ints): fills d_dup (n_reads bytes) and returns the four counts (one synchronisation)."""
    ctx = ctx or _lib.default_context()
    counts = np.zeros(4, dtype=np.uint64)
    pc = params.to_c()
    _lib.check(_lib.lib().bg_sam_markdup_dev(ctx.h, pc.ctypes.data, n_reads, d_contigs, n_contigs, d_hits, d_strand, d_recs, d_qual, d_dup,
                                             counts.ctypes.data, stream), "bg_sam_markdup_dev")
    return [int(c) for c in counts]


def sort_keys_arrays(params, contigs, n_reads, hits, strand, ctx=None):
    """bg_sam_sort_keys, host buffers: uint64[n_reads * K], ref_start of the line's RNAME / POS or 2^64 - 1."""
    ctx = ctx or _lib.default_context()
    hits = np.ascontiguousarray(hits).reshape(-1)
    strand = np.ascontiguousarray(strand, dtype=np.uint8).reshape(-1)
    key = np.zeros(max(n_reads * max(params.max_hits, 1), 1), dtype=np.uint64)
    pc = params.to_c()
    _lib.check(_lib.lib().bg_sam_sort_keys(ctx.h, C.byref(pc), n_reads, contigs.table.ctypes.data, len(contigs), hits.ctypes.data,
                                           strand.ctypes.data, key.ctypes.data), "bg_sam_sort_keys")
    return key[:n_reads * params.max_hits]


def sort_keys_dev(params, n_reads, d_contigs, n_contigs, d_hits, d_strand, d_key, stream=0, ctx=None):
    """bg_sam_sort_keys_dev (pointers are ints; asynchronous on `stream`)"""
    ctx = ctx or _lib.default_context()
    pc = params.to_c()
    _lib.check(_lib.lib().bg_sam_sort_keys_dev(ctx.h, C.byref(pc), n_reads, d_contigs, n_contigs, d_hits, d_strand, d_key, stream),
               "bg_sam_sort_keys_dev")


def sort_arrays(key, text, off, ctx=None):
    """bg_sam_sort, host buffers: records text[off[i] .. off[i + 1]) in the stable ascending order of key.  Returns
    (text: bytes, out_off: uint64[n + 1], perm: uint64[n]).  Knows nothing of SAM: any variable-length records."""
    ctx = ctx or _lib.default_context()
    key = np.ascontiguousarray(key, dtype=np.uint64)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(key)
    src = _lib.as_u8(text)
    nbytes = len(src)
    src = src if nbytes else np.zeros(1, np.uint8)
    out = np.zeros(max(nbytes, 1), dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    perm = np.zeros(max(n, 1), dtype=np.uint64)
    _lib.check(_lib.lib().bg_sam_sort(ctx.h, n, key.ctypes.data if n else None, src.ctypes.data, off.ctypes.data, nbytes, out.ctypes.data,
                                      nbytes, out_off.ctypes.data, perm.ctypes.data), "bg_sam_sort")
    return out[:nbytes].tobytes(), out_off, perm[:n]


def sort_dev(n_slots, d_key, d_in, d_in_off, in_bytes, d_out, out_cap, d_out_off, d_perm, stream=0, ctx=None):
    """bg_sam_sort_dev (pointers are ints; asynchronous on `stream`, nothing is read back); raises BiogpuError with status -9
    (OPS_CAP) when out_cap < in_bytes."""
    ctx = ctx or _lib.default_context()
    _lib.check(_lib.lib().bg_sam_sort_dev(ctx.h, n_slots, d_key or None, d_in or None, d_in_off or None, in_bytes, d_out or None, out_cap,
                                          d_out_off, d_perm, stream), "bg_sam_sort_dev")


def sorted_sam(fm, params, contigs, parsed, hits, strand, ops, multi=None, pairs=None, markdup=None, ctx=None):
    """The chain on host buffers: duplicate flags (markdup: a MarkdupParams, or None for no flags), SAM text that carries them,
    a key per line, the lines in coordinate order.  Returns the header (SO:coordinate) plus the sorted body, as bytes."""
    dup = None
    if markdup is not None:
        dup, _ = markdup_arrays(markdup, contigs, parsed, hits, strand, ctx=ctx)
    text, off = emit_arrays(fm, params, contigs, parsed, hits, strand, ops, multi=multi, pairs=pairs, dup=dup)
    key = sort_keys_arrays(params, contigs, len(parsed.recs), hits, strand, ctx=ctx)
    body, _, _ = sort_arrays(key, text, off, ctx=ctx)
    return header(contigs, SAM_SO_COORDINATE) + body


def emit_arrays(fm, params, contigs, parsed, hits, strand, ops, multi=None, pairs=None, dup=None):
    """bg_sam_emit_batch, host buffers: `parsed` is a fastq.Parsed (text, recs, seq, qual), hits / strand / ops / multi / pairs
    what the host seed-extend calls returned for its reads; dup (optional, uint8[n_reads], bg_sam_emit_dup_batch): the placed
    lines of read r carry 0x400 where dup[r] != 0.  Returns (text: bytes, out_off: uint64[n_reads * K + 1])."""
    n = len(parsed.recs)
    hits = np.ascontiguousarray(hits).reshape(-1)
    strand = np.ascontiguousarray(strand, dtype=np.uint8).reshape(-1)
    bufs = [np.ascontiguousarray(x) if len(x) else np.zeros(1, np.uint8) for x in (parsed.text, parsed.seq, parsed.qual, ops)]
    recs = np.ascontiguousarray(parsed.recs)
    out_off = np.zeros(n * max(params.max_hits, 1) + 1, dtype=np.uint64)
    total = C.c_uint64(0)
    pc = params.to_c()

    if dup is not None:
        dup = np.ascontiguousarray(dup, dtype=np.uint8)
        assert len(dup) == n

    def call(out, cap):
        front = (fm.h, C.byref(pc), n, contigs.table.ctypes.data, len(contigs), contigs.names.ctypes.data, bufs[0].ctypes.data,
                 recs.ctypes.data, bufs[1].ctypes.data, bufs[2].ctypes.data, hits.ctypes.data, strand.ctypes.data, bufs[3].ctypes.data,
                 _ptr(multi), _ptr(pairs))
        back = (out, cap, out_off.ctypes.data, C.byref(total))
        if dup is None:
            return _lib.lib().bg_sam_emit_batch(*front, *back)
        return _lib.lib().bg_sam_emit_dup_batch(*front, dup.ctypes.data if n else None, *back)
    _lib.check(call(None, 0), "bg_sam_emit_batch")
    out = np.zeros(max(total.value, 1), dtype=np.uint8)
    _lib.check(call(out.ctypes.data, total.value), "bg_sam_emit_batch")
    return out[:total.value].tobytes(), out_off


def emit_dev(fm, params, n_reads, d_contigs, n_contigs, d_names, d_fastq_text, d_recs, d_seq, d_qual, d_hits, d_strand, d_ops,
             d_out, out_cap, d_out_off, d_multi=0, d_pairs=0, stream=0, d_dup=0):
    """bg_sam_emit_batch_dev (pointers are ints; d_multi / d_pairs may be 0; d_out = 0 with out_cap = 0 sizes), or, with d_dup
    (n_reads bytes on the device), bg_sam_emit_dup_batch_dev.  Returns the total number of bytes of the lines; raises
    BiogpuError with status -9 (OPS_CAP) when it exceeds out_cap."""
    total = C.c_uint64(0)
    pc = params.to_c()
    front = (fm.h, C.byref(pc), n_reads, d_contigs, n_contigs, d_names, d_fastq_text, d_recs, d_seq, d_qual, d_hits, d_strand, d_ops,
             d_multi or None, d_pairs or None)
    back = (d_out or None, out_cap, d_out_off, C.byref(total), stream)
    if d_dup:
        rc = _lib.lib().bg_sam_emit_dup_batch_dev(*front, d_dup, *back)
    else:
        rc = _lib.lib().bg_sam_emit_batch_dev(*front, *back)
    _lib.check(rc, "bg_sam_emit_batch_dev")
    return int(total.value)
