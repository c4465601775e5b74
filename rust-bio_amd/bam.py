"""BAM records, BGZF framing and reading, and the BAI index — host mirror of `bg_bam_header`, `bg_bam_emit_batch[_dev]`, `bg_bgzf_frame[_dev]`,
`bg_bgzf_deflate[_dev]`, `bg_bgzf_blocks[_dev]`, `bg_bgzf_inflate[_dev]` and `bg_bam_index[_dev]`; `sorted_bam` chains them with `sam.markdup_*`, `sam.sort_keys_*` and `sam.sort_*` into a complete coordinate-sorted BAM file.

rust-bio has no BAM writer; the record is defined in include/biogpu.h as the BAM encoding (SAM v1.6, section 4.2) of the line
the SAM writer gives a slot and is written by HIP kernels (rust-bio_amd/csrc/bam_emit.hip) out of the same arguments; the
container holds stored deflate blocks with a CRC-32 each (rust-bio_amd/csrc/bgzf.hip) or blocks compressed on the device
(rust-bio_amd/csrc/bgzf_deflate.hip) and is read back by `read_bgzf` (rust-bio_amd/csrc/bgzf_inflate.hip: the block table
of a stream, every block inflated and checked on the device); the index is built from the sorted records and the framing's block table
(rust-bio_amd/csrc/bam_index.hip).  This module only marshals arguments."""
import ctypes as C

import numpy as np

from . import _lib, sam
from ._lib import BGZF_EOF, SAM_SO_COORDINATE, SAM_SO_UNSORTED  # noqa: F401

PAYLOAD = 65280      # bytes of a full block's payload
BLOCK_HEAD = 23      # bytes of a block in front of its payload
BLOCK_EXTRA = 31     # ... and behind it: CRC-32, ISIZE
EOF_BYTES = 28


def header(contigs, sort_order=SAM_SO_UNSORTED):
    """bg_bam_header: "BAM\\1", the text of `sam.header`, the reference table, as bytes (host only)"""
    n = C.c_uint64(0)
    args = (contigs.table.ctypes.data, len(contigs), contigs.names.ctypes.data, sort_order)
    _lib.check(_lib.lib().bg_bam_header(*args, None, 0, C.byref(n)), "bg_bam_header")
    out = np.zeros(max(n.value, 1), dtype=np.uint8)
    _lib.check(_lib.lib().bg_bam_header(*args, out.ctypes.data, n.value, C.byref(n)), "bg_bam_header")
    return out[:n.value].tobytes()


def emit_arrays(fm, params, contigs, parsed, hits, strand, ops, multi=None, pairs=None, dup=None):
    """bg_bam_emit_batch, host buffers: the arguments of `sam.emit_arrays`.  Returns (records: bytes,
    out_off: uint64[n_reads * K + 1]); raises BiogpuError with status -11 (UNSUPPORTED) when a record is not representable."""
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
        return _lib.lib().bg_bam_emit_batch(fm.h, C.byref(pc), n, contigs.table.ctypes.data, len(contigs), contigs.names.ctypes.data,
                                            bufs[0].ctypes.data, recs.ctypes.data, bufs[1].ctypes.data, bufs[2].ctypes.data, hits.ctypes.data,
                                            strand.ctypes.data, bufs[3].ctypes.data, sam._ptr(multi), sam._ptr(pairs),
                                            dup.ctypes.data if dup is not None and n else None, out, cap, out_off.ctypes.data, C.byref(total))
    _lib.check(call(None, 0), "bg_bam_emit_batch")
    out = np.zeros(max(total.value, 1), dtype=np.uint8)
    _lib.check(call(out.ctypes.data, total.value), "bg_bam_emit_batch")
    return out[:total.value].tobytes(), out_off


def emit_dev(fm, params, n_reads, d_contigs, n_contigs, d_names, d_fastq_text, d_recs, d_seq, d_qual, d_hits, d_strand, d_ops,
             d_out, out_cap, d_out_off, d_multi=0, d_pairs=0, stream=0, d_dup=0):
    """bg_bam_emit_batch_dev (pointers are ints; d_multi / d_pairs / d_dup may be 0; d_out = 0 with out_cap = 0 sizes).
    Returns the total number of bytes of the records; raises BiogpuError with status -9 (OPS_CAP) when it exceeds out_cap and
    -11 (UNSUPPORTED) when a record is not representable."""
    total = C.c_uint64(0)
    pc = params.to_c()
    rc = _lib.lib().bg_bam_emit_batch_dev(fm.h, C.byref(pc), n_reads, d_contigs, n_contigs, d_names, d_fastq_text, d_recs, d_seq, d_qual, d_hits,
                                          d_strand, d_ops, d_multi or None, d_pairs or None, d_dup or None, d_out or None, out_cap, d_out_off,
                                          C.byref(total), stream)
    _lib.check(rc, "bg_bam_emit_batch_dev")
    return int(total.value)


def framed_bytes(in_bytes, flags=0):
    """the closed-form size of bg_bgzf_frame's output"""
    return in_bytes + BLOCK_EXTRA * ((in_bytes + PAYLOAD - 1) // PAYLOAD) + (EOF_BYTES if flags & BGZF_EOF else 0)


def bgzf_frame_arrays(data, flags=0, ctx=None):
    """bg_bgzf_frame, host buffers: `data` (bytes or uint8 array) as BGZF blocks, with the end-of-file block under BGZF_EOF"""
    ctx = ctx or _lib.default_context()
    src = _lib.as_u8(data)
    nbytes = len(src)
    src = src if nbytes else np.zeros(1, np.uint8)
    n = C.c_uint64(0)
    _lib.check(_lib.lib().bg_bgzf_frame(ctx.h, src.ctypes.data, nbytes, flags, None, 0, C.byref(n)), "bg_bgzf_frame")
    out = np.zeros(max(n.value, 1), dtype=np.uint8)
    _lib.check(_lib.lib().bg_bgzf_frame(ctx.h, src.ctypes.data, nbytes, flags, out.ctypes.data, n.value, C.byref(n)), "bg_bgzf_frame")
    return out[:n.value].tobytes()


def bgzf_frame_dev(d_in, in_bytes, d_out, out_cap, flags=0, stream=0, ctx=None):
    """bg_bgzf_frame_dev (pointers are ints; asynchronous on `stream`, nothing is read back; d_out = 0 with out_cap = 0 sizes).
    Returns the number of bytes of the framed stream; raises BiogpuError with status -9 (OPS_CAP) when it exceeds out_cap."""
    ctx = ctx or _lib.default_context()
    n = C.c_uint64(0)
    _lib.check(_lib.lib().bg_bgzf_frame_dev(ctx.h, d_in or None, in_bytes, flags, d_out or None, out_cap, C.byref(n), stream), "bg_bgzf_frame_dev")
    return int(n.value)


def bgzf_deflate_arrays(data, flags=0, ctx=None):
    """bg_bgzf_deflate, host buffers: `data` as BGZF blocks with deflate-compressed payloads.  Returns (bytes, block_off:
    uint64[n_blocks + 1], the start of every block in the bytes and the end of the last; the end-of-file block is not counted)"""
    ctx = ctx or _lib.default_context()
    src = _lib.as_u8(data)
    nbytes = len(src)
    src = src if nbytes else np.zeros(1, np.uint8)
    n = C.c_uint64(0)
    _lib.check(_lib.lib().bg_bgzf_deflate(ctx.h, src.ctypes.data, nbytes, flags, None, 0, None, C.byref(n)), "bg_bgzf_deflate")
    out = np.zeros(max(n.value, 1), dtype=np.uint8)
    block_off = np.zeros((nbytes + PAYLOAD - 1) // PAYLOAD + 1, dtype=np.uint64)
    _lib.check(_lib.lib().bg_bgzf_deflate(ctx.h, src.ctypes.data, nbytes, flags, out.ctypes.data, n.value, block_off.ctypes.data, C.byref(n)),
               "bg_bgzf_deflate")
    return out[:n.value].tobytes(), block_off


def bgzf_deflate_dev(d_in, in_bytes, d_out, out_cap, flags=0, stream=0, ctx=None, d_block_off=0):
    """bg_bgzf_deflate_dev (pointers are ints; d_block_off may be 0; d_out = 0 with out_cap = 0 returns the stored bound,
    `framed_bytes`, which out_cap must hold).  Returns the actual number of bytes, read back with one synchronisation of
    `stream`; raises BiogpuError with status -9 (OPS_CAP) when out_cap is below the bound."""
    ctx = ctx or _lib.default_context()
    n = C.c_uint64(0)
    _lib.check(_lib.lib().bg_bgzf_deflate_dev(ctx.h, d_in or None, in_bytes, flags, d_out or None, out_cap, d_block_off or None, C.byref(n), stream),
               "bg_bgzf_deflate_dev")
    return int(n.value)


INFLATE_STATUS = ["ok", "bad block type", "bad stored lengths", "bad code lengths", "bad symbol", "bad distance", "truncated",
                  "trailing bytes", "size", "CRC"]  # BG_INFLATE_*


class BgzfError(_lib.BiogpuError):
    """bg_bgzf_blocks[_dev] or bg_bgzf_inflate[_dev] refused a stream: `block` is the index of the first offending member (None:
    none is to blame), `offset` its file offset where known, `inflate_status` its BG_INFLATE_* status (None: it came from the
    block table or from the call's arguments)"""

    def __init__(self, status, where, block, offset=None, inflate_status=None):
        super().__init__(status, where)
        self.block, self.offset, self.inflate_status = block, offset, inflate_status


def _bad(first_bad):
    return None if first_bad.value == 2**64 - 1 else int(first_bad.value)


def bgzf_blocks_arrays(data, ctx=None):
    """bg_bgzf_blocks, host buffers: the block table of the BGZF stream `data`.  Returns (block_off, out_off), uint64[n_blocks + 1]
    each: the members' starts and `len(data)`; the exclusive prefix sum of their ISIZE fields.  Raises BgzfError (status -1
    INVALID_ARG, -11 UNSUPPORTED) with the index of the first member the chain cannot continue with and its file offset."""
    ctx = ctx or _lib.default_context()
    src = _lib.as_u8(data)
    nbytes = len(src)
    src = src if nbytes else np.zeros(1, np.uint8)
    n, total, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call(block_off, out_off, cap):
        rc = _lib.lib().bg_bgzf_blocks(ctx.h, src.ctypes.data, nbytes, block_off, out_off, cap, C.byref(n), C.byref(total), C.byref(bad))
        if rc != _lib.BG_OK:
            at = 0
            for _ in range(_bad(bad) or 0):  # the members in front of the offending one are good: their BSIZE leads to it
                at += int(src[at + 16]) + (int(src[at + 17]) << 8) + 1
            raise BgzfError(rc, "bg_bgzf_blocks", _bad(bad), None if _bad(bad) is None else at)
    call(None, None, 0)
    block_off, out_off = np.zeros(n.value + 1, np.uint64), np.zeros(n.value + 1, np.uint64)
    call(block_off.ctypes.data, out_off.ctypes.data, n.value)
    return block_off, out_off


def bgzf_blocks_dev(d_in, in_bytes, d_block_off=0, d_out_off=0, cap_blocks=0, stream=0, ctx=None):
    """bg_bgzf_blocks_dev (pointers are ints; both tables 0 with cap_blocks = 0 sizes).  Returns (n_blocks, out_bytes), read back
    with one synchronisation of `stream`; the tables get n_blocks + 1 entries each.  Raises BgzfError as `bgzf_blocks_arrays`
    (`block` only: the tables stay unwritten on an error and the file is in HBM, so `offset` is None),
    BiogpuError with status -9 (OPS_CAP) when cap_blocks is too small."""
    ctx = ctx or _lib.default_context()
    n, total, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = _lib.lib().bg_bgzf_blocks_dev(ctx.h, d_in or None, in_bytes, d_block_off or None, d_out_off or None, cap_blocks, C.byref(n), C.byref(total),
                                       C.byref(bad), stream)
    if rc in (-1, -11):
        raise BgzfError(rc, "bg_bgzf_blocks_dev", _bad(bad))
    _lib.check(rc, "bg_bgzf_blocks_dev")
    return int(n.value), int(total.value)


def bgzf_inflate_arrays(data, block_off, out_off, ctx=None):
    """bg_bgzf_inflate, host buffers: the payloads of the members `block_off` names, each at its `out_off`.  Returns (bytes,
    status: uint8[n_blocks]) when every block is good; raises BgzfError with the lowest bad block, its file offset and its
    BG_INFLATE_* status otherwise."""
    ctx = ctx or _lib.default_context()
    src = _lib.as_u8(data)
    nbytes = len(src)
    src = src if nbytes else np.zeros(1, np.uint8)
    block_off = np.ascontiguousarray(block_off, dtype=np.uint64)
    out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
    n = len(block_off) - 1
    assert n >= 0 and len(out_off) == n + 1
    total = int(out_off[n])
    out, status, bad = np.zeros(max(total, 1), np.uint8), np.zeros(max(n, 1), np.uint8), C.c_uint64(0)
    rc = _lib.lib().bg_bgzf_inflate(ctx.h, src.ctypes.data, nbytes, n, block_off.ctypes.data, out_off.ctypes.data, out.ctypes.data, total,
                                    status.ctypes.data, C.byref(bad))
    if rc == -1:
        b = _bad(bad)
        raise BgzfError(rc, "bg_bgzf_inflate", b, None if b is None else int(block_off[b]), None if b is None or not status[b] else int(status[b]))
    _lib.check(rc, "bg_bgzf_inflate")
    return out[:total].tobytes(), status[:n]


def bgzf_inflate_dev(d_in, in_bytes, n_blocks, d_block_off, d_out_off, d_out, out_cap, d_status=0, stream=0, ctx=None):
    """bg_bgzf_inflate_dev (pointers are ints; d_status may be 0).  One read-back with one synchronisation of `stream`.  Raises
    BgzfError (status -1) with the lowest bad block, or the first offending row of the tables; BiogpuError with status -9
    (OPS_CAP) when out_cap is below out_off[n_blocks].  Good blocks' payloads are written in either case but the last.
    The error carries `block` only: this module holds no device copy routine, so the caller reads d_status[block] (the
    BG_INFLATE_* status; 0 there means the tables were refused) and d_block_off[block] (the file offset) from its own
    buffers.  d_out may be 0 with out_cap = 0 for a stream of empty members."""
    ctx = ctx or _lib.default_context()
    bad = C.c_uint64(0)
    rc = _lib.lib().bg_bgzf_inflate_dev(ctx.h, d_in or None, in_bytes, n_blocks, d_block_off or None, d_out_off or None, d_out or None, out_cap,
                                        d_status or None, C.byref(bad), stream)
    if rc == -1:
        raise BgzfError(rc, "bg_bgzf_inflate_dev", _bad(bad))
    _lib.check(rc, "bg_bgzf_inflate_dev")


def read_bgzf(data, ctx=None):
    """The payload of the BGZF stream `data` (a .bam, a bgzipped .fastq.gz) as bytes: `bgzf_blocks_arrays`, then
    `bgzf_inflate_arrays`"""
    block_off, out_off = bgzf_blocks_arrays(data, ctx=ctx)
    return bgzf_inflate_arrays(data, block_off, out_off, ctx=ctx)[0]


def virtual_offsets(stream_offsets, block_off, base=0):
    """The BGZF virtual offsets of bytes `stream_offsets` of a stream framed by one bg_bgzf_deflate call whose output starts at
    byte `base` of the file and whose block table is `block_off`: (base + block_off[o // 65280]) << 16 | o % 65280, as uint64."""
    o = np.asarray(stream_offsets, dtype=np.uint64)
    block_off = np.asarray(block_off, dtype=np.uint64)
    return ((np.uint64(base) + block_off[(o // np.uint64(PAYLOAD)).astype(np.int64)]) << np.uint64(16)) | (o % np.uint64(PAYLOAD))


def virtual_offset(stream_offset, base=0):
    """The BGZF virtual offset (block start << 16 | offset inside the block's payload) of byte `stream_offset` of a stream
    framed by one bg_bgzf_frame call whose output starts at byte `base` of the file."""
    block, within = divmod(stream_offset, PAYLOAD)
    return ((base + block * (PAYLOAD + BLOCK_EXTRA)) << 16) | within


class BamIndexError(_lib.BiogpuError):
    """bg_bam_index[_dev] refused the records; `first_bad` is the offending slot (None: no slot is to blame)"""

    def __init__(self, status, where, first_bad):
        super().__init__(status, where)
        self.first_bad = first_bad


def _index_check(rc, where, first_bad):
    if rc != _lib.BG_OK:
        raise BamIndexError(rc, where, None if first_bad.value == 2**64 - 1 else int(first_bad.value))


def index_arrays(records, out_off, contigs, block_off=None, base=0, ctx=None):
    """bg_bam_index, host buffers: the bytes of the BAI index of the coordinate-sorted BAM records records[out_off[i] ..
    out_off[i + 1]) (what `sam.sort_arrays` returns for `emit_arrays`' records).  block_off: the table `bgzf_deflate_arrays`
    returned for these records, None where `bgzf_frame_arrays` framed them; base: the file offset of that framing call's first
    block, the length of the framed header.  Raises BamIndexError (status -1 INVALID_ARG, -11 UNSUPPORTED) with the offending slot."""
    ctx = ctx or _lib.default_context()
    off = np.ascontiguousarray(out_off, dtype=np.uint64)
    n = len(off) - 1 if len(off) else 0
    src = _lib.as_u8(records)
    src = src if len(src) else np.zeros(1, np.uint8)
    assert n == 0 or int(off[n]) <= len(src)
    table = np.ascontiguousarray(contigs.table)
    if block_off is not None:
        block_off = np.ascontiguousarray(block_off, dtype=np.uint64)
        assert len(block_off) == ((int(off[n]) if n else 0) + PAYLOAD - 1) // PAYLOAD + 1
    total, bad = C.c_uint64(0), C.c_uint64(0)

    def call(out, cap):
        return _lib.lib().bg_bam_index(ctx.h, n, src.ctypes.data, off.ctypes.data if n else None, table.ctypes.data if len(table) else None,
                                       len(table), block_off.ctypes.data if block_off is not None else None, base, out, cap, C.byref(total),
                                       C.byref(bad))
    _index_check(call(None, 0), "bg_bam_index", bad)
    out = np.zeros(max(total.value, 1), dtype=np.uint8)
    _index_check(call(out.ctypes.data, total.value), "bg_bam_index", bad)
    return out[:total.value].tobytes()


def index_dev(n_slots, d_recs, d_off, d_contigs, n_contigs, d_out, out_cap, d_block_off=0, base=0, stream=0, ctx=None):
    """bg_bam_index_dev (pointers are ints; d_block_off = 0: the stream was framed by bg_bgzf_frame; d_out = 0 with out_cap = 0
    sizes).  Returns the number of bytes of the index, read back with one synchronisation of `stream`; raises BamIndexError with
    the offending slot, BiogpuError with status -9 (OPS_CAP) when the index exceeds out_cap."""
    ctx = ctx or _lib.default_context()
    total, bad = C.c_uint64(0), C.c_uint64(0)
    rc = _lib.lib().bg_bam_index_dev(ctx.h, n_slots, d_recs or None, d_off or None, d_contigs or None, n_contigs, d_block_off or None, base,
                                     d_out or None, out_cap, C.byref(total), C.byref(bad), stream)
    _index_check(rc, "bg_bam_index_dev", bad)
    return int(total.value)


def sorted_bam(fm, params, contigs, parsed, hits, strand, ops, multi=None, pairs=None, markdup=None, ctx=None, compress=False, index=False):
    """The chain on host buffers, as `sam.sorted_sam`: duplicate flags (markdup: a MarkdupParams, or None), BAM records that
    carry them, a key per record, the records in coordinate order.  Returns the complete file as bytes: the header
    (SO:coordinate) framed, then the sorted records framed with the end-of-file block.  compress: both framing calls are
    bg_bgzf_deflate instead of bg_bgzf_frame (the same payloads, compressed).  index: returns (file, bai), bai the bytes of the
    file's BAI index (`index_arrays` on the sorted records, the records' block table and the framed header's length)."""
    dup = None
    if markdup is not None:
        dup, _ = sam.markdup_arrays(markdup, contigs, parsed, hits, strand, ctx=ctx)
    recs, off = emit_arrays(fm, params, contigs, parsed, hits, strand, ops, multi=multi, pairs=pairs, dup=dup)
    key = sam.sort_keys_arrays(params, contigs, len(parsed.recs), hits, strand, ctx=ctx)
    body, body_off, _ = sam.sort_arrays(key, recs, off, ctx=ctx)
    block_off = None
    if compress:
        head = bgzf_deflate_arrays(header(contigs, SAM_SO_COORDINATE), 0, ctx=ctx)[0]
        framed, block_off = bgzf_deflate_arrays(body, BGZF_EOF, ctx=ctx)
    else:
        head = bgzf_frame_arrays(header(contigs, SAM_SO_COORDINATE), 0, ctx=ctx)
        framed = bgzf_frame_arrays(body, BGZF_EOF, ctx=ctx)
    if not index:
        return head + framed
    return head + framed, index_arrays(body, body_off, contigs, block_off=block_off, base=len(head), ctx=ctx)
