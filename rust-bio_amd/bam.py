"""BAM records, BGZF framing and reading, and the BAI index — host mirror of `bg_bam_header`, `bg_bam_emit_batch[_dev]`, `bg_bgzf_frame[_dev]`,
`bg_bgzf_deflate[_dev]`, `bg_bgzf_blocks[_dev]`, `bg_bgzf_inflate[_dev]`, `bg_bam_index[_dev]` and of reading BAM back (`bg_bam_header_parse`, `bg_bam_records[_dev]`, `bg_bam_reads[_dev]`, `bg_bam_sort_keys[_dev]`, `bg_bam_index_blocks[_dev]`; rust-bio_amd/csrc/bam_read.hip) and of the pileup over sorted records, its candidate variant sites and its indel events (`bg_bam_pileup[_dev]`, `bg_bam_sites[_dev]`, `bg_bam_indels[_dev]`, `bg_bam_indels_left[_dev]`; rust-bio_amd/csrc/bam_pileup.hip, bam_sites.hip, bam_indels.hip); `sorted_bam` chains them with `sam.markdup_*`, `sam.sort_keys_*` and `sam.sort_*` into a complete coordinate-sorted BAM file.

rust-bio has no BAM writer; the record is defined in include/biogpu.h as the BAM encoding (SAM v1.6, section 4.2) of the line
the SAM writer gives a slot and is written by HIP kernels (rust-bio_amd/csrc/bam_emit.hip) out of the same arguments; the
container holds stored deflate blocks with a CRC-32 each (rust-bio_amd/csrc/bgzf.hip) or blocks compressed on the device
(rust-bio_amd/csrc/bgzf_deflate.hip) and is read back by `read_bgzf` (rust-bio_amd/csrc/bgzf_inflate.hip: the block table
of a stream, every block inflated and checked on the device); the index is built from the sorted records and the framing's block table
(rust-bio_amd/csrc/bam_index.hip).  This module only marshals arguments."""
import ctypes as C
import zlib

import numpy as np

from . import _lib, sam
from ._lib import BAM_READS_ORIGINAL, BGZF_EOF, SAM_SO_COORDINATE, SAM_SO_UNSORTED  # noqa: F401

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


def index_blocks_arrays(stream, off, contigs, block_off, out_off, ctx=None):
    """bg_bam_index_blocks, host buffers: `index_arrays` for a stream in any framing.  `stream` is the whole uncompressed stream,
    `off` the absolute record table (`records_arrays`), block_off / out_off the tables `bgzf_blocks_arrays` gave for the file."""
    ctx = ctx or _lib.default_context()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1 if len(off) else 0
    src = _lib.as_u8(stream)
    src = src if len(src) else np.zeros(1, np.uint8)
    table = np.ascontiguousarray(contigs.table)
    block_off, out_off = np.ascontiguousarray(block_off, dtype=np.uint64), np.ascontiguousarray(out_off, dtype=np.uint64)
    assert len(block_off) == len(out_off) >= 1
    total, bad = C.c_uint64(0), C.c_uint64(0)

    def call(out, cap):
        return _lib.lib().bg_bam_index_blocks(ctx.h, n, src.ctypes.data, off.ctypes.data if n else None, table.ctypes.data if len(table) else None,
                                              len(table), len(block_off) - 1, block_off.ctypes.data, out_off.ctypes.data, out, cap, C.byref(total),
                                              C.byref(bad))
    _index_check(call(None, 0), "bg_bam_index_blocks", bad)
    out = np.zeros(max(total.value, 1), dtype=np.uint8)
    _index_check(call(out.ctypes.data, total.value), "bg_bam_index_blocks", bad)
    return out[:total.value].tobytes()


def index_blocks_dev(n_slots, d_stream, d_off, d_contigs, n_contigs, n_blocks, d_block_off, d_out_off, d_out, out_cap, stream=0, ctx=None):
    """bg_bam_index_blocks_dev (pointers are ints; d_out = 0 with out_cap = 0 sizes).  Returns the number of bytes of the index;
    raises BamIndexError with the offending slot, BiogpuError with status -9 (OPS_CAP) when the index exceeds out_cap."""
    ctx = ctx or _lib.default_context()
    total, bad = C.c_uint64(0), C.c_uint64(0)
    rc = _lib.lib().bg_bam_index_blocks_dev(ctx.h, n_slots, d_stream or None, d_off or None, d_contigs or None, n_contigs, n_blocks, d_block_off or None,
                                            d_out_off or None, d_out or None, out_cap, C.byref(total), C.byref(bad), stream)
    _index_check(rc, "bg_bam_index_blocks_dev", bad)
    return int(total.value)


# ---- reading BAM ------------------------------------------------------------------------------------------------------------
class BamReadError(_lib.BiogpuError):
    """bg_bam_header_parse, bg_bam_records[_dev], bg_bam_reads[_dev] or bg_bam_sort_keys[_dev] refused a stream: `record` is the
    index of the first offending record or slot (None: none is to blame), `offset` its offset in the stream where known"""

    def __init__(self, status, where, record, offset=None):
        super().__init__(status, where)
        self.record, self.offset = record, offset


def read_header(fetch, first=65536):
    """bg_bam_header_parse on a growing prefix.  `fetch(n)` returns (at most) the first n bytes of the uncompressed stream —
    bytes, or a function over a device buffer; each round asks for at least twice the previous prefix, so a long reference
    list costs a logarithmic number of copies.  `fetch` may also be the bytes themselves.  Returns (text: bytes, contigs:
    sam.Contigs with start = sum of (len + 1) over the contigs in front, body_off)."""
    if not callable(fetch):
        data = fetch
        fetch = lambda n: data[:n]  # noqa: E731
    want = first
    out = [C.c_uint64(0) for _ in range(6)]  # n_contigs, names_bytes, text_off, text_len, body_off, need
    refs = [C.byref(x) for x in out]
    while True:
        pre = _lib.as_u8(fetch(want))
        buf = pre if len(pre) else np.zeros(1, np.uint8)
        rc = _lib.lib().bg_bam_header_parse(buf.ctypes.data, len(pre), None, 0, None, 0, *refs)
        if rc == -9 and out[5].value > len(pre) and len(pre) >= want:  # the prefix ends inside the header, and there may be more
            want = max(int(out[5].value), 2 * want)
            continue
        if rc != _lib.BG_OK:
            raise BamReadError(rc, "bg_bam_header_parse", None)
        break
    table = np.zeros(out[0].value, dtype=_lib.SAM_CONTIG_DTYPE)
    names = np.zeros(out[1].value + 1, dtype=np.uint8)
    rc = _lib.lib().bg_bam_header_parse(buf.ctypes.data, len(pre), table.ctypes.data if len(table) else None, len(table),
                                        names.ctypes.data if len(table) else None, out[1].value if len(table) else 0, *refs)
    if rc != _lib.BG_OK:
        raise BamReadError(rc, "bg_bam_header_parse", None)
    contigs = sam.Contigs.from_arrays(table, names[:out[1].value])
    return buf[out[2].value:out[2].value + out[3].value].tobytes(), contigs, int(out[4].value)


def _read_check(rc, where, bad, off=None):
    if rc in (-1,):
        b = _bad(bad)
        raise BamReadError(rc, where, b, None if b is None or off is None else int(off[b]))
    _lib.check(rc, where)


def records_arrays(stream, body_off, n_ref, ctx=None, candidates=False):
    """bg_bam_records, host buffers: the record table of the uncompressed BAM stream `stream`: uint64[n_records + 1], absolute
    offsets, off[0] = body_off, off[-1] = len(stream).  Raises BamReadError with the number of records in front of what is no
    record.  candidates: returns (off, n_candidates)."""
    ctx = ctx or _lib.default_context()
    src = _lib.as_u8(stream)
    nbytes = len(src)
    src = src if nbytes else np.zeros(1, np.uint8)
    n, cand, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _read_check(_lib.lib().bg_bam_records(ctx.h, src.ctypes.data, nbytes, body_off, n_ref, None, 0, C.byref(n), C.byref(cand), C.byref(bad)),
                "bg_bam_records", bad)
    off = np.zeros(n.value + 1, np.uint64)
    _read_check(_lib.lib().bg_bam_records(ctx.h, src.ctypes.data, nbytes, body_off, n_ref, off.ctypes.data, n.value, C.byref(n), C.byref(cand),
                                          C.byref(bad)), "bg_bam_records", bad)
    return (off, int(cand.value)) if candidates else off


def records_dev(d_bam, in_bytes, body_off, n_ref, d_off=0, cap_records=0, stream=0, ctx=None):
    """bg_bam_records_dev (pointers are ints; d_off = 0 with cap_records = 0 sizes).  Returns (n_records, n_candidates), read back
    with two synchronisations of `stream`; d_off gets n_records + 1 entries.  Raises BamReadError (`record`: the records in
    front of the offending position), BiogpuError with status -9 (OPS_CAP) when cap_records is too small."""
    ctx = ctx or _lib.default_context()
    n, cand, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = _lib.lib().bg_bam_records_dev(ctx.h, d_bam or None, in_bytes, body_off, n_ref, d_off or None, cap_records, C.byref(n), C.byref(cand),
                                       C.byref(bad), stream)
    _read_check(rc, "bg_bam_records_dev", bad)
    return int(n.value), int(cand.value)


def reads_params(flags=0, require=0, exclude=0):
    return _lib.BAM_READS(flags, require, exclude)


def reads_arrays(stream, off, n_ref, flags=0, require=0, exclude=0, ctx=None):
    """bg_bam_reads, host buffers: the kept records of the table `off` as the five FASTQ columns.  Returns (recs: FQREC_DTYPE[],
    seq, seq_off, qual, qual_off, src: uint64[], the record of every read); id_off points into `stream`."""
    ctx = ctx or _lib.default_context()
    src_b = _lib.as_u8(stream)
    src_b = src_b if len(src_b) else np.zeros(1, np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1 if len(off) else 0
    prm = reads_params(flags, require, exclude)
    k, sb, qb, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    tail = (C.byref(k), C.byref(sb), C.byref(qb), C.byref(bad))
    head = (ctx.h, C.byref(prm), n, src_b.ctypes.data, off.ctypes.data if n else None, n_ref)
    _read_check(_lib.lib().bg_bam_reads(*head, None, 0, None, 0, None, None, 0, None, None, *tail), "bg_bam_reads", bad, off)
    recs = np.zeros(max(k.value, 1), dtype=_lib.FQREC_DTYPE)
    seq, qual = np.zeros(max(sb.value, 1), np.uint8), np.zeros(max(qb.value, 1), np.uint8)
    seq_off, qual_off, src = np.zeros(k.value + 1, np.uint64), np.zeros(k.value + 1, np.uint64), np.zeros(max(k.value, 1), np.uint64)
    _read_check(_lib.lib().bg_bam_reads(*head, recs.ctypes.data, k.value, seq.ctypes.data, sb.value, seq_off.ctypes.data, qual.ctypes.data, qb.value,
                                        qual_off.ctypes.data, src.ctypes.data, *tail), "bg_bam_reads", bad, off)
    return recs[:k.value], seq[:sb.value], seq_off, qual[:qb.value], qual_off, src[:k.value]


def reads_dev(n_records, d_bam, d_off, n_ref, d_recs=0, cap_reads=0, d_seq=0, seq_cap=0, d_seq_off=0, d_qual=0, qual_cap=0, d_qual_off=0, d_src=0,
              flags=0, require=0, exclude=0, stream=0, ctx=None):
    """bg_bam_reads_dev (pointers are ints; every output 0 with caps 0 sizes; d_src may be 0).  Returns (n_reads, seq_bytes,
    qual_bytes), read back with one synchronisation of `stream`; the columns are then written asynchronously.  Raises
    BamReadError with the first slot that is no record, BiogpuError with status -9 (OPS_CAP) when a cap is too small."""
    ctx = ctx or _lib.default_context()
    prm = reads_params(flags, require, exclude)
    k, sb, qb, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = _lib.lib().bg_bam_reads_dev(ctx.h, C.byref(prm), n_records, d_bam or None, d_off or None, n_ref, d_recs or None, cap_reads, d_seq or None, seq_cap,
                                     d_seq_off or None, d_qual or None, qual_cap, d_qual_off or None, d_src or None, C.byref(k), C.byref(sb), C.byref(qb),
                                     C.byref(bad), stream)
    _read_check(rc, "bg_bam_reads_dev", bad)
    return int(k.value), int(sb.value), int(qb.value)


def sort_keys_records_arrays(stream, off, contigs, ctx=None):
    """bg_bam_sort_keys, host buffers: uint64[n_records], contigs.start[refID] + pos, 2^64 - 1 for a record without a position
    and for an empty slot: what `sam.sort_arrays` takes as `key` with (stream, off)"""
    ctx = ctx or _lib.default_context()
    src = _lib.as_u8(stream)
    src = src if len(src) else np.zeros(1, np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1 if len(off) else 0
    table = np.ascontiguousarray(contigs.table)
    key, bad = np.zeros(max(n, 1), np.uint64), C.c_uint64(0)
    rc = _lib.lib().bg_bam_sort_keys(ctx.h, n, src.ctypes.data, off.ctypes.data if n else None, table.ctypes.data if len(table) else None, len(table),
                                     key.ctypes.data, C.byref(bad))
    _read_check(rc, "bg_bam_sort_keys", bad, off)
    return key[:n]


def sort_keys_records_dev(n_records, d_bam, d_off, d_contigs, n_contigs, d_key, stream=0, ctx=None):
    """bg_bam_sort_keys_dev (pointers are ints); one synchronisation of `stream`.  Raises BamReadError with the first bad slot."""
    ctx = ctx or _lib.default_context()
    bad = C.c_uint64(0)
    rc = _lib.lib().bg_bam_sort_keys_dev(ctx.h, n_records, d_bam or None, d_off or None, d_contigs or None, n_contigs, d_key or None, C.byref(bad), stream)
    _read_check(rc, "bg_bam_sort_keys_dev", bad)


def read_bam(data, ctx=None):
    """A BAM file (bytes) in one call: block table, inflate, header, record table.  Returns (text: the SAM header text, contigs:
    sam.Contigs, stream: the uncompressed bytes, off: uint64[n_records + 1], absolute offsets into `stream`)."""
    stream = read_bgzf(data, ctx=ctx)
    text, contigs, body_off = read_header(stream)
    return text, contigs, stream, records_arrays(stream, body_off, len(contigs), ctx=ctx)


def index_bam(data, ctx=None):
    """The bytes of the .bai of the coordinate-sorted BAM file `data`, whatever wrote it: `bgzf_blocks_arrays`, `read_bgzf`'s
    inflate, `read_header`, `records_arrays`, `index_blocks_arrays`."""
    block_off, out_off = bgzf_blocks_arrays(data, ctx=ctx)
    stream = bgzf_inflate_arrays(data, block_off, out_off, ctx=ctx)[0]
    _, contigs, body_off = read_header(stream)
    off = records_arrays(stream, body_off, len(contigs), ctx=ctx)
    return index_blocks_arrays(stream, off, contigs, block_off, out_off, ctx=ctx)


# ---- pileup ------------------------------------------------------------------------------------------------------------------
PILEUP_TILE = _lib.PILEUP_TILE  # BG_PILEUP_TILE: the positions one workgroup counts; results do not depend on it
PILEUP_STRANDS = _lib.PILEUP_STRANDS
PILEUP_A, PILEUP_C, PILEUP_G, PILEUP_T, PILEUP_OTHER = _lib.PILEUP_A, _lib.PILEUP_C, _lib.PILEUP_G, _lib.PILEUP_T, _lib.PILEUP_OTHER
PILEUP_DEL, PILEUP_SKIP, PILEUP_INS, PILEUP_COLS = _lib.PILEUP_DEL, _lib.PILEUP_SKIP, _lib.PILEUP_INS, _lib.PILEUP_COLS


class BamPileupError(_lib.BiogpuError):
    """bg_bam_pileup[_dev] refused the records or the regions: `slot` is the first offending slot (None: no slot is to blame)"""

    def __init__(self, status, where, slot):
        super().__init__(status, where)
        self.slot = slot


def _pileup_check(rc, where, bad):
    if rc in (-1, -11):
        raise BamPileupError(rc, where, _bad(bad))
    _lib.check(rc, where)


def pileup_params(flags=0, require=0, exclude=0x704, min_mapq=0, min_baseq=0):
    """bg_bam_pileup_t.  The default `exclude` drops secondary alignments, QC failures and duplicates (and unmapped records,
    which are never kept)."""
    p = np.zeros(1, dtype=_lib.BAM_PILEUP_DTYPE)
    p[0] = (flags, require, exclude, min_mapq, min_baseq, 0)
    return p


def pileup_regions(regions):
    """(ref, beg, end) triples, 0-based and half-open, as bg_bam_region_t[]"""
    if isinstance(regions, np.ndarray) and regions.dtype == _lib.BAM_REGION_DTYPE:
        return np.ascontiguousarray(regions)
    out = np.zeros(len(regions), dtype=_lib.BAM_REGION_DTYPE)
    for k, (ref, beg, end) in enumerate(regions):
        out[k] = (ref, beg, end)
    return out


def pileup_arrays(stream, off, contigs, regions, flags=0, require=0, exclude=0x704, min_mapq=0, min_baseq=0, ctx=None):
    """bg_bam_pileup, host buffers: the counters of every position of `regions` ((ref, beg, end), 0-based, half-open) from the
    coordinate-sorted records stream[off[i] .. off[i + 1]).  Returns (rows: uint32[n_rows, W], W = 16 under PILEUP_STRANDS and
    8 otherwise, columns PILEUP_A .. PILEUP_INS; row_off: uint64[n_regions + 1]): position p of region r is
    rows[row_off[r] + p - beg].  Raises BamPileupError (status -1 INVALID_ARG, -11 UNSUPPORTED) with the offending slot."""
    ctx = ctx or _lib.default_context()
    src = _lib.as_u8(stream)
    src = src if len(src) else np.zeros(1, np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1 if len(off) else 0
    table = np.ascontiguousarray(contigs.table)
    reg = pileup_regions(regions)
    prm = pileup_params(flags, require, exclude, min_mapq, min_baseq)
    w = 2 * PILEUP_COLS if flags & PILEUP_STRANDS else PILEUP_COLS
    total, bad = C.c_uint64(0), C.c_uint64(0)

    def call(rows, cap, row_off):
        return _lib.lib().bg_bam_pileup(ctx.h, prm.ctypes.data, n, src.ctypes.data, off.ctypes.data if n else None, table.ctypes.data if len(table) else None,
                                        len(table), reg.ctypes.data if len(reg) else None, len(reg), rows, cap, row_off, C.byref(total), C.byref(bad))
    _pileup_check(call(None, 0, None), "bg_bam_pileup", bad)
    rows = np.zeros((max(total.value, 1), w), dtype=np.uint32)
    row_off = np.zeros(len(reg) + 1, dtype=np.uint64)
    _pileup_check(call(rows.ctypes.data, total.value, row_off.ctypes.data), "bg_bam_pileup", bad)
    return rows[:total.value], row_off


def pileup_dev(n_slots, d_recs, d_off, d_contigs, n_contigs, d_regions, n_regions, d_rows=0, rows_cap=0, d_row_off=0, flags=0, require=0, exclude=0x704,
               min_mapq=0, min_baseq=0, stream=0, ctx=None):
    """bg_bam_pileup_dev (pointers are ints; d_rows = 0 with rows_cap = 0 sizes; d_row_off may be 0; rows_cap counts rows).
    Returns n_rows, read back with one synchronisation of `stream`; the rows are then written asynchronously.  Raises
    BamPileupError with the offending slot, BiogpuError with status -9 (OPS_CAP) when rows_cap is too small."""
    ctx = ctx or _lib.default_context()
    prm = pileup_params(flags, require, exclude, min_mapq, min_baseq)
    total, bad = C.c_uint64(0), C.c_uint64(0)
    rc = _lib.lib().bg_bam_pileup_dev(ctx.h, prm.ctypes.data, n_slots, d_recs or None, d_off or None, d_contigs or None, n_contigs, d_regions or None,
                                      n_regions, d_rows or None, rows_cap, d_row_off or None, C.byref(total), C.byref(bad), stream)
    _pileup_check(rc, "bg_bam_pileup_dev", bad)
    return int(total.value)


def resolve_regions(contigs, regions):
    """regions given as (name or index, beg, end) against a contig table: bg_bam_region_t[].  Raises ValueError naming the
    region for an unknown name, an index outside the table, or an interval that is not 0 <= beg <= end <= the contig's length."""
    names = {contigs.name(c): c for c in reversed(range(len(contigs)))}
    out = np.zeros(len(regions), dtype=_lib.BAM_REGION_DTYPE)
    for k, region in enumerate(regions):
        ref, beg, end = region
        if isinstance(ref, (str, bytes)):
            c = names.get(ref.encode() if isinstance(ref, str) else bytes(ref))
            if c is None:
                raise ValueError(f"region {region!r}: the header names no such reference")
        else:
            c = int(ref)
            if not 0 <= c < len(contigs):
                raise ValueError(f"region {region!r}: no reference of that index")
        if not 0 <= beg <= end <= int(contigs.table["len"][c]):
            raise ValueError(f"region {region!r}: not 0 <= beg <= end <= {int(contigs.table['len'][c])}")
        out[k] = (c, beg, end)
    return out


def pileup_bam(data, regions, flags=0, require=0, exclude=0x704, min_mapq=0, min_baseq=0, ctx=None):
    """The pileup of a coordinate-sorted BAM file (bytes): `read_bam`, then `pileup_arrays`, with `regions` given as (name or
    index, beg, end) and resolved through the file's header (`resolve_regions`: a ValueError names a bad region before the
    records are touched).  Returns (rows, row_off)."""
    for region in regions:
        if not 0 <= region[1] <= region[2]:
            raise ValueError(f"region {region!r}: not 0 <= beg <= end")
    src = _lib.as_u8(data)

    def prefix(n):  # the header is a few members: inflated here, so that the regions are judged before any device work
        out, at = b"", 0
        while len(out) < n and at + 18 <= len(src):
            size = int(src[at + 16]) + (int(src[at + 17]) << 8) + 1
            try:
                out += zlib.decompress(src[at + 18:at + size - 8].tobytes(), -15)
            except zlib.error:  # no BGZF member: read_header says so of what there is
                break
            at += size
        return out[:n]
    _, contigs, _ = read_header(prefix)
    reg = resolve_regions(contigs, regions)
    _, contigs, stream, off = read_bam(data, ctx=ctx)
    return pileup_arrays(stream, off, contigs, reg, flags, require, exclude, min_mapq, min_baseq, ctx=ctx)


def depth(rows, deletions=False):
    """The depth of every position: the sum of the base columns (A, C, G, T, OTHER; both strands where the rows carry them),
    plus DEL where `deletions`"""
    rows = np.asarray(rows)
    cols = list(range(PILEUP_OTHER + 1)) + ([PILEUP_DEL] if deletions else [])
    total = rows[:, cols].sum(axis=1, dtype=np.uint64)
    if rows.shape[1] == 2 * PILEUP_COLS:
        total += rows[:, [PILEUP_COLS + c for c in cols]].sum(axis=1, dtype=np.uint64)
    return total


# ---- candidate sites and region summaries ------------------------------------------------------------------------------------
SITE_SNV, SITE_DEL, SITE_INS = _lib.SITE_SNV, _lib.SITE_DEL, _lib.SITE_INS


def sites_params(require=0, exclude=0x704, min_mapq=0, min_baseq=0, min_depth=0, min_alt=1, min_alt_permille=0, min_alt_strand=0, cover=(1, 10, 20, 30)):
    """bg_bam_sites_t: the pileup's filters, the four thresholds a candidate passes to be a site, and the four depths
    `covered` counts positions at"""
    p = np.zeros(1, dtype=_lib.BAM_SITES_DTYPE)
    p[0] = (0, require, exclude, min_mapq, min_baseq, 0, min_depth, min_alt, min_alt_permille, min_alt_strand, tuple(cover))
    return p


def sites_arrays(stream, off, contigs, text, regions, ctx=None, **params):
    """bg_bam_sites, host buffers: the candidate variant sites and the summaries of `regions` ((ref, beg, end), 0-based, half-open)
    from the coordinate-sorted records stream[off[i] .. off[i + 1]) held against the index text `text` that contigs.table's
    `start` addresses.  params: those of `sites_params`.  Returns (sites: BAM_SITE_DTYPE[], in region order, then by position,
    then SNVs by base, DEL, INS; site_off: uint64[n_regions + 1]; summary: BAM_REGION_SUMMARY_DTYPE[n_regions]).  Raises
    BamPileupError (status -1 INVALID_ARG, -11 UNSUPPORTED) with the offending slot."""
    ctx = ctx or _lib.default_context()
    src = _lib.as_u8(stream)
    src = src if len(src) else np.zeros(1, np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1 if len(off) else 0
    table = np.ascontiguousarray(contigs.table)
    ref_text = _lib.as_u8(text)
    reg = pileup_regions(regions)
    prm = sites_params(**params)
    total, bad = C.c_uint64(0), C.c_uint64(0)

    def call(sites, cap, site_off, summary):
        return _lib.lib().bg_bam_sites(ctx.h, prm.ctypes.data, n, src.ctypes.data, off.ctypes.data if n else None, table.ctypes.data if len(table) else None,
                                       len(table), ref_text.ctypes.data if len(ref_text) else None, len(ref_text), reg.ctypes.data if len(reg) else None,
                                       len(reg), sites, cap, site_off, summary, C.byref(total), C.byref(bad))
    _pileup_check(call(None, 0, None, None), "bg_bam_sites", bad)
    sites = np.zeros(max(total.value, 1), dtype=_lib.BAM_SITE_DTYPE)
    site_off = np.zeros(len(reg) + 1, dtype=np.uint64)
    summary = np.zeros(max(len(reg), 1), dtype=_lib.BAM_REGION_SUMMARY_DTYPE)
    _pileup_check(call(sites.ctypes.data, len(sites), site_off.ctypes.data, summary.ctypes.data), "bg_bam_sites", bad)
    return sites[:total.value], site_off, summary[:len(reg)]


def sites_dev(n_slots, d_recs, d_off, d_contigs, n_contigs, d_text, n_text, d_regions, n_regions, d_sites=0, sites_cap=0, d_site_off=0, d_summary=0,
              stream=0, ctx=None, **params):
    """bg_bam_sites_dev (pointers are ints; d_sites = 0 with sites_cap = 0 sizes; d_site_off and d_summary may be 0).  Returns
    n_sites, read back with the second synchronisation of `stream`; the records are then written asynchronously.  Raises
    BamPileupError with the offending slot, BiogpuError with status -9 (OPS_CAP) when sites_cap is too small."""
    ctx = ctx or _lib.default_context()
    prm = sites_params(**params)
    total, bad = C.c_uint64(0), C.c_uint64(0)
    rc = _lib.lib().bg_bam_sites_dev(ctx.h, prm.ctypes.data, n_slots, d_recs or None, d_off or None, d_contigs or None, n_contigs, d_text or None, n_text,
                                     d_regions or None, n_regions, d_sites or None, sites_cap, d_site_off or None, d_summary or None, C.byref(total),
                                     C.byref(bad), stream)
    _pileup_check(rc, "bg_bam_sites_dev", bad)
    return int(total.value)


def _reference_text(reference, contigs, ctx):
    """the index text behind `contigs` (a BAM header's table) from FASTA text (it begins with '>') or from a ready index text
    (sequences closed by '$' each); ValueError names the first contig whose length is not the header's"""
    ref = _lib.as_u8(reference)
    want = [int(v) for v in contigs.table["len"]]
    if len(ref) and ref[0] == ord(">"):
        from . import fasta
        parsed = fasta.parse_arrays(ref, ctx=ctx)
        if parsed.status != "ok":
            raise ValueError("the reference is no FASTA text: %s at byte %d" % (parsed.status, parsed.err_pos))
        text, got = fasta.reference_arrays(parsed)
        have = [int(v) for v in got.table["len"]]
    else:
        text = ref
        ends = np.nonzero(ref == ord("$"))[0].tolist()
        have = [e - b for b, e in zip([0] + [e + 1 for e in ends], ends)]
    for c in range(max(len(want), len(have))):
        if c >= len(want) or c >= len(have) or want[c] != have[c]:
            name = contigs.name(c).decode(errors="replace") if c < len(want) else "#%d" % c
            raise ValueError("contig %r: the header says %s bases, the reference %s" % (name, want[c] if c < len(want) else "nothing of",
                                                                                        have[c] if c < len(have) else "nothing of"))
    return text


def sites_bam(data, reference, regions, ctx=None, **params):
    """The candidate sites of a coordinate-sorted BAM file (bytes) against `reference`, FASTA text or a ready index text:
    `read_bam`, then `sites_arrays`, with `regions` given as (name or index, beg, end) and resolved through the file's header
    (`resolve_regions`).  The reference's contig lengths must be the header's: a ValueError names the first contig that
    differs.  Returns (sites, site_off, summary)."""
    _, contigs, stream, off = read_bam(data, ctx=ctx)
    reg = resolve_regions(contigs, regions)
    text = _reference_text(reference, contigs, ctx)
    return sites_arrays(stream, off, contigs, text, reg, ctx=ctx, **params)


# ---- indel events ------------------------------------------------------------------------------------------------------------
INDEL_DTYPE = _lib.BAM_INDEL_DTYPE
SEQ_CODES = b"=ACMGRSVTWYHKDBN"  # the ASCII byte of a 4-bit base code


def indels_params(require=0, exclude=0x704, min_mapq=0, min_baseq=0, min_depth=0, min_alt=1, min_alt_permille=0, min_alt_strand=0):
    """bg_bam_indels_t: the pileup's filters (min_baseq enters the depth only) and the four thresholds a kept event passes"""
    p = np.zeros(1, dtype=_lib.BAM_INDELS_DTYPE)
    p[0] = (0, require, exclude, min_mapq, min_baseq, 0, min_depth, min_alt, min_alt_permille, min_alt_strand)
    return p


def _indels_arrays(where, prm, stream, off, contigs, text, regions, ctx):
    """bg_bam_indels (text None) or bg_bam_indels_left behind `indels_arrays` / `indels_left_arrays`: a sizing call, then the call"""
    ctx = ctx or _lib.default_context()
    src = _lib.as_u8(stream)
    src = src if len(src) else np.zeros(1, np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1 if len(off) else 0
    table = np.ascontiguousarray(contigs.table)
    reg = pileup_regions(regions)
    ref_text = None if text is None else _lib.as_u8(text)
    with_text = () if text is None else (ref_text.ctypes.data if len(ref_text) else None, len(ref_text))
    total, n_seq, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call(events, cap, seq, seq_cap, event_off):
        return getattr(_lib.lib(), where)(ctx.h, prm.ctypes.data, n, src.ctypes.data, off.ctypes.data if n else None, table.ctypes.data if len(table) else None,
                                          len(table), *with_text, reg.ctypes.data if len(reg) else None, len(reg), events, cap, seq, seq_cap, event_off,
                                          C.byref(total), C.byref(n_seq), C.byref(bad))
    _pileup_check(call(None, 0, None, 0, None), where, bad)
    events = np.zeros(max(total.value, 1), dtype=INDEL_DTYPE)
    seq = np.zeros(max(n_seq.value, 1), dtype=np.uint8)
    event_off = np.zeros(len(reg) + 1, dtype=np.uint64)
    _pileup_check(call(events.ctypes.data, len(events), seq.ctypes.data, len(seq), event_off.ctypes.data), where, bad)
    return events[:total.value], seq[:n_seq.value], event_off


def indels_arrays(stream, off, contigs, regions, ctx=None, **params):
    """bg_bam_indels, host buffers: the indel events of `regions` ((ref, beg, end), 0-based, half-open) from the coordinate-sorted
    records stream[off[i] .. off[i + 1]).  params: those of `indels_params`.  Returns (events: INDEL_DTYPE[], in region order,
    then by anchor, deletions before insertions, then by length, insertions of one length by their codes; seq: uint8[], the
    inserted bases as ASCII, an insertion's at seq[seq_off : seq_off + len]; event_off: uint64[n_regions + 1]).  Raises
    BamPileupError (status -1 INVALID_ARG, -11 UNSUPPORTED) with the offending slot."""
    return _indels_arrays("bg_bam_indels", indels_params(**params), stream, off, contigs, None, regions, ctx)


def _indels_dev(where, prm, n_slots, d_recs, d_off, d_contigs, n_contigs, with_text, d_regions, n_regions, d_events, events_cap, d_seq, seq_cap, d_event_off,
                stream, ctx):
    """bg_bam_indels_dev (with_text empty) or bg_bam_indels_left_dev (with_text: d_text, n_text) behind `indels_dev` / `indels_left_dev`"""
    ctx = ctx or _lib.default_context()
    total, n_seq, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = getattr(_lib.lib(), where)(ctx.h, prm.ctypes.data, n_slots, d_recs or None, d_off or None, d_contigs or None, n_contigs, *with_text, d_regions or None,
                                    n_regions, d_events or None, events_cap, d_seq or None, seq_cap, d_event_off or None, C.byref(total), C.byref(n_seq),
                                    C.byref(bad), stream)
    try:
        _pileup_check(rc, where, bad)
    except _lib.BiogpuError as e:
        e.totals = (int(total.value), int(n_seq.value))
        raise
    return int(total.value), int(n_seq.value)


def indels_dev(n_slots, d_recs, d_off, d_contigs, n_contigs, d_regions, n_regions, d_events=0, events_cap=0, d_seq=0, seq_cap=0, d_event_off=0, stream=0,
               ctx=None, **params):
    """bg_bam_indels_dev (pointers are ints; d_events = 0 with events_cap = 0 sizes, d_seq must then be 0 too; d_event_off may be
    0).  Returns (n_events, n_seq), read back with the third synchronisation of `stream`; the records and sequences are then
    written asynchronously.  Raises BamPileupError with the offending slot, BiogpuError with status -9 (OPS_CAP) when a
    capacity is too small (`totals` then holds both totals)."""
    return _indels_dev("bg_bam_indels_dev", indels_params(**params), n_slots, d_recs, d_off, d_contigs, n_contigs, (), d_regions, n_regions, d_events, events_cap,
                       d_seq, seq_cap, d_event_off, stream, ctx)


def indels_bam(data, regions, ctx=None, **params):
    """The indel events of a coordinate-sorted BAM file (bytes): `read_bam`, then `indels_arrays`, with `regions` given as (name
    or index, beg, end) and resolved through the file's header (`resolve_regions`).  Returns (events, seq, event_off)."""
    _, contigs, stream, off = read_bam(data, ctx=ctx)
    reg = resolve_regions(contigs, regions)
    return indels_arrays(stream, off, contigs, reg, ctx=ctx, **params)


def indels_left_params(max_shift=0xFFFFFFFF, **thresholds):
    """bg_bam_indels_left_t: `indels_params` and the steps a raw event may take to the left (0: none, 0xFFFFFFFF: no limit)"""
    p = np.zeros(1, dtype=_lib.BAM_INDELS_LEFT_DTYPE)
    p.view(np.uint8)[:28] = indels_params(**thresholds).view(np.uint8)
    p["max_shift"] = max_shift
    return p


def indels_left_arrays(stream, off, contigs, text, regions, ctx=None, **params):
    """bg_bam_indels_left, host buffers: `indels_arrays` with every raw event shifted to the left against the index text `text`
    (the one `sites_arrays` takes) before events are merged, so that the spellings of one indel inside a repeat are one event.
    params: those of `indels_left_params`.  Returns what `indels_arrays` returns; the anchors are the shifted ones."""
    return _indels_arrays("bg_bam_indels_left", indels_left_params(**params), stream, off, contigs, text, regions, ctx)


def indels_left_dev(n_slots, d_recs, d_off, d_contigs, n_contigs, d_text, n_text, d_regions, n_regions, d_events=0, events_cap=0, d_seq=0, seq_cap=0,
                    d_event_off=0, stream=0, ctx=None, **params):
    """bg_bam_indels_left_dev: `indels_dev` with (d_text, n_text) behind n_contigs and `indels_left_params`; sizing, the returned
    totals and the errors are `indels_dev`'s."""
    return _indels_dev("bg_bam_indels_left_dev", indels_left_params(**params), n_slots, d_recs, d_off, d_contigs, n_contigs, (d_text or None, n_text), d_regions,
                       n_regions, d_events, events_cap, d_seq, seq_cap, d_event_off, stream, ctx)


def indels_left_bam(data, reference, regions, ctx=None, **params):
    """The left-aligned indel events of a coordinate-sorted BAM file (bytes) against `reference`, FASTA text or a ready index
    text, as `sites_bam` takes it: `read_bam`, then `indels_left_arrays`.  Returns (events, seq, event_off)."""
    _, contigs, stream, off = read_bam(data, ctx=ctx)
    reg = resolve_regions(contigs, regions)
    text = _reference_text(reference, contigs, ctx)
    return indels_left_arrays(stream, off, contigs, text, reg, ctx=ctx, **params)


def indel_sequences(events, seq):
    """the inserted strings of `events` (bytes each; b"" for a deletion)"""
    raw = _lib.as_u8(seq).tobytes()
    return [raw[int(e["seq_off"]):int(e["seq_off"]) + int(e["len"])] if int(e["kind"]) == SITE_INS else b"" for e in events]


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
