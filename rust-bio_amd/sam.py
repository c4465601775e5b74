"""SAM records from seed-and-extend hits — host mirror of `bg_sam_header` and `bg_sam_emit_batch[_dev]`.

rust-bio has no SAM writer; the record is defined in include/biogpu.h from the SAM specification and formatted in HIP kernels
(rust-bio_amd/csrc/sam_emit.hip) out of what `fastq.parse_*` and the `pipeline.seed_extend_*` calls leave behind: FASTQ records,
hits, strands, operations and, where given, the multi and pair records.  This module only marshals arguments."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SAM_PAIRED, SAM_SECONDARY, SAM_TAG_MD, SAM_TAG_NM  # noqa: F401


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


def header(contigs):
    """bg_sam_header: the @HD, @SQ and @PG lines as bytes (host only)."""
    n = C.c_uint64(0)
    args = (contigs.table.ctypes.data, len(contigs), contigs.names.ctypes.data)
    _lib.check(_lib.lib().bg_sam_header(*args, None, 0, C.byref(n)), "bg_sam_header")
    out = np.zeros(max(n.value, 1), dtype=np.uint8)
    _lib.check(_lib.lib().bg_sam_header(*args, out.ctypes.data, n.value, C.byref(n)), "bg_sam_header")
    return out[:n.value].tobytes()


def emit_arrays(fm, params, contigs, parsed, hits, strand, ops, multi=None, pairs=None):
    """bg_sam_emit_batch, host buffers: `parsed` is a fastq.Parsed (text, recs, seq, qual), hits / strand / ops / multi / pairs
    what the host seed-extend calls returned for its reads.  Returns (text: bytes, out_off: uint64[n_reads * K + 1])."""
    n = len(parsed.recs)
    hits = np.ascontiguousarray(hits).reshape(-1)
    strand = np.ascontiguousarray(strand, dtype=np.uint8).reshape(-1)
    bufs = [np.ascontiguousarray(x) if len(x) else np.zeros(1, np.uint8) for x in (parsed.text, parsed.seq, parsed.qual, ops)]
    recs = np.ascontiguousarray(parsed.recs)
    out_off = np.zeros(n * max(params.max_hits, 1) + 1, dtype=np.uint64)
    total = C.c_uint64(0)
    pc = params.to_c()

    def call(out, cap):
        return _lib.lib().bg_sam_emit_batch(fm.h, C.byref(pc), n, contigs.table.ctypes.data, len(contigs), contigs.names.ctypes.data,
                                            bufs[0].ctypes.data, recs.ctypes.data, bufs[1].ctypes.data, bufs[2].ctypes.data,
                                            hits.ctypes.data, strand.ctypes.data, bufs[3].ctypes.data,
                                            multi.ctypes.data if multi is not None else None,
                                            pairs.ctypes.data if pairs is not None else None, out, cap, out_off.ctypes.data,
                                            C.byref(total))
    _lib.check(call(None, 0), "bg_sam_emit_batch")
    out = np.zeros(max(total.value, 1), dtype=np.uint8)
    _lib.check(call(out.ctypes.data, total.value), "bg_sam_emit_batch")
    return out[:total.value].tobytes(), out_off


def emit_dev(fm, params, n_reads, d_contigs, n_contigs, d_names, d_fastq_text, d_recs, d_seq, d_qual, d_hits, d_strand, d_ops,
             d_out, out_cap, d_out_off, d_multi=0, d_pairs=0, stream=0):
    """bg_sam_emit_batch_dev (pointers are ints; d_multi / d_pairs may be 0; d_out = 0 with out_cap = 0 sizes).  Returns the
    total number of bytes of the lines; raises BiogpuError with status -9 (OPS_CAP) when it exceeds out_cap."""
    total = C.c_uint64(0)
    pc = params.to_c()
    rc = _lib.lib().bg_sam_emit_batch_dev(fm.h, C.byref(pc), n_reads, d_contigs, n_contigs, d_names, d_fastq_text, d_recs, d_seq, d_qual,
                                          d_hits, d_strand, d_ops, d_multi or None, d_pairs or None, d_out or None, out_cap, d_out_off,
                                          C.byref(total), stream)
    _lib.check(rc, "bg_sam_emit_batch_dev")
    return int(total.value)
