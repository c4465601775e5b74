"""`bio::io::fastq` (io/fastq.rs:153-599) on FASTQ text held in memory.  Reading: the records are parsed on the device
(csrc/fastq_ingest.hip) — line index, four-line hypothesis, sequential walk only where it fails — and the sequences land
concatenated with offsets, i.e. in the layout the aligner's batch calls take.  Writing (csrc/fastq_emit.hip): `Writer`,
`emit_arrays` / `emit_dev` write the text of parsed, trimmed or filtered records on the device, `filter_arrays` /
`filter_dev` select records by length, 'N' count, `check`, trim state and pair (the rule is defined in include/biogpu.h).
Demultiplexing (csrc/fastq_demux.hip): `demux_assign_*` turn the records of a Myers best call into a sample per read,
`demux_split_*` group the records by sample, `demux_texts` slices one emitted buffer into per-sample texts.
Qualities (csrc/fastq_qual.hip): `qual_cut_*` give a cut point per read by the running-sum or the sliding-window rule,
`qual_select_*` per-read statistics and a pass / fail bin, `qc_tables_*` the per-cycle tables of a batch; `qual_trim_arrays`
is cut, trim 3', trim 5' in one call and `ee_weights` the table that makes the selection an expected-error filter."""
import ctypes as C

import numpy as np

from . import _lib

from ._lib import FQF_CHECK_OK, FQF_DISCARD_TRIMMED, FQF_DISCARD_UNTRIMMED, FQF_PAIR_BOTH, FQF_PAIRED  # noqa: F401
from ._lib import DMX_ANCHOR_3P, DMX_ANCHOR_5P, DMX_IGNORE, DMX_MATE1, DMX_MATE2, DMX_MAX_BINS, DMX_PAIRED  # noqa: F401
from ._lib import QC_MAX_CYCLES, QCUT_NONE, QCUT_RUNSUM, QCUT_WINDOW, QSEL_PAIR_BOTH, QSEL_PAIRED  # noqa: F401

STATUS = ["ok", "MissingAt", "IncompleteRecord", "Io"]
CHECK = ["ok", "EmptyId", "NonAsciiSequence", "InvalidSequence", "NonAsciiQualities", "UnequalLength"]


class ReadError(Exception):
    """fastq::ReadError (fastq.rs:113-126)"""

    def __init__(self, kind, pos):
        super().__init__(f"{kind} at byte {pos}")
        self.kind, self.pos = kind, pos


class CheckError(Exception):
    """fastq::CheckError (fastq.rs:129-150)"""

    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


class Record:
    """fastq::Record (fastq.rs:309-452)"""

    def __init__(self, id_=b"", desc=None, seq=b"", qual=b"", check_code=0):
        self._id, self._desc, self._seq, self._qual, self._check = id_, desc, seq, qual, check_code

    def id(self):
        return self._id.decode()

    def desc(self):
        return None if self._desc is None else self._desc.decode()

    def seq(self):
        return self._seq

    def qual(self):
        return self._qual

    def is_empty(self):  # fastq.rs:363-365
        return not self._id and self._desc is None and not self._seq and not self._qual

    def check(self):  # fastq.rs:388-410, evaluated on the device with the parse
        if self._check:
            raise CheckError(CHECK[self._check])

    def __eq__(self, o):
        return (self._id, self._desc, self._seq, self._qual) == (o._id, o._desc, o._seq, o._qual)

    def __repr__(self):
        return f"Record(id={self._id!r}, desc={self._desc!r}, seq={self._seq!r}, qual={self._qual!r})"


class Parsed:
    """columns of one parse: recs (bg_fastq_record_t), seq/qual (concatenated), seq_off/qual_off (n+1)"""

    def __init__(self, text, recs, seq, seq_off, qual, qual_off, status, err_pos):
        self.text, self.recs, self.seq, self.seq_off, self.qual, self.qual_off = text, recs, seq, seq_off, qual, qual_off
        self.status, self.err_pos = STATUS[status], err_pos

    def __len__(self):
        return len(self.recs)

    def record(self, k):
        r, t = self.recs[k], self.text
        return Record(t[int(r["id_off"]):int(r["id_off"]) + int(r["id_len"])].tobytes(),
                      t[int(r["desc_off"]):int(r["desc_off"]) + int(r["desc_len"])].tobytes() if r["has_desc"] else None,
                      self.seq[int(self.seq_off[k]):int(self.seq_off[k + 1])].tobytes(),
                      self.qual[int(self.qual_off[k]):int(self.qual_off[k + 1])].tobytes(), int(r["check"]))


def parse_arrays(text, ctx=None):
    """All records up to the end of the text or the first ReadError (Parsed.status / err_pos)."""
    ctx = ctx or _lib.default_context()
    t = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, dtype=np.uint8)
    cap = len(t) // 4 + 2
    recs = np.zeros(cap, dtype=_lib.FQREC_DTYPE)
    seq = np.zeros(max(1, len(t)), dtype=np.uint8)
    qual = np.zeros(max(1, len(t)), dtype=np.uint8)
    so = np.zeros(cap + 1, dtype=np.uint64)
    qo = np.zeros(cap + 1, dtype=np.uint64)
    n, st, ep = C.c_uint64(0), C.c_int32(0), C.c_uint64(0)
    _lib.check(_lib.lib().bg_fastq_parse(ctx.h, t.ctypes.data, len(t), recs.ctypes.data, cap, seq.ctypes.data, so.ctypes.data,
                                         qual.ctypes.data, qo.ctypes.data, C.byref(n), C.byref(st), C.byref(ep)), "bg_fastq_parse")
    k = int(n.value)
    return Parsed(t, recs[:k], seq[:int(so[k])], so[:k + 1], qual[:int(qo[k])], qo[:k + 1], st.value, int(ep.value))


def parse_dev(d_text, ctx=None, stream=0, bufs=None):
    """d_text: uint8 torch tensor on the device.  Returns (n_records, status name, err_pos, d_recs, d_seq, d_seq_off,
    d_qual, d_qual_off) with everything but the first three left in HBM (d_seq_off is an int64 tensor usable as x_off).
    `bufs`: the five tensors of `alloc_dev(len)` to reuse across calls (a caller's own buffers)."""
    import torch
    ctx = ctx or _lib.default_context()
    ln = int(d_text.numel())
    cap = ln // 4 + 2
    d_recs, d_seq, d_qual, d_so, d_qo = bufs if bufs is not None else alloc_dev(ln, d_text.device)
    n, st, ep = C.c_uint64(0), C.c_int32(0), C.c_uint64(0)
    _lib.check(_lib.lib().bg_fastq_parse_dev(ctx.h, d_text.data_ptr(), ln, d_recs.data_ptr(), cap, d_seq.data_ptr(), d_so.data_ptr(),
                                             d_qual.data_ptr(), d_qo.data_ptr(), C.byref(n), C.byref(st), C.byref(ep), stream),
               "bg_fastq_parse_dev")
    k = int(n.value)
    return k, STATUS[st.value], int(ep.value), d_recs[:k * 56], d_seq, d_so[:k + 1], d_qual, d_qo[:k + 1]


def parse_bgzf_dev(d_file, ctx=None, stream=0):
    """d_file: uint8 torch tensor on the device holding a bgzipped FASTQ file (.fastq.gz written by bgzip, htslib or
    `bam.bgzf_deflate_*`).  The block table (bg_bgzf_blocks_dev), the payloads (bg_bgzf_inflate_dev) and the parse
    (`parse_dev`) run on the device; the text never visits the host.  Returns (d_text, the tuple of `parse_dev` on it); raises
    `bam.BgzfError` where the file is not BGZF or a block does not inflate."""
    import torch
    from . import bam
    ctx = ctx or _lib.default_context()
    ln = int(d_file.numel())
    cap = ln // 28 + 1  # a member has at least 28 bytes: the tables need no sizing call
    d_block_off = torch.empty(cap + 1, dtype=torch.int64, device=d_file.device)
    d_out_off = torch.empty(cap + 1, dtype=torch.int64, device=d_file.device)
    n_blocks, out_bytes = bam.bgzf_blocks_dev(d_file.data_ptr(), ln, d_block_off.data_ptr(), d_out_off.data_ptr(), cap, stream=stream, ctx=ctx)
    d_text = torch.empty(out_bytes, dtype=torch.uint8, device=d_file.device)  # (no bytes, no address: a file of empty members)
    bam.bgzf_inflate_dev(d_file.data_ptr(), ln, n_blocks, d_block_off.data_ptr(), d_out_off.data_ptr(), d_text.data_ptr() if out_bytes else 0, out_bytes,
                         stream=stream, ctx=ctx)
    return d_text, parse_dev(d_text, ctx=ctx, stream=stream)


def parse_bam_dev(d_file, flags=0, require=0, exclude=0, ctx=None, stream=0):
    """d_file: uint8 torch tensor on the device holding a BAM file (uBAM from an instrument, a mapped BAM to be re-mapped).  The
    block table, the payloads, the record table (bg_bam_records_dev) and the reads (bg_bam_reads_dev) run on the device; only
    the header's prefix visits the host.  Returns (d_stream, (n_reads, d_recs, d_seq, d_seq_off, d_qual, d_qual_off, d_src)):
    the columns every call after `parse_dev` takes, with d_stream where those take the FASTQ text.  flags: bam.BAM_READS_ORIGINAL;
    require / exclude: FLAG bits (exclude=0x900 drops secondary and supplementary records)."""
    import torch
    from . import bam
    ctx = ctx or _lib.default_context()
    ln = int(d_file.numel())
    cap = ln // 28 + 1
    dev = d_file.device
    d_block_off = torch.empty(cap + 1, dtype=torch.int64, device=dev)
    d_out_off = torch.empty(cap + 1, dtype=torch.int64, device=dev)
    n_blocks, out_bytes = bam.bgzf_blocks_dev(d_file.data_ptr(), ln, d_block_off.data_ptr(), d_out_off.data_ptr(), cap, stream=stream, ctx=ctx)
    d_stream = torch.empty(max(out_bytes, 1), dtype=torch.uint8, device=dev)[:out_bytes]
    bam.bgzf_inflate_dev(d_file.data_ptr(), ln, n_blocks, d_block_off.data_ptr(), d_out_off.data_ptr(), d_stream.data_ptr() if out_bytes else 0, out_bytes,
                         stream=stream, ctx=ctx)
    _, contigs, body_off = bam.read_header(lambda n: d_stream[:n].cpu().numpy())
    n_ref = len(contigs)
    n_rec, _ = bam.records_dev(d_stream.data_ptr(), out_bytes, body_off, n_ref, stream=stream, ctx=ctx)
    d_off = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
    bam.records_dev(d_stream.data_ptr(), out_bytes, body_off, n_ref, d_off.data_ptr(), n_rec, stream=stream, ctx=ctx)
    k, sb, qb = bam.reads_dev(n_rec, d_stream.data_ptr(), d_off.data_ptr(), n_ref, flags=flags, require=require, exclude=exclude, stream=stream, ctx=ctx)
    d_recs = torch.empty(max(k, 1) * 56, dtype=torch.uint8, device=dev)
    d_seq, d_qual = torch.empty(max(sb, 1), dtype=torch.uint8, device=dev), torch.empty(max(qb, 1), dtype=torch.uint8, device=dev)
    d_so, d_qo = torch.empty(k + 1, dtype=torch.int64, device=dev), torch.empty(k + 1, dtype=torch.int64, device=dev)
    d_src = torch.empty(max(k, 1), dtype=torch.int64, device=dev)
    bam.reads_dev(n_rec, d_stream.data_ptr(), d_off.data_ptr(), n_ref, d_recs.data_ptr(), k, d_seq.data_ptr(), sb, d_so.data_ptr(), d_qual.data_ptr(), qb,
                  d_qo.data_ptr(), d_src.data_ptr(), flags=flags, require=require, exclude=exclude, stream=stream, ctx=ctx)
    return d_stream, (k, d_recs[:k * 56], d_seq[:sb], d_so, d_qual[:qb], d_qo, d_src[:k])


def alloc_dev(ln, device):
    """output buffers of parse_dev for a text of `ln` bytes: records, sequences, qualities, their offsets"""
    import torch
    cap = ln // 4 + 2
    return (torch.empty(cap * 56, dtype=torch.uint8, device=device), torch.empty(max(1, ln), dtype=torch.uint8, device=device),
            torch.empty(max(1, ln), dtype=torch.uint8, device=device), torch.empty(cap + 1, dtype=torch.int64, device=device),
            torch.empty(cap + 1, dtype=torch.int64, device=device))


class Reader:
    """fastq::Reader over an in-memory text (`Reader::new(&[u8])`, fastq.rs:170-176)."""

    def __init__(self, text, ctx=None):
        self._parsed = parse_arrays(text, ctx)

    def records(self):
        """`Reader::records()` (fastq.rs:218-220): yields Records; raises ReadError where the iterator yields Err."""
        p = self._parsed
        for k in range(len(p)):
            yield p.record(k)
        if p.status != "ok":
            raise ReadError(p.status, p.err_pos)


# ---- filtering -------------------------------------------------------------------------------------------------------
NO_BOUND = 0xFFFFFFFF


def filter_params(flags=0, min_len=0, max_len=NO_BOUND, max_n=NO_BOUND):
    """bg_fastq_filter_t as a one-element array"""
    f = np.zeros(1, dtype=_lib.FQ_FILTER_DTYPE)
    f["flags"], f["min_len"], f["max_len"], f["max_n"] = flags, min_len, max_len, max_n
    return f


def filter_arrays(recs, seq, seq_off, qual, qual_off, flags=0, min_len=0, max_len=NO_BOUND, max_n=NO_BOUND, hits=None, n_pat=0, ctx=None):
    """bg_fastq_filter over host arrays (the columns of parse_arrays or myers.trim; hits: the records of best_batch the trim
    was given, needed by the two DISCARD flags only).  Returns (recs, seq, seq_off, qual, qual_off, keep): the kept records
    compacted, and keep[n] = 0 / 1."""
    ctx = ctx or _lib.default_context()
    n = len(recs)
    f = filter_params(flags, min_len, max_len, max_n)
    hits = np.ascontiguousarray(hits, dtype=_lib.ALN_DTYPE) if hits is not None else None
    recs, seq, seq_off, qual, qual_off = _lib.fq_columns(recs, seq, seq_off, qual, qual_off)
    o_recs, o_seq, o_so, o_qual, o_qo = _lib.fq_host_outputs(n, n, seq, qual)
    keep = np.zeros(max(1, n), dtype=np.uint8)
    tot = (C.c_uint64 * 3)()
    _lib.check(_lib.lib().bg_fastq_filter(ctx.h, n, f.ctypes.data, hits.ctypes.data if hits is not None else None, int(n_pat),
                                          recs.ctypes.data, seq.ctypes.data, seq_off.ctypes.data, qual.ctypes.data, qual_off.ctypes.data,
                                          o_recs.ctypes.data, o_seq.ctypes.data, o_so.ctypes.data, o_qual.ctypes.data, o_qo.ctypes.data,
                                          keep.ctypes.data, tot), "bg_fastq_filter")
    k = int(tot[0])
    return o_recs[:k], o_seq[:int(tot[1])], o_so[:k + 1], o_qual[:int(tot[2])], o_qo[:k + 1], keep[:n]


def filter_dev(n, d_recs, d_seq, d_seq_off, d_qual, d_qual_off, flags=0, min_len=0, max_len=NO_BOUND, max_n=NO_BOUND, d_hits=None, n_pat=0,
               ctx=None, stream=0, want_totals=True, want_keep=False, out=None):
    """bg_fastq_filter_dev on torch device tensors (the outputs of parse_dev or myers.trim_dev).  Returns (d_recs, d_seq,
    d_seq_off, d_qual, d_qual_off, d_keep, totals) — new tensors in HBM, never the inputs; totals = (records kept, sequence
    bytes, quality bytes), and the record and offset tensors cut to the kept records — or None (then the call does not
    synchronise and the tensors keep the capacity of the inputs).  d_keep: n bytes 0 / 1, or None without want_keep.  `out`:
    the first six results of an earlier call of the same shape made without totals, to write into instead of allocating."""
    import torch
    ctx = ctx or _lib.default_context()
    f = filter_params(flags, min_len, max_len, max_n)
    if out is not None:
        o_recs, o_seq, o_so, o_qual, o_qo, d_keep = out[:6]
    else:
        o_recs, o_seq, o_so, o_qual, o_qo = _lib.fq_dev_outputs(n, n, d_seq, d_qual)
        d_keep = torch.empty(max(1, n), dtype=torch.uint8, device=d_seq.device) if want_keep else None
    tot = (C.c_uint64 * 3)()
    _lib.check(_lib.lib().bg_fastq_filter_dev(ctx.h, n, f.ctypes.data, d_hits.data_ptr() if d_hits is not None else None, int(n_pat),
                                              d_recs.data_ptr(), d_seq.data_ptr(), d_seq_off.data_ptr(), d_qual.data_ptr(),
                                              d_qual_off.data_ptr(), o_recs.data_ptr(), o_seq.data_ptr(), o_so.data_ptr(),
                                              o_qual.data_ptr(), o_qo.data_ptr(), d_keep.data_ptr() if d_keep is not None else None,
                                              tot if want_totals else None, stream), "bg_fastq_filter_dev")
    if not want_totals:
        return o_recs, o_seq, o_so, o_qual, o_qo, d_keep, None
    k = int(tot[0])
    return o_recs[:k * 56], o_seq, o_so[:k + 1], o_qual, o_qo[:k + 1], d_keep, (k, int(tot[1]), int(tot[2]))


# ---- demultiplexing --------------------------------------------------------------------------------------------------
def demux_params(n_bins, flags=0, min_margin=0, max_offset=0):
    """bg_demux_params_t as a one-element array"""
    p = np.zeros(1, dtype=_lib.DEMUX_PARAMS_DTYPE)
    p["flags"], p["n_bins"], p["min_margin"], p["max_offset"] = flags, n_bins, min_margin, max_offset
    return p


def demux_assign_arrays(hits, n_pat, pat_bin, n_bins, flags=0, min_margin=0, max_offset=0, want_pat=True, ctx=None):
    """bg_fastq_demux_assign over host arrays: hits are the n * n_pat records of myers.best_batch / long_best_batch, pat_bin
    the sample of every pattern (DMX_IGNORE: none).  Returns (bin uint32[n], hit_out records[n], pat_out uint32[n] or None):
    bin n_bins is unassigned, n_bins + 1 ambiguous; hit_out is what myers.trim takes with n_pat = 1."""
    ctx = ctx or _lib.default_context()
    hits = np.ascontiguousarray(hits, dtype=_lib.ALN_DTYPE)
    pat_bin = np.ascontiguousarray(pat_bin, dtype=np.uint32)
    n = len(hits) // max(1, int(n_pat))
    prm = demux_params(n_bins, flags, min_margin, max_offset)
    o_bin, o_hit = np.zeros(max(1, n), dtype=np.uint32), np.zeros(max(1, n), dtype=_lib.ALN_DTYPE)
    o_pat = np.zeros(max(1, n), dtype=np.uint32) if want_pat else None
    _lib.check(_lib.lib().bg_fastq_demux_assign(ctx.h, n, prm.ctypes.data, hits.ctypes.data, int(n_pat), pat_bin.ctypes.data,
                                                o_bin.ctypes.data, o_hit.ctypes.data, o_pat.ctypes.data if want_pat else None),
               "bg_fastq_demux_assign")
    return o_bin[:n], o_hit[:n], o_pat[:n] if want_pat else None


def demux_assign_dev(n, d_hits, n_pat, pat_bin, n_bins, flags=0, min_margin=0, max_offset=0, ctx=None, stream=0, want_pat=False, out=None):
    """bg_fastq_demux_assign_dev on the device records of myers.best_batch_dev (pat_bin is a host array).  Returns (d_bin
    int32[n], d_hit_out uint8[n * 64], d_pat int32[n] or None) in HBM without synchronising; the 32-bit columns hold
    unsigned values.  `out`: the results of an earlier call of the same shape, to write into instead of allocating."""
    import torch
    ctx = ctx or _lib.default_context()
    pat_bin = np.ascontiguousarray(pat_bin, dtype=np.uint32)
    prm = demux_params(n_bins, flags, min_margin, max_offset)
    if out is not None:
        d_bin, d_hit, d_pat = out[:3]
    else:
        dev = d_hits.device
        d_bin = torch.empty(max(1, n), dtype=torch.int32, device=dev)
        d_hit = torch.empty(max(1, n) * 64, dtype=torch.uint8, device=dev)
        d_pat = torch.empty(max(1, n), dtype=torch.int32, device=dev) if want_pat else None
    _lib.check(_lib.lib().bg_fastq_demux_assign_dev(ctx.h, n, prm.ctypes.data, d_hits.data_ptr(), int(n_pat), pat_bin.ctypes.data,
                                                    d_bin.data_ptr(), d_hit.data_ptr(), d_pat.data_ptr() if d_pat is not None else None,
                                                    stream), "bg_fastq_demux_assign_dev")
    return d_bin[:n], d_hit[:n * 64], d_pat[:n] if d_pat is not None else None


def demux_split_arrays(bins, n_bins, recs, seq, seq_off, qual, qual_off, hit=None, ctx=None):
    """bg_fastq_demux_split over host arrays: the columns of parse_arrays, myers.trim or filter_arrays grouped by `bins` (the
    first result of demux_assign_arrays), stably.  Returns (recs, seq, seq_off, qual, qual_off, hit_out or None, perm
    uint64[n], bin_off uint64[n_bins + 3]): group g's records are bin_off[g] .. bin_off[g + 1]."""
    ctx = ctx or _lib.default_context()
    n = len(recs)
    bins = np.ascontiguousarray(bins, dtype=np.uint32)
    hit = np.ascontiguousarray(hit, dtype=_lib.ALN_DTYPE) if hit is not None else None
    recs, seq, seq_off, qual, qual_off = _lib.fq_columns(recs, seq, seq_off, qual, qual_off)
    o_recs, o_seq, o_so, o_qual, o_qo = _lib.fq_host_outputs(n, max(1, n), seq, qual)
    o_hit = np.zeros(max(1, n), dtype=_lib.ALN_DTYPE) if hit is not None else None
    perm, bin_off = np.zeros(max(1, n), dtype=np.uint64), np.zeros(int(n_bins) + 3, dtype=np.uint64)
    pad = np.zeros(1, dtype=np.uint8)  # no empty buffers: the call refuses null pointers
    _lib.check(_lib.lib().bg_fastq_demux_split(ctx.h, n, int(n_bins), bins.ctypes.data if n else pad.ctypes.data,
                                               hit.ctypes.data if hit is not None else None, recs.ctypes.data, seq.ctypes.data,
                                               seq_off.ctypes.data, qual.ctypes.data, qual_off.ctypes.data, o_recs.ctypes.data,
                                               o_seq.ctypes.data, o_so.ctypes.data, o_qual.ctypes.data, o_qo.ctypes.data,
                                               o_hit.ctypes.data if o_hit is not None else None, perm.ctypes.data, bin_off.ctypes.data),
               "bg_fastq_demux_split")
    return (o_recs[:n], o_seq[:int(o_so[n])], o_so, o_qual[:int(o_qo[n])], o_qo, o_hit[:n] if o_hit is not None else None, perm[:n],
            bin_off)


def demux_split_dev(n, d_bin, n_bins, d_recs, d_seq, d_seq_off, d_qual, d_qual_off, d_hit=None, ctx=None, stream=0, want_bin_off=True,
                    want_perm=False, out=None):
    """bg_fastq_demux_split_dev on torch device tensors (d_bin: demux_assign_dev's; the columns of parse_dev, myers.trim_dev or
    filter_dev; d_hit: n records, e.g. demux_assign_dev's second result).  Returns (d_recs, d_seq, d_seq_off, d_qual,
    d_qual_off, d_hit_out or None, d_perm or None, d_bin_off int64[n_bins + 3], bin_off) — new tensors in HBM, never the
    inputs; bin_off is the host copy of d_bin_off (a uint64 array), or None without want_bin_off, and then the call does not
    synchronise.  `out`: the first eight results of an earlier call of the same shape, to write into instead of allocating."""
    import torch
    ctx = ctx or _lib.default_context()
    dev = d_seq.device
    if out is not None:
        o_recs, o_seq, o_so, o_qual, o_qo, o_hit, d_perm, d_boff = out[:8]
    else:
        o_recs, o_seq, o_so, o_qual, o_qo = _lib.fq_dev_outputs(n, max(1, n), d_seq, d_qual)
        o_hit = torch.empty(max(1, n) * 64, dtype=torch.uint8, device=dev) if d_hit is not None else None
        d_perm = torch.empty(max(1, n), dtype=torch.int64, device=dev) if want_perm else None
        d_boff = torch.empty(int(n_bins) + 3, dtype=torch.int64, device=dev)
    bin_off = np.zeros(int(n_bins) + 3, dtype=np.uint64) if want_bin_off else None
    _lib.check(_lib.lib().bg_fastq_demux_split_dev(ctx.h, n, int(n_bins), d_bin.data_ptr(), d_hit.data_ptr() if d_hit is not None else None,
                                                   d_recs.data_ptr(), d_seq.data_ptr(), d_seq_off.data_ptr(), d_qual.data_ptr(),
                                                   d_qual_off.data_ptr(), o_recs.data_ptr(), o_seq.data_ptr(), o_so.data_ptr(),
                                                   o_qual.data_ptr(), o_qo.data_ptr(), o_hit.data_ptr() if o_hit is not None else None,
                                                   d_perm.data_ptr() if d_perm is not None else None, d_boff.data_ptr(),
                                                   bin_off.ctypes.data if want_bin_off else None, stream), "bg_fastq_demux_split_dev")
    return (o_recs[:n * 56], o_seq, o_so, o_qual, o_qo, o_hit[:n * 64] if o_hit is not None else None,
            d_perm[:n] if d_perm is not None else None, d_boff, bin_off)


def demux_texts(out, out_off, bin_off, n_bins, first=0, step=1):
    """The per-sample texts inside ONE emit over split columns: `out`, `out_off` as emit_dev / emit_arrays return them for
    (first, step), bin_off the host offsets of the split.  Returns n_bins + 2 slices of `out` (views, nothing is copied):
    the samples, then unassigned, then ambiguous.  With (0, 2) and (1, 2) on interleaved mates: the R1 and the R2 texts."""
    lines = [n_lines(int(b), first, step) for b in bin_off[:int(n_bins) + 3]]
    idx = np.asarray(lines, dtype=np.int64)
    if isinstance(out_off, np.ndarray):
        cuts = out_off[idx]
    else:  # a device tensor: n_bins + 3 offsets cross, not the column
        import torch
        cuts = out_off[torch.from_numpy(idx).to(out_off.device)].cpu().numpy()
    return [out[int(cuts[g]):int(cuts[g + 1])] for g in range(int(n_bins) + 2)]


# ---- qualities -------------------------------------------------------------------------------------------------------
def qual_cut_params(method_5p=QCUT_NONE, method_3p=QCUT_RUNSUM, cutoff_5p=0, cutoff_3p=0, window=0, phred_offset=33):
    """bg_qual_cut_t as a one-element array"""
    p = np.zeros(1, dtype=_lib.QUAL_CUT_DTYPE)
    p["phred_offset"], p["method_5p"], p["method_3p"] = phred_offset, method_5p, method_3p
    p["cutoff_5p"], p["cutoff_3p"], p["window"] = cutoff_5p, cutoff_3p, window
    return p


def qual_cut_arrays(qual, qual_off, want_totals=False, ctx=None, **params):
    """bg_fastq_qual_cut over host arrays (the quality column of parse_arrays, myers.trim, filter_arrays or a split; params:
    those of qual_cut_params).  Returns the cut records[n] — what myers.trim takes with n_pat = 1: TRIM_3P keeps [0, e),
    TRIM_5P of its output then [b, e) — or (records, (reads cut, symbols removed)) with want_totals."""
    ctx = ctx or _lib.default_context()
    qual, qual_off = _lib.as_u8(qual), np.ascontiguousarray(qual_off, dtype=np.uint64)
    n = len(qual_off) - 1
    prm = qual_cut_params(**params)
    pad = np.zeros(1, dtype=np.uint8)  # no empty buffers: the call refuses null pointers
    cut = np.zeros(max(1, n), dtype=_lib.ALN_DTYPE)
    tot = (C.c_uint64 * 2)()
    _lib.check(_lib.lib().bg_fastq_qual_cut(ctx.h, n, prm.ctypes.data, qual.ctypes.data if len(qual) else pad.ctypes.data, qual_off.ctypes.data,
                                            cut.ctypes.data, tot if want_totals else None), "bg_fastq_qual_cut")
    return (cut[:n], (int(tot[0]), int(tot[1]))) if want_totals else cut[:n]


def qual_cut_dev(n, d_qual, d_qual_off, ctx=None, stream=0, want_totals=False, out=None, **params):
    """bg_fastq_qual_cut_dev on torch device tensors.  Returns (d_cut uint8[n * 64], totals): the records in HBM — what
    myers.trim_dev takes as d_hits with n_pat = 1 — and (reads cut, symbols removed), or None without want_totals, and then
    the call does not synchronise.  `out`: d_cut of an earlier call of the same shape, to write into instead of allocating."""
    import torch
    ctx = ctx or _lib.default_context()
    prm = qual_cut_params(**params)
    d_cut = out if out is not None else torch.empty(max(1, n) * 64, dtype=torch.uint8, device=d_qual.device)
    tot = (C.c_uint64 * 2)()
    _lib.check(_lib.lib().bg_fastq_qual_cut_dev(ctx.h, n, prm.ctypes.data, d_qual.data_ptr(), d_qual_off.data_ptr(), d_cut.data_ptr(),
                                                tot if want_totals else None, stream), "bg_fastq_qual_cut_dev")
    return d_cut[:n * 64], ((int(tot[0]), int(tot[1])) if want_totals else None)


def ee_weights(phred_offset=33, scale_bits=20):
    """The weight table of an expected-error filter: round(10^(-q / 10) * 2^scale_bits) per raw byte, q = max(0, c - phred_offset)"""
    q = np.maximum(np.arange(256, dtype=np.int64) - int(phred_offset), 0)
    return np.round(10.0 ** (-q / 10.0) * float(1 << scale_bits)).astype(np.uint32)


def qual_select_params(flags=0, min_mean_q=0, low_q=0, max_low_pct=100, max_weight=0, phred_offset=33):
    """bg_qual_select_t as a one-element array"""
    p = np.zeros(1, dtype=_lib.QUAL_SELECT_DTYPE)
    p["flags"], p["phred_offset"], p["min_mean_q"], p["low_q"] = flags, phred_offset, min_mean_q, low_q
    p["max_low_pct"], p["max_weight"] = max_low_pct, max_weight
    return p


def _select_table(params, weight, max_ee, scale_bits):
    """max_ee (a float) is ee_weights with max_weight scaled the same way"""
    if max_ee is not None:
        weight = ee_weights(params.get("phred_offset", 33), scale_bits)
        params["max_weight"] = int(round(float(max_ee) * float(1 << scale_bits)))
    return qual_select_params(**params), (np.ascontiguousarray(weight, dtype=np.uint32) if weight is not None else None)


def qual_select_arrays(qual, qual_off, weight=None, max_ee=None, scale_bits=20, want_totals=False, ctx=None, **params):
    """bg_fastq_qual_select over host arrays (params: those of qual_select_params; weight: uint32[256] by raw byte, or max_ee:
    the largest expected number of errors).  Returns (stats QUAL_STATS_DTYPE[n], bin uint32[n]) — bin 0 passed, 1 failed: what
    demux_split_arrays takes with n_bins = 1 — and the number of records passed as a third with want_totals."""
    ctx = ctx or _lib.default_context()
    qual, qual_off = _lib.as_u8(qual), np.ascontiguousarray(qual_off, dtype=np.uint64)
    n = len(qual_off) - 1
    prm, weight = _select_table(dict(params), weight, max_ee, scale_bits)
    pad = np.zeros(1, dtype=np.uint8)
    stats, bins = np.zeros(max(1, n), dtype=_lib.QUAL_STATS_DTYPE), np.zeros(max(1, n), dtype=np.uint32)
    tot = (C.c_uint64 * 1)()
    _lib.check(_lib.lib().bg_fastq_qual_select(ctx.h, n, prm.ctypes.data, weight.ctypes.data if weight is not None else None,
                                               qual.ctypes.data if len(qual) else pad.ctypes.data, qual_off.ctypes.data, stats.ctypes.data,
                                               bins.ctypes.data, tot if want_totals else None), "bg_fastq_qual_select")
    return (stats[:n], bins[:n], int(tot[0])) if want_totals else (stats[:n], bins[:n])


def qual_select_dev(n, d_qual, d_qual_off, weight=None, max_ee=None, scale_bits=20, ctx=None, stream=0, want_stats=True, want_bin=True,
                    want_totals=False, out=None, **params):
    """bg_fastq_qual_select_dev on torch device tensors (weight is a host array).  Returns (d_stats uint8[n * 32] or None, d_bin
    int32[n] or None, passed): in HBM; `passed` is the number of records passed, or None without want_totals, and then the call
    does not synchronise.  `out`: the first two results of an earlier call of the same shape, to write into."""
    import torch
    ctx = ctx or _lib.default_context()
    prm, weight = _select_table(dict(params), weight, max_ee, scale_bits)
    if out is not None:
        d_stats, d_bin = out[:2]
    else:
        d_stats = torch.empty(max(1, n) * 32, dtype=torch.uint8, device=d_qual.device) if want_stats else None
        d_bin = torch.empty(max(1, n), dtype=torch.int32, device=d_qual.device) if want_bin else None
    tot = (C.c_uint64 * 1)()
    _lib.check(_lib.lib().bg_fastq_qual_select_dev(ctx.h, n, prm.ctypes.data, weight.ctypes.data if weight is not None else None,
                                                   d_qual.data_ptr(), d_qual_off.data_ptr(), d_stats.data_ptr() if d_stats is not None else None,
                                                   d_bin.data_ptr() if d_bin is not None else None, tot if want_totals else None, stream),
               "bg_fastq_qual_select_dev")
    return (d_stats[:n * 32] if d_stats is not None else None, d_bin[:n] if d_bin is not None else None,
            int(tot[0]) if want_totals else None)


def qc_tables_words(max_cycles):
    """bg_qc_tables_words: 64-bit words of the tables' buffer"""
    return int(_lib.lib().bg_qc_tables_words(int(max_cycles)))


class QcTables:
    """views into the one buffer of bg_fastq_qc_tables (a uint64 array, or an int64 device tensor): base[R, 5], qhist[R, 64],
    len_hist[R + 1], meanq_hist[64], n_reads[1], R = max_cycles + 1"""

    def __init__(self, buf, max_cycles):
        R = int(max_cycles) + 1
        self.buf, self.max_cycles = buf, int(max_cycles)
        self.base = buf[:R * 5].reshape(R, 5)
        self.qhist = buf[R * 5:R * 69].reshape(R, 64)
        self.len_hist = buf[R * 69:R * 70 + 1]
        self.meanq_hist = buf[R * 70 + 1:R * 70 + 65]
        self.n_reads = buf[R * 70 + 65:R * 70 + 66]


def qc_tables_arrays(seq, seq_off, qual, qual_off, max_cycles, first=0, step=1, phred_offset=33, ctx=None):
    """bg_fastq_qc_tables over host arrays: the tables of records first, first + step, ... as a QcTables of uint64 arrays"""
    ctx = ctx or _lib.default_context()
    seq, qual = _lib.as_u8(seq), _lib.as_u8(qual)
    seq_off, qual_off = np.ascontiguousarray(seq_off, dtype=np.uint64), np.ascontiguousarray(qual_off, dtype=np.uint64)
    pad = np.zeros(1, dtype=np.uint8)
    buf = np.zeros(qc_tables_words(max_cycles), dtype=np.uint64)
    _lib.check(_lib.lib().bg_fastq_qc_tables(ctx.h, len(seq_off) - 1, int(first), int(step), int(phred_offset), int(max_cycles),
                                             seq.ctypes.data if len(seq) else pad.ctypes.data, seq_off.ctypes.data,
                                             qual.ctypes.data if len(qual) else pad.ctypes.data, qual_off.ctypes.data, buf.ctypes.data),
               "bg_fastq_qc_tables")
    return QcTables(buf, max_cycles)


def qc_tables_dev(n, d_seq, d_seq_off, d_qual, d_qual_off, max_cycles, first=0, step=1, phred_offset=33, ctx=None, stream=0, out=None):
    """bg_fastq_qc_tables_dev on torch device tensors: a QcTables of views into one int64 tensor in HBM (the counts are
    unsigned), without synchronising.  `out`: the `buf` of an earlier result for the same max_cycles, to write into."""
    import torch
    ctx = ctx or _lib.default_context()
    buf = out if out is not None else torch.empty(qc_tables_words(max_cycles), dtype=torch.int64, device=d_seq.device)
    _lib.check(_lib.lib().bg_fastq_qc_tables_dev(ctx.h, n, int(first), int(step), int(phred_offset), int(max_cycles), d_seq.data_ptr(),
                                                 d_seq_off.data_ptr(), d_qual.data_ptr(), d_qual_off.data_ptr(), buf.data_ptr(), stream),
               "bg_fastq_qc_tables_dev")
    return QcTables(buf, max_cycles)


def qual_trim_arrays(recs, seq, seq_off, qual, qual_off, ctx=None, **params):
    """Quality trimming of host columns in one call: qual_cut_arrays, then myers.trim at the 3' end, then at the 5' end with
    the same records.  Returns (recs, seq, seq_off, qual, qual_off, cut records)."""
    from . import myers
    cut = qual_cut_arrays(qual, qual_off, ctx=ctx, **params)
    cols = myers.trim(_lib.TRIM_3P, cut, 1, recs, seq, seq_off, qual, qual_off, ctx=ctx)
    return (*myers.trim(_lib.TRIM_5P, cut, 1, *cols, ctx=ctx), cut)


# ---- writing ---------------------------------------------------------------------------------------------------------
def n_lines(n, first=0, step=1):
    """how many of n records `first, first + step, ...` are"""
    return (n - first - 1) // step + 1 if first < n else 0


def emit_arrays(parsed, first=0, step=1, ctx=None):
    """bg_fastq_emit over host arrays: `parsed` is a Parsed, or (text, recs, seq, qual) — the FASTQ text the ids point into
    and the columns of parse_arrays, myers.trim or filter_arrays.  Returns (text bytes, offsets uint64[m + 1]) of the records
    first, first + step, ..."""
    ctx = ctx or _lib.default_context()
    text, recs, seq, qual = (parsed.text, parsed.recs, parsed.seq, parsed.qual) if isinstance(parsed, Parsed) else parsed
    text, seq, qual = _lib.as_u8(text), _lib.as_u8(seq), _lib.as_u8(qual)
    recs = np.ascontiguousarray(recs, dtype=_lib.FQREC_DTYPE)
    n = len(recs)
    off = np.zeros(n_lines(n, first, step) + 1, dtype=np.uint64)
    total = C.c_uint64(0)
    args = (ctx.h, n, int(first), int(step), text.ctypes.data, recs.ctypes.data, seq.ctypes.data, qual.ctypes.data)
    _lib.check(_lib.lib().bg_fastq_emit(*args, None, 0, off.ctypes.data, C.byref(total)), "bg_fastq_emit")
    out = np.zeros(max(1, int(total.value)), dtype=np.uint8)
    _lib.check(_lib.lib().bg_fastq_emit(*args, out.ctypes.data, int(total.value), off.ctypes.data, C.byref(total)), "bg_fastq_emit")
    return out[:int(total.value)].tobytes(), off


def emit_dev(n, d_text, d_recs, d_seq, d_qual, first=0, step=1, ctx=None, stream=0, out=None):
    """bg_fastq_emit_dev on torch device tensors (d_text: the FASTQ text that was parsed; the other three as parse_dev,
    myers.trim_dev or filter_dev return them).  Returns (d_out uint8[total], d_off int64[m + 1], total) in HBM: a sizing call,
    then the writing one.  `out`: (d_out, d_off) to write into — one call; BiogpuError OPS_CAP if d_out is too small."""
    import torch
    ctx = ctx or _lib.default_context()
    total = C.c_uint64(0)
    args = (ctx.h, n, int(first), int(step), d_text.data_ptr(), d_recs.data_ptr(), d_seq.data_ptr(), d_qual.data_ptr())
    if out is not None:
        d_out, d_off = out
    else:
        d_off = torch.empty(n_lines(n, first, step) + 1, dtype=torch.int64, device=d_seq.device)
        _lib.check(_lib.lib().bg_fastq_emit_dev(*args, None, 0, d_off.data_ptr(), C.byref(total), stream), "bg_fastq_emit_dev")
        d_out = torch.empty(max(1, int(total.value)), dtype=torch.uint8, device=d_seq.device)
    _lib.check(_lib.lib().bg_fastq_emit_dev(*args, d_out.data_ptr(), int(d_out.numel()), d_off.data_ptr(), C.byref(total), stream),
               "bg_fastq_emit_dev")
    return d_out[:int(total.value)], d_off, int(total.value)


class Writer:
    """fastq::Writer (fastq.rs:528-599) into memory: records are collected and their text is written on the device, a batch
    at a time (bg_fastq_emit); getvalue() is what the reference's writer has written after flush()."""

    def __init__(self, ctx=None, batch=1 << 16):
        self._ctx, self._batch = ctx, batch
        self._pending, self._done = [], []

    def write(self, id, desc, seq, qual):  # fastq.rs:573-593
        self._pending.append((_bytes(id), None if desc is None else _bytes(desc), bytes(seq), bytes(qual)))
        if len(self._pending) >= self._batch:
            self.flush()

    def write_record(self, record):  # fastq.rs:568-570
        self.write(record._id, record._desc, record._seq, record._qual)

    def flush(self):  # fastq.rs:596-598
        if not self._pending:
            return
        recs = np.zeros(len(self._pending), dtype=_lib.FQREC_DTYPE)
        names, seqs, quals = [], [], []
        t = s = q = 0
        for k, (id_, desc, seq, qual) in enumerate(self._pending):
            r = recs[k]
            r["id_off"], r["id_len"] = t, len(id_)
            names.append(id_)
            t += len(id_)
            if desc is not None:
                r["has_desc"], r["desc_off"], r["desc_len"] = 1, t, len(desc)
                names.append(desc)
                t += len(desc)
            r["seq_off"], r["seq_len"], r["qual_off"], r["qual_len"] = s, len(seq), q, len(qual)
            seqs.append(seq)
            quals.append(qual)
            s += len(seq)
            q += len(qual)
        pad = b"\0"  # no empty buffers: the call refuses null pointers
        text, _ = emit_arrays((b"".join(names) + pad, recs, b"".join(seqs) + pad, b"".join(quals) + pad), ctx=self._ctx)
        self._done.append(text)
        self._pending = []

    def getvalue(self):
        self.flush()
        return b"".join(self._done)


def _bytes(s):
    return s.encode() if isinstance(s, str) else bytes(s)
