"""VCF text from candidate sites and indel events — host mirror of `bg_vcf_header` and `bg_vcf_emit[_dev]`
(rust-bio_amd/csrc/vcf_emit.hip; THE RULE is in include/biogpu.h): one VCF v4.3 data line for every SNV site of
`bam.sites_*` and every event of `bam.indels_*`, written on the device from the records those calls leave there, the reference
text and the contig table.  `vcf_bam` chains reading a BAM file, the two calls and the writer into a complete file.

rust-bio has no VCF writer.  This module only marshals arguments."""
import ctypes as C

import numpy as np

from . import _lib, bam

NONE = 2**64 - 1
THRESHOLDS = ("require", "exclude", "min_mapq", "min_baseq", "min_depth", "min_alt", "min_alt_permille", "min_alt_strand")


class VcfError(_lib.BiogpuError):
    """bg_vcf_emit[_dev] refused an element: `first_bad` is its index in the combined list (the sites at 0 .. n_sites - 1, event j
    at n_sites + j), None where no element is to blame"""

    def __init__(self, status, where, first_bad):
        super().__init__(status, where)
        self.first_bad = None if first_bad == NONE else int(first_bad)


def _check(rc, where, bad, totals):
    if rc == -1:
        raise VcfError(rc, where, bad.value)
    try:
        _lib.check(rc, where)
    except _lib.BiogpuError as e:
        e.totals = totals
        raise


def params():
    """bg_vcf_params_t: flags and reserved, both 0"""
    return np.zeros(1, dtype=_lib.VCF_PARAMS_DTYPE)


def header(contigs):
    """bg_vcf_header: ##fileformat, ##source, a ##contig line for every contig, the ##INFO lines and the #CHROM line, as bytes
    (host only)"""
    n = C.c_uint64(0)
    args = (contigs.table.ctypes.data if len(contigs) else None, len(contigs), contigs.names.ctypes.data)
    _lib.check(_lib.lib().bg_vcf_header(*args, None, 0, C.byref(n)), "bg_vcf_header")
    out = np.zeros(max(n.value, 1), dtype=np.uint8)
    _lib.check(_lib.lib().bg_vcf_header(*args, out.ctypes.data, n.value, C.byref(n)), "bg_vcf_header")
    return out[:n.value].tobytes()


def emit_dev(n_sites, d_sites, n_events, d_events, d_seq, n_seq, d_contigs, n_contigs, d_names, d_text, n_text, d_out=0, out_cap=0, d_line_off=0,
             stream=0, ctx=None):
    """bg_vcf_emit_dev (pointers are ints; d_out = 0 with out_cap = 0 sizes; d_line_off may be 0).  Returns (n_lines, out_bytes),
    read back with the call's one synchronisation of `stream`; the text is then written asynchronously.  Raises VcfError with
    the first refused element, BiogpuError with status -9 (OPS_CAP) when out_cap is too small (`totals` then holds both
    totals)."""
    ctx = ctx or _lib.default_context()
    prm = params()
    n_lines, total, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = _lib.lib().bg_vcf_emit_dev(ctx.h, prm.ctypes.data, d_sites or None, n_sites, d_events or None, n_events, d_seq or None, n_seq,
                                    d_contigs or None, n_contigs, d_names or None, d_text or None, n_text, d_out or None, out_cap,
                                    d_line_off or None, C.byref(n_lines), C.byref(total), C.byref(bad), stream)
    _check(rc, "bg_vcf_emit_dev", bad, (int(n_lines.value), int(total.value)))
    return int(n_lines.value), int(total.value)


def emit_arrays(sites, events, seq, contigs, text, ctx=None):
    """bg_vcf_emit, host buffers: `sites` (BAM_SITE_DTYPE[]) and `events` (BAM_INDEL_DTYPE[]) with the inserted bases `seq`, as
    `bam.sites_arrays` and `bam.indels_arrays` return them, against the index text `text` that contigs.table's `start`
    addresses.  Returns (text: bytes, line_off: uint64[n_lines + 1]).  Raises VcfError with the first refused element."""
    ctx = ctx or _lib.default_context()
    sites = np.ascontiguousarray(sites, dtype=_lib.BAM_SITE_DTYPE)
    events = np.ascontiguousarray(events, dtype=_lib.BAM_INDEL_DTYPE)
    seq, ref_text = _lib.as_u8(seq), _lib.as_u8(text)
    table = np.ascontiguousarray(contigs.table)
    prm = params()
    n_lines, total, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call(out, cap, line_off):
        rc = _lib.lib().bg_vcf_emit(ctx.h, prm.ctypes.data, sites.ctypes.data if len(sites) else None, len(sites),
                                    events.ctypes.data if len(events) else None, len(events), seq.ctypes.data if len(seq) else None, len(seq),
                                    table.ctypes.data if len(table) else None, len(table), contigs.names.ctypes.data if len(table) else None,
                                    ref_text.ctypes.data if len(ref_text) else None, len(ref_text), out, cap, line_off, C.byref(n_lines),
                                    C.byref(total), C.byref(bad))
        _check(rc, "bg_vcf_emit", bad, (int(n_lines.value), int(total.value)))
    call(None, 0, None)
    out = np.zeros(max(total.value, 1), dtype=np.uint8)
    line_off = np.zeros(n_lines.value + 1, dtype=np.uint64)
    call(out.ctypes.data, len(out), line_off.ctypes.data)
    return out[:total.value].tobytes(), line_off


def vcf_bam(data, text, regions=None, compress=False, ctx=None, left_align=None, **thresholds):
    """The VCF file of a coordinate-sorted BAM file (bytes) against `text`, FASTA text or a ready index text, as bytes: the header
    of `header`, then a line for every SNV site and every indel event of `regions` ((name or index, beg, end); None: every
    contig, whole).  `bam.read_bam`, `bam.resolve_regions`, then on the device `bam.sites_dev`, `bam.indels_dev` and `emit_dev`
    behind one another: sites, events and lines stay there, only their totals come back.  compress: the file as BGZF blocks
    with deflate-compressed payloads and the end-of-file block (`bam.bgzf_deflate_dev` over header plus body).  thresholds:
    those `bam.sites_params` and `bam.indels_params` share.  left_align: None takes the events as the records spell them
    (`bam.indels_dev`); an integer is the `max_shift` of `bam.indels_left_dev`, which shifts every indel to the left against the
    text before events are merged; True shifts without a limit."""
    import torch
    for k in thresholds:
        if k not in THRESHOLDS:
            raise TypeError(f"vcf_bam: no threshold {k!r}")
    ctx = ctx or _lib.default_context()
    _, contigs, stream, off = bam.read_bam(data, ctx=ctx)
    if regions is None:
        regions = [(c, 0, int(contigs.table["len"][c])) for c in range(len(contigs))]
    reg = bam.resolve_regions(contigs, regions)
    ref_text = bam._reference_text(text, contigs, ctx)
    head = header(contigs)
    dev = torch.device("cuda", ctx.device)
    st = torch.cuda.current_stream(dev).cuda_stream

    def up(a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return torch.from_numpy(a.copy() if len(a) else np.zeros(16, np.uint8)).to(dev)

    def room(nbytes):
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
    n_slots, n_contigs, n_regions, n_text = len(off) - 1, len(contigs), len(reg), len(ref_text)
    d_recs, d_off, d_contigs, d_names, d_text, d_reg = up(_lib.as_u8(stream)), up(off), up(contigs.table), up(contigs.names), up(ref_text), up(reg)
    front = (n_slots, d_recs.data_ptr(), d_off.data_ptr() if n_slots else 0, d_contigs.data_ptr() if n_contigs else 0, n_contigs)
    regs = (d_reg.data_ptr() if n_regions else 0, n_regions)
    text_args = (d_text.data_ptr() if n_text else 0, n_text)
    n_sites = bam.sites_dev(*front, *text_args, *regs, stream=st, ctx=ctx, **thresholds)
    d_sites = room(32 * n_sites)
    bam.sites_dev(*front, *text_args, *regs, d_sites.data_ptr(), n_sites, stream=st, ctx=ctx, **thresholds)
    if left_align is None:
        def indels(*out):
            return bam.indels_dev(*front, *regs, *out, stream=st, ctx=ctx, **thresholds)
    else:
        max_shift = 0xFFFFFFFF if left_align is True else int(left_align)

        def indels(*out):
            return bam.indels_left_dev(*front, *text_args, *regs, *out, stream=st, ctx=ctx, max_shift=max_shift, **thresholds)
    n_events, n_seq = indels()
    d_events, d_seq = room(40 * n_events), room(n_seq)
    indels(d_events.data_ptr(), n_events, d_seq.data_ptr(), n_seq)
    lists = (n_sites, d_sites.data_ptr() if n_sites else 0, n_events, d_events.data_ptr() if n_events else 0, d_seq.data_ptr() if n_seq else 0, n_seq,
             d_contigs.data_ptr() if n_contigs else 0, n_contigs, d_names.data_ptr() if n_contigs else 0, *text_args)
    _, body = emit_dev(*lists, stream=st, ctx=ctx)
    d_file = room(len(head) + body)
    d_file[:len(head)].copy_(torch.from_numpy(np.frombuffer(head, dtype=np.uint8).copy()))
    emit_dev(*lists, d_file.data_ptr() + len(head), body, stream=st, ctx=ctx)
    total = len(head) + body
    if compress:
        cap = bam.bgzf_deflate_dev(d_file.data_ptr(), total, 0, 0, bam.BGZF_EOF, stream=st, ctx=ctx)
        d_framed = room(cap)
        total = bam.bgzf_deflate_dev(d_file.data_ptr(), total, d_framed.data_ptr(), cap, bam.BGZF_EOF, stream=st, ctx=ctx)
        d_file = d_framed
    torch.cuda.current_stream(dev).synchronize()
    return d_file[:total].cpu().numpy().tobytes()
