"""The `_dev` entry points on caller pointers that are NOT the start of an allocation: every byte pointer at chosen residues
mod 16 between guard bytes (tests/dev_shift.py), on the inputs of tests/dev_align_cases.py.  Every call is compared with the
CPU oracle and with the same call made with all pointers at residue 0 (which names the culprit when only the shifted call
fails); every output's guard bytes must survive.  tests/test_dev_align_cases.py shows without a GPU that the inputs reach
the branches, and that the lines listed here still hold what is said of them.

What the kernels do through a caller's BYTE pointer that is wider than a byte, found by reading, with the guard in front of
it.  No access without one was found: nothing had to be fixed or refused.

bg_fastq_parse_dev (d_text 1 / 4 / 8 / 12 / 15, d_seq 0 / 5, d_qual 0 / 11; both with and without `fq_no_fused`)
  fastq_ingest.hip:42    load16: a 16-byte load of the text only if `aligned` (the text's address, decided at :57, :77 for the
                         general kernels and :648 for the one-pass kernel) and 16 bytes are left; else 16 byte loads.  Every d_text
                         residue tested is the byte half; the residue-0 twin is the vector half.
  fastq_ingest.hip:652   the halo in front of a tile and :660 the tile itself, :711 the windows of the search in front of a tile:
                         through load16.  A window starts at a multiple of 1024 of the text or at 0, so the `(wstart & 15) == 0`
                         half of :711 is always true: `aligned` alone decides.
  fastq_ingest.hip:296   F5's header scan: bytes up to the first 8-byte boundary OF THE ADDRESS, then :301 8-byte loads while 8 bytes
                         of the header are left, then bytes.  Headers begin at every address mod 8 (every d_text residue).
  fastq_ingest.hip:340   F6 copy_line: head bytes up to the destination's 16-byte boundary, then :364 16-byte stores; d_seq 5 and
                         d_qual 11 move the head.  :350 the source is read as five DWORD-aligned words from `pa = p - (p & 3)`
                         (:356) when they end inside the text (:353), else byte by byte; `pa` may lie up to 3 bytes in front of the
                         text — inside the aligned dword that holds its first byte, so the access cannot leave the caller's memory
                         page; those bytes are shifted out.  d_text 4 / 8 / 12 keep `sh` as at residue 0, 1 and 15 change it.
  fastq_ingest.hip:844   one-pass kernel, a header's two 8-byte words: from the LDS copy of the tile (filled through load16, so its
                         layout does not depend on the address), or (:850) from memory only if the word's address is 8-byte aligned
                         and both words lie inside the text — d_text 8 (and 0); at 1 / 4 / 12 / 15 the byte loop.  Reached by the
                         mid-lines text, whose headers lie more than the halo in front of the tile their record ends in.  (The
                         long-lines text makes the search of :711 run through all its windows and give up: a record of 40 KB
                         goes to the general kernels, whose gather then takes a wavefront per record.)
  fastq_ingest.hip:1005  one-pass gather: d0s / d0q from the sequence / quality output's own address; :1103 16-byte stores of whole
                         pieces on that alignment, partial pieces byte by byte.
bg_pack2_dev (d_bytes 0 .. 15)
  pack2.hip:21           one 16-byte load (:22) for a whole word at an aligned address, else up to 16 byte loads.  Residue 0: vector
                         for whole words; 1 .. 15: bytes for every word.  bg_unpack2_dev stores bytes.
bg_fasta_reference_dev (output 0 / 1 / 8 / 15, inputs 0 / 3)
  fasta_ingest.hip:628   16 output bytes as one store (:629) only for a whole piece at an aligned `out`, else byte stores.  The
                         record text and sequences are read byte by byte.
bg_align_batch_dev (d_x, d_y 0 / 1 / 7; d_ops 0 .. 3 with strides 324 and 325)
  sw_traceback.hip:116   dword_ok from the address of the END of a pair's slot: four operations per (:123) dword store, else byte
                         stores.  Stride 324: all pairs dword at d_ops 0, none at 1 / 2 / 3; stride 325: both in every call.  The
                         fill kernels read x and y byte by byte.
bg_align_banded_batch_dev (d_x, d_y 0 / 1 / 9 / 15)
  band_device.hip:45     stage_bytes: `mis` bytes up to the first 16-byte boundary of the source, then (:49) 16-byte loads of whole
                         vectors, then bytes.
bg_seed_extend_strands_batch_dev, bg_seed_extend_tiered_batch_dev (d_reads 0 / 3 / 8 / 13, d_ops 0 / 5, index text 0 / 6)
  seed_tiered.hip:83     copy_wave: bytes unless source (the call's scratch slot) and destination (the caller's) agree mod 16; then
                         (:87) head bytes up to the destination's boundary and (:90) 16-byte loads / stores.  d_ops 0: both kinds
                         among the re-seeded reads; d_ops 5: bytes only.  Reads and text are read byte by byte; the traceback's
                         stores are those of sw_traceback.hip:116.
bg_sam_emit_batch_dev, bg_sam_sort_dev (output 0 / 1 / 15, input columns 0 / 7)
  sam_emit.hip:384       `mis` of a line's address in the output: the line is formatted at that offset of an LDS buffer, and (:394)
                         copied out with 16-byte stores between its first and last boundary, bytes outside; the id, sequence and
                         quality columns are read byte by byte.
  sam_rule.h:204         sam_copy_line: head / body / tail from the destination's address; (:211) 16-byte stores of the body, each
                         put together by sam_copy_vec (:178): one aligned load when source and destination agree mod 16 (:181), else
                         two aligned loads when both lie inside the line (:182), else bytes.
bg_revcomp_batch_dev, bg_cigar_batch_dev, bg_fastq_trim_dev, bg_fastq_filter_dev, bg_fastq_demux_split_dev, bg_fastq_qual_cut_dev
                         byte loads and stores only through the byte pointers (align_text.hip, fastq_trim.hip, fastq_emit.hip,
                         fastq_demux.hip, fastq_qual.hip): no branch on an address."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import dev_align_cases as dc
import oracle_py as orc
from dev_shift import guards_intact, shifted, shifted_from
from rust_bio_amd import _lib, fasta, fastq, myers, pack2, sam
from rust_bio_amd.pairwise import Aligner, Scoring

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (file, line, what the line must still contain): checked against the sources by tests/test_dev_align_cases.py
ACCESSES = [
    ("fastq_ingest.hip", 42, "if (aligned && base + 16 <= len) return *(const uint4*)(t + base);"),
    ("fastq_ingest.hip", 57, "load16(t, len, base, ((uintptr_t)t & 15) == 0)"),
    ("fastq_ingest.hip", 77, "load16(t, len, b0, ((uintptr_t)t & 15) == 0)"),
    ("fastq_ingest.hip", 296, "while (sp < n && ((uintptr_t)(p + sp) & 7))"),
    ("fastq_ingest.hip", 301, "*(const uint64_t*)(p + sp)"),
    ("fastq_ingest.hip", 340, "min(n, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15))"),
    ("fastq_ingest.hip", 350, "const uint32_t sh = (uint32_t)((uintptr_t)p & 3);"),
    ("fastq_ingest.hip", 353, "if (pa + 20 <= t_end)"),
    ("fastq_ingest.hip", 356, "r[q] = *(const uint32_t*)(pa + 4 * q);"),
    ("fastq_ingest.hip", 364, "*(uint4*)(dst + head + 16 * j) ="),
    ("fastq_ingest.hip", 648, "const bool aligned = ((uintptr_t)a.t & 15) == 0;"),
    ("fastq_ingest.hip", 652, "hv = load16(a.t, t0, t0 - kHaloBytes + (uint64_t)lane * 16, aligned);"),
    ("fastq_ingest.hip", 660, "load16(a.t, a.len, base, aligned)"),
    ("fastq_ingest.hip", 711, "load16(a.t, end, base, aligned && (wstart & 15) == 0)"),
    ("fastq_ingest.hip", 844, "const bool h2 = h_lds || (((uintptr_t)hw & 7) == 0 && (const uint8_t*)hw >= a.t && (const uint8_t*)(hw + 2) <= a.t + a.len);"),
    ("fastq_ingest.hip", 850, "w0 = hw[0];"),
    ("fastq_ingest.hip", 1005, "const uint32_t d0s = (uint32_t)((uintptr_t)seq_base & 15), d0q = (uint32_t)((uintptr_t)qual_base & 15);"),
    ("fastq_ingest.hip", 1103, "*(uint4*)(dst_base + o_lo) ="),
    ("pack2.hip", 21, "if (s0 + 16 <= n && ((uintptr_t)(in + s0) & 15) == 0) {"),
    ("pack2.hip", 22, "const uint4 v = *(const uint4*)(in + s0);"),
    ("fasta_ingest.hip", 628, "if (cnt == 16 && ((uintptr_t)out & 15) == 0) {"),
    ("fasta_ingest.hip", 629, "*(uint4*)(out + q0) ="),
    ("sw_traceback.hip", 116, "const bool dword_ok = ops_end && (((uintptr_t)ops_end & 3) == 0);"),
    ("sw_traceback.hip", 123, "if ((n_ops & 3) == 0) *(uint32_t*)(ops_end - n_ops) = acc;"),
    ("band_device.hip", 45, "const uint32_t mis = (uint32_t)((uintptr_t)src & 15u);"),
    ("band_device.hip", 49, "const uint4* s4 = (const uint4*)(src + headb);"),
    ("seed_tiered.hip", 83, "if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) != 0) {"),
    ("seed_tiered.hip", 87, "const uint32_t head = min(n, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15));"),
    ("seed_tiered.hip", 90, "const uint4* s16 = (const uint4*)(src + head);"),
    ("sam_emit.hip", 384, "const uint32_t mis = (uint32_t)((uintptr_t)line & 15);"),
    ("sam_emit.hip", 394, "*(uint4*)(line + head + 16 * i) = *(const uint4*)(stage + head + 16 * i);"),
    ("sam_rule.h", 178, "const uint32_t sh = (uint32_t)((uintptr_t)p & 15u);"),
    ("sam_rule.h", 181, "if (sh == 0) return *(const sam_v16*)q;"),
    ("sam_rule.h", 182, "if (q >= lb && q + 32 <= le) {"),
    ("sam_rule.h", 204, "sam_copy_plan((uint32_t)((uintptr_t)dst & 15u), len)"),
    ("sam_rule.h", 211, "*(sam_v16*)(dst + p.head + 16 * v) = sam_copy_vec("),
]


def stream():
    return torch.cuda.current_stream().cuda_stream


def host(view, dtype=np.uint8):
    """the bytes of a device view as a numpy array of `dtype`"""
    torch.cuda.synchronize()
    return view.cpu().numpy().view(dtype)


def typed(a, residue=0):
    """a numpy array of any dtype on the device, at a residue that is a multiple of its item size"""
    a = np.ascontiguousarray(a)
    assert residue % min(a.dtype.alignment, 16) == 0
    return shifted_from(a, residue)


def i64(a):
    return typed(np.ascontiguousarray(a).astype(np.int64))


@pytest.fixture(scope="module")
def no_fused_ctx():
    ctx = _lib.Context(0)
    ctx.set_option("fq_no_fused", 1)
    yield ctx
    ctx.close()


# ---- bg_fastq_parse_dev -------------------------------------------------------------------------------------------------------
def fq_call(ctx, text, r_text, r_seq, r_qual):
    """-> (records, status, err_pos, recs bytes, seq_off, qual_off, seq, qual) of one call, its five outputs between guards"""
    n, cap = len(text), len(text) // 4 + 2
    d_text = shifted_from(text, r_text)
    outs = (shifted(cap * 56, 0), shifted(n, r_seq), shifted(n, r_qual), shifted((cap + 1) * 8, 0), shifted((cap + 1) * 8, 0))
    k, status, err_pos = fastq.parse_dev(d_text, ctx=ctx, stream=stream(), bufs=outs)[:3]
    assert all(guards_intact(o) for o in outs), ("a write outside an output", r_text, r_seq, r_qual)
    assert host(d_text).tobytes() == text
    recs = host(outs[0], _lib.FQREC_DTYPE)[:k]
    so, qo = host(outs[3], np.uint64)[:k + 1], host(outs[4], np.uint64)[:k + 1]
    return (k, status, err_pos, recs.tobytes(), so.tobytes(), qo.tobytes(), host(outs[1])[:int(so[k])].tobytes(),
            host(outs[2])[:int(qo[k])].tobytes())


def fq_same_as_oracle(text, got, want):
    wrecs, wstatus, wpos = want
    k, status, err_pos, recs, so, qo, seq, qual = got
    t = np.frombuffer(text, np.uint8)
    p = fastq.Parsed(t, np.frombuffer(recs, _lib.FQREC_DTYPE), np.frombuffer(seq, np.uint8), np.frombuffer(so, np.uint64),
                     np.frombuffer(qual, np.uint8), np.frombuffer(qo, np.uint64), fastq.STATUS.index(status), err_pos)
    assert (status, k) == (wstatus, len(wrecs))
    for i, w in enumerate(wrecs):
        r = p.record(i)
        assert (r._id, r._desc, r._seq, r._qual, fastq.CHECK[r._check]) == (w["id"], w["desc"], w["seq"], w["qual"], w["check"]), i


@functools.lru_cache(maxsize=None)
def fq_oracle(name):
    return orc.fastq_parse(dc.fastq_texts()[name][0])


@pytest.mark.parametrize("path", ["one-pass", "general"])
@pytest.mark.parametrize("name", sorted(dc.fastq_texts()))
def test_fastq_parse(name, path, no_fused_ctx):
    text, n = dc.fastq_texts()[name]
    ctx = no_fused_ctx if path == "general" else _lib.default_context()
    base = fq_call(ctx, text, 0, 0, 0)
    assert base[0] == n
    fq_same_as_oracle(text, base, fq_oracle(name))
    for r_text in dc.FQ_TEXT_RES:
        for r_seq in dc.FQ_SEQ_RES:
            for r_qual in dc.FQ_QUAL_RES:
                got = fq_call(ctx, text, r_text, r_seq, r_qual)
                if got != base:  # say what differs, against the oracle
                    fq_same_as_oracle(text, got, fq_oracle(name))
                assert got == base, (name, path, r_text, r_seq, r_qual)


# ---- bg_pack2_dev, bg_unpack2_dev ---------------------------------------------------------------------------------------------
CODES = (C.c_uint8 * 4)(*pack2.DNA_CODES)


def pack_call(data, r_in, r_out):
    """pack at r_in, unpack the result to r_out -> (words, invalid count, unpacked bytes)"""
    n, ctx, L = len(data), _lib.default_context(), _lib.lib()
    n_words = (n + 15) // 16
    d_in, d_packed, d_bad = shifted_from(data, r_in), shifted(4 * n_words, 0), shifted(8, 0)
    d_bad.zero_()
    _lib.check(L.bg_pack2_dev(ctx.h, d_in.data_ptr(), n, CODES, d_packed.data_ptr(), d_bad.data_ptr(), stream()), "bg_pack2_dev")
    d_out = shifted(n, r_out)
    _lib.check(L.bg_unpack2_dev(ctx.h, d_packed.data_ptr(), n, CODES, d_out.data_ptr(), stream()), "bg_unpack2_dev")
    assert guards_intact(d_packed) and guards_intact(d_bad) and guards_intact(d_out), (n, r_in, r_out)
    return host(d_packed, np.uint32).copy(), int(host(d_bad, np.uint64)[0]), host(d_out).tobytes()


@pytest.mark.parametrize("n", dc.PACK_N)
def test_pack2(n):
    for name, data, bad in dc.pack_inputs(n):
        want = pack2.pack_numpy(np.frombuffer(data, np.uint8))[:-1]
        back = data.replace(bytes([dc.INVALID]), b"A")
        for r in dc.PACK_RES:
            words, n_bad, unpacked = pack_call(data, r, (r + 5) % 16)
            assert (words == want).all(), (n, name, r, np.flatnonzero(words != want)[:4])
            assert n_bad == bad and unpacked == back, (n, name, r)


# ---- bg_fasta_reference_dev ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_parsed():
    from test_gpu_fasta import REF_TEXT
    d_fa = torch.from_numpy(np.frombuffer(REF_TEXT, np.uint8).copy()).to(DEV)
    n, status, _, d_recs, d_seq, d_so = fasta.parse_dev(d_fa)
    assert status == "ok"
    return REF_TEXT, n, d_recs, host(d_seq)[:int(host(d_so, np.int64)[n])].tobytes()


def ref_call(flags, r_in, r_out):
    text, n, d_recs, seq = ref_parsed()
    ctx, L = _lib.default_context(), _lib.lib()
    d_fa, d_seq = shifted_from(text, r_in), shifted_from(seq, r_in)
    nt, nb, bad = (C.c_uint64(0) for _ in range(3))
    tail = (C.byref(nt), C.byref(nb), C.byref(bad), stream())
    front = (ctx.h, n, d_recs.data_ptr(), d_fa.data_ptr(), d_seq.data_ptr(), flags)
    _lib.check(L.bg_fasta_reference_dev(*front, None, 0, None, None, 0, *tail), "bg_fasta_reference_dev")
    d_out, d_tab, d_names = shifted(nt.value, r_out), shifted(n * 32, 0), shifted(nb.value, r_out)
    _lib.check(L.bg_fasta_reference_dev(*front, d_out.data_ptr(), nt.value, d_tab.data_ptr(), d_names.data_ptr(), nb.value, *tail),
               "bg_fasta_reference_dev")
    assert guards_intact(d_out) and guards_intact(d_tab) and guards_intact(d_names), (flags, r_in, r_out)
    return host(d_out).tobytes(), host(d_tab).tobytes(), host(d_names).tobytes()


@pytest.mark.parametrize("flags", [0, fasta.REF_FMD, fasta.REF_UPPER, fasta.REF_FMD | fasta.REF_UPPER])
def test_fasta_reference(flags):
    import fasta_oracle as fo
    records, status, _ = fo.parse(ref_parsed()[0])
    want, contigs = fo.reference(records, fmd=bool(flags & fasta.REF_FMD), upper=bool(flags & fasta.REF_UPPER))
    base = ref_call(flags, 0, 0)
    assert base[0] == want.tobytes()
    table = sam.Contigs.from_arrays(np.frombuffer(base[1], _lib.SAM_CONTIG_DTYPE), np.frombuffer(base[2], np.uint8))
    assert [(table.name(c), int(table.table["start"][c]), int(table.table["len"][c])) for c in range(len(table))] == contigs
    for r_in in dc.REF_IN_RES:
        for r_out in dc.REF_OUT_RES:
            got = ref_call(flags, r_in, r_out)
            assert got[0] == want.tobytes(), (flags, r_in, r_out)
            assert got == base, (flags, r_in, r_out)


# ---- bg_align_batch_dev, bg_cigar_batch_dev -----------------------------------------------------------------------------------
MODES = {"local": 3, "semiglobal": 2}
FILL = 0xA5  # of operation slots: no operation code, so that a byte a copy leaves out shows


@functools.lru_cache(maxsize=None)
def sw_arrays():
    xs, ys = dc.sw_pairs()
    return _lib.concat(xs) + _lib.concat(ys)


@functools.lru_cache(maxsize=None)
def sw_oracle(mode):
    from test_gpu_pk16 import CLIPS
    x, xo, y, yo = sw_arrays()
    return orc.align_batch(orc.make_scoring(**dc.SW_SCORES, **CLIPS), mode, x, xo, y, yo, threads=8)


def sw_call(al, mode, r_x, r_y, r_ops, stride):
    """-> (records, operation slots) with the slots between guards"""
    x, xo, y, yo = sw_arrays()
    n = dc.SW_PAIRS
    d_x, d_y, d_xo, d_yo = shifted_from(x, r_x), shifted_from(y, r_y), i64(xo), i64(yo)
    d_out, d_ops = shifted(n * 64, 0), shifted(n * stride, r_ops, fill=FILL)
    al.align_dev(MODES[mode], n, d_x.data_ptr(), d_xo.data_ptr(), d_y.data_ptr(), d_yo.data_ptr(), dc.SW_M, dc.SW_N, d_out.data_ptr(),
                 d_ops.data_ptr(), stride, stream())
    assert guards_intact(d_out) and guards_intact(d_ops), (mode, r_x, r_y, r_ops, stride)
    return host(d_out, _lib.ALN_DTYPE).copy(), host(d_ops).copy()


def sw_same_as_oracle(mode, stride, rec, ops):
    from rust_bio_amd.pairwise import decode_ops
    oout, oops, ostride = sw_oracle(mode)
    for f in ("score", "xstart", "xend", "ystart", "yend", "xlen", "ylen", "n_ops"):
        assert (rec[f].astype(np.int64) == oout[f].astype(np.int64)).all(), (mode, f)
    assert (rec["status"] == 0).all()
    assert (rec["ops_off"] == (np.arange(len(rec), dtype=np.uint64) + 1) * stride - rec["n_ops"]).all()
    for p in range(len(rec)):
        assert decode_ops(rec[p], ops) == orc.decode_ops(oops[p * ostride:p * ostride + int(oout["n_ops"][p])]), (mode, p)
        assert (ops[p * stride:int(rec["ops_off"][p])] == FILL).all(), (mode, p, "bytes in front of the operations were written")


@pytest.mark.parametrize("kernel", ["k1p", "no_pk16"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_align_batch(mode, kernel):
    ctx = _lib.Context(0)
    ctx.set_option("no_pk16", int(kernel == "no_pk16"))
    al = Aligner.with_scoring(Scoring.from_scores(*(dc.SW_SCORES[k] for k in ("gap_open", "gap_extend", "match", "mismatch"))), ctx=ctx)
    try:
        for stride in dc.SW_STRIDES:
            rec0, ops0 = sw_call(al, mode, 0, 0, 0, stride)
            packed = bool(ctx.last_fill_kernels() & (_lib.FILL["K1P"] | _lib.FILL["K1P_LF"]))
            assert packed == (kernel == "k1p"), (mode, kernel, ctx.last_fill_kernels())
            sw_same_as_oracle(mode, stride, rec0, ops0)
            for r_ops in dc.SW_OPS_RES:
                for r_x in dc.SW_SEQ_RES:
                    for r_y in dc.SW_SEQ_RES:
                        rec, ops = sw_call(al, mode, r_x, r_y, r_ops, stride)
                        if rec.tobytes() != rec0.tobytes() or ops.tobytes() != ops0.tobytes():
                            sw_same_as_oracle(mode, stride, rec, ops)
                        assert rec.tobytes() == rec0.tobytes() and ops.tobytes() == ops0.tobytes(), (mode, kernel, stride, r_x, r_y, r_ops)
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def cigar_jobs():
    """70 alignments of the pairwise case: the 37 local ones and 33 semiglobal ones, their operations in one buffer"""
    al = Aligner.with_scoring(Scoring.from_scores(-5, -1, 1, -1))
    x, xo, y, yo = sw_arrays()
    recs, bufs, at = [], [], 0
    for mode, count in ((3, 37), (2, 33)):
        out, ops = al.align_arrays(mode, x, xo, y, yo)
        out = out[:count].copy()
        out["ops_off"] += at
        recs.append(out)
        bufs.append(ops)
        at += len(ops)
    return np.concatenate(recs), np.concatenate(bufs)


@pytest.mark.parametrize("hard_clip", [0, 1])
def test_cigar_batch(hard_clip):
    recs, ops = cigar_jobs()
    n, stride = len(recs), 2 * int(recs["n_ops"].max()) + 32
    assert n == 70
    want = [orc.cigar({"xstart": int(r["xstart"]), "xend": int(r["xend"]), "xlen": int(r["xlen"]), "mode": int(r["mode"])},
                      ops[int(r["ops_off"]):int(r["ops_off"]) + int(r["n_ops"])].astype(np.uint64), bool(hard_clip)) for r in recs]
    assert len(set(want)) >= 30
    base = None
    for r_in in dc.TEXT_RES:
        for r_out in dc.TEXT_RES:
            d_aln, d_ops = typed(recs), shifted_from(ops, r_in)
            d_out, d_len = shifted(n * stride, r_out), shifted(n * 4, 0)
            _lib.check(_lib.lib().bg_cigar_batch_dev(_lib.default_context().h, n, d_aln.data_ptr(), d_ops.data_ptr(), hard_clip, d_out.data_ptr(),
                                                     stride, d_len.data_ptr(), stream()), "bg_cigar_batch_dev")
            assert guards_intact(d_out) and guards_intact(d_len), (r_in, r_out)
            out, lens = host(d_out), host(d_len, np.int32)
            got = [out[p * stride:p * stride + int(lens[p])].tobytes().decode() for p in range(n)]
            assert got == want, (hard_clip, r_in, r_out)
            slots = out.tobytes()
            base = base or slots
            assert slots == base, (hard_clip, r_in, r_out)  # the bytes behind a CIGAR stay the fill, too


# ---- bg_revcomp_batch_dev -------------------------------------------------------------------------------------------------------
def test_revcomp_batch():
    from rust_bio_amd.pipeline import revcomp_dev
    seqs = dc.revcomp_seqs()
    buf, off = dc.fc.concat(seqs)
    want = b"".join(dc.fc.revcomp(s) for s in seqs)
    for r_in in dc.TEXT_RES:
        for r_out in dc.TEXT_RES:
            d_in, d_off, d_out = shifted_from(buf, r_in), i64(off), shifted(len(buf), r_out)
            revcomp_dev(len(seqs), d_in.data_ptr(), d_off.data_ptr(), d_out.data_ptr(), stream=stream())
            assert guards_intact(d_out), (r_in, r_out)
            assert host(d_out).tobytes() == want, (r_in, r_out)


# ---- bg_align_banded_batch_dev ------------------------------------------------------------------------------------------------
def test_align_banded_batch(capfd, monkeypatch):
    import band_edge_cases as bec
    from rust_bio_amd.banded import Aligner as BandedAligner
    from test_gpu_band_builder_edges import MODE, assert_same_records
    monkeypatch.setenv("BG_TRACE", "1")
    pairs = dc.band_pairs()
    al = BandedAligner.with_scoring(Scoring.from_scores(-5, -1, 1, -1), bec.K, bec.W)
    x, xo = _lib.concat([p.x for p in pairs])
    y, yo = _lib.concat([p.y for p in pairs])
    al.ctx.set_option("band_on_host", 1)
    try:
        out_h, ops_h = al.align_arrays(MODE, x, xo, y, yo)
        host_run = (out_h.copy(), ops_h.copy(), al.last_cells.copy())
    finally:
        al.ctx.set_option("band_on_host", 0)
    assert (out_h["status"] == 0).all()
    n = len(pairs)
    stride = int(np.diff(xo).max() + np.diff(yo).max()) + 8
    base = None
    for r_x in dc.BAND_RES:
        for r_y in dc.BAND_RES:
            d_x, d_y, d_xo, d_yo = shifted_from(x, r_x), shifted_from(y, r_y), i64(xo), i64(yo)
            d_out, d_ops = shifted(n * 64, 0), shifted(n * stride, 0, fill=FILL)
            capfd.readouterr()
            cells = al.align_dev(MODE, n, d_x.data_ptr(), d_xo.data_ptr(), d_y.data_ptr(), d_yo.data_ptr(), d_out.data_ptr(), d_ops.data_ptr(),
                                 stride, want_cells=True)
            err = capfd.readouterr().err
            assert "band build (device)" in err and "rebuilt on the host" not in err, err
            assert guards_intact(d_out) and guards_intact(d_ops), (r_x, r_y)
            rec, ops = host(d_out, _lib.ALN_DTYPE).copy(), host(d_ops).copy()
            assert_same_records((rec, ops, cells), host_run, (r_x, r_y), ops_off=False)
            got = (rec.tobytes(), ops.tobytes(), cells.tobytes())
            base = base or got
            assert got == base, (r_x, r_y)


# ---- bg_seed_extend_strands_batch_dev, bg_seed_extend_tiered_batch_dev --------------------------------------------------------
SC = Scoring.from_scores(-5, -1, 1, -1)


@functools.lru_cache(maxsize=None)
def strands_index():
    """a plain FM index over T$ and the oracle's tables of it"""
    from test_gpu_pipeline import build
    text = np.frombuffer(dc.seed_genome() + b"$", np.uint8)
    sa, b, ls, fm = build(text, 8)
    return text, sa, b, ls, fm


@functools.lru_cache(maxsize=None)
def strands_oracle():
    from test_gpu_seed_extend_strands import oracle_strands
    text = np.frombuffer(dc.seed_genome() + b"$", np.uint8)
    sa = np.asarray(orc.suffix_array(text), np.uint64)
    b = np.frombuffer(bytes(orc.bwt(text, sa)), np.uint8)
    from test_gpu_pipeline import ALPHA
    ls = np.asarray(orc.less(b, ALPHA), np.uint64)
    buf, off, _ = dc.seed_reads()
    return oracle_strands(b, ls, sa, text, len(text) - 1, buf, off)


def seed_buffers(r_reads, r_ops, tier=False):
    buf, off, _ = dc.seed_reads()
    n = dc.SEED_READS
    d = types.SimpleNamespace(reads=shifted_from(buf, r_reads), off=i64(off), hits=shifted(n * 96, 0), strand=shifted(n, 0, fill=77),
                              ops=shifted(n * dc.SEED_STRIDE, r_ops, fill=FILL), tier=shifted(n, 0, fill=77) if tier else None)
    return d


def seed_results(d):
    outs = [d.hits, d.strand, d.ops] + ([d.tier] if d.tier is not None else [])
    assert all(guards_intact(o) for o in outs)
    return tuple(host(o).tobytes() for o in outs)


def test_seed_extend_strands():
    from rust_bio_amd.pipeline import SeedParams, attach_text, seed_extend_strands_dev
    from test_gpu_pipeline import compare
    text, sa, b, ls, fm = strands_index()
    ohits, ostrand, oops, ostride = strands_oracle()
    base = None
    for r_text in dc.SEED_TEXT_RES:
        d_text = shifted_from(text, r_text)
        attach_text(fm, d_text=d_text)
        for r_reads in dc.SEED_READS_RES:
            for r_ops in dc.SEED_OPS_RES:
                d = seed_buffers(r_reads, r_ops)
                tot = np.zeros(2, dtype=np.uint64)
                seed_extend_strands_dev(fm, SC, dc.SEED_READS, d.reads.data_ptr(), d.off.data_ptr(), dc.SEED_LEN, d.hits.data_ptr(),
                                        d.strand.data_ptr(), d.ops.data_ptr(), dc.SEED_STRIDE, SeedParams(20, 10, 16, dc.SEED_PAD), 3, stream(), tot)
                got = seed_results(d)
                if base is None:
                    hits = np.frombuffer(got[0], _lib.SEED_HIT_DTYPE)
                    compare(hits, np.frombuffer(got[2], np.uint8), ohits, oops, ostride)
                    assert (np.frombuffer(got[1], np.uint8) == ostrand).all()
                    base = got
                assert got == base, (r_text, r_reads, r_ops)
    assert host(d_text).tobytes() == text.tobytes()


def test_seed_extend_tiered():
    import test_gpu_seed_extend_tiered as t
    import tiered_seed_oracle as tso
    from rust_bio_amd.pipeline import attach_text, seed_extend_tiered_dev
    buf, off, planted = dc.seed_reads()
    res = t.oracle(dc.seed_genome(), buf, off, reseed_below=dc.SEED_BELOW)
    fm = t.device_index(dc.seed_genome())
    text = np.frombuffer(dc.fc.full_text(dc.seed_genome()), np.uint8)
    n, base = dc.SEED_READS, None
    try:
        for r_text in dc.SEED_TEXT_RES:
            d_text = shifted_from(text, r_text)
            attach_text(fm, d_text=d_text)
            for r_reads in dc.SEED_READS_RES:
                for r_ops in dc.SEED_OPS_RES:
                    d = seed_buffers(r_reads, r_ops, tier=True)
                    tot = np.zeros(3, dtype=np.uint64)
                    seed_extend_tiered_dev(fm, SC, n, d.reads.data_ptr(), d.off.data_ptr(), dc.SEED_LEN, d.hits.data_ptr(), d.strand.data_ptr(),
                                           d.tier.data_ptr(), d.ops.data_ptr(), dc.SEED_STRIDE, t.params(reseed_below=dc.SEED_BELOW), 3, stream(), tot)
                    raw = seed_results(d)
                    hits, strand, ops, tier = (np.frombuffer(b_, dt) for b_, dt in zip(raw, (_lib.SEED_HIT_DTYPE, np.uint8, np.uint8, np.uint8)))
                    got = dict(hits=hits, strand=strand, tier=tier, ops=ops, stride=dc.SEED_STRIDE, totals=tot, status=0)
                    if base is None or raw != base:
                        t.check(got, res, (r_text, r_reads, r_ops))
                    base = base or raw
                    assert raw == base, (r_text, r_reads, r_ops)
        assert (tier[planted] == tso.TIER_SECOND).all()
    finally:
        fm.close()


# ---- bg_sam_emit_batch_dev, bg_sam_sort_dev -----------------------------------------------------------------------------------
def test_sam_emit():
    import sam_oracle as so
    from test_gpu_sam_emit_edges import index, same
    fm, case = index(), dc.sam_case()
    want = case.want()
    total = sum(len(w) for w in want)
    table = sam.Contigs(case.contigs)
    n = case.n
    fixed = [typed(a) for a in (table.table, table.names, case.fq.recs, case.hits, case.strand, case.ops)]
    d_table, d_names, d_recs, d_hits, d_strand, d_ops = (a.data_ptr() for a in fixed)
    for r_in in dc.SAM_IN_RES:
        d_fq, d_seq, d_qual = (shifted_from(np.ascontiguousarray(a), r_in) for a in (case.fq.text, case.fq.seq, case.fq.qual))
        for r_out in dc.SAM_OUT_RES:
            d_out, d_off = shifted(total, r_out), shifted((n + 1) * 8, 0)
            got = sam.emit_dev(fm, sam.SamParams(case.flags, 1), n, d_table, len(table), d_names, d_fq.data_ptr(), d_recs, d_seq.data_ptr(),
                               d_qual.data_ptr(), d_hits, d_strand, d_ops, d_out.data_ptr(), total, d_off.data_ptr(), stream=stream())
            assert got == total and guards_intact(d_out) and guards_intact(d_off), (r_in, r_out)
            same(want, host(d_out).tobytes(), host(d_off, np.uint64), (r_in, r_out))
    assert (so.offsets(want) == host(d_off, np.uint64)).all()


def test_sam_sort():
    import sam_oracle as so
    import sam_sort_oracle as sso
    b = dc.sort_batch()
    perm, out_off, want = sso.sort(b.key, b.recs)
    text, in_off = b"".join(b.recs), so.offsets(b.recs)
    n, nbytes = len(b.recs), len(text)
    d_key, d_in_off = typed(b.key), typed(in_off)
    for r_in in dc.SAM_IN_RES:
        d_in = shifted_from(text, r_in)
        for r_out in dc.SAM_OUT_RES:
            d_out, d_out_off, d_perm = shifted(nbytes, r_out), shifted((n + 1) * 8, 0), shifted(n * 8, 0)
            sam.sort_dev(n, d_key.data_ptr(), d_in.data_ptr(), d_in_off.data_ptr(), nbytes, d_out.data_ptr(), nbytes, d_out_off.data_ptr(),
                         d_perm.data_ptr(), stream=stream())
            assert guards_intact(d_out) and guards_intact(d_out_off) and guards_intact(d_perm), (r_in, r_out)
            assert (host(d_perm, np.uint64) == perm).all() and (host(d_out_off, np.uint64) == out_off).all(), (r_in, r_out)
            out = host(d_out).tobytes()
            for j in range(n):  # name the first record that differs
                a, e = int(out_off[j]), int(out_off[j + 1])
                assert out[a:e] == want[a:e], (r_in, r_out, j, int(perm[j]), e - a)


# ---- bg_fastq_trim_dev, bg_fastq_filter_dev, bg_fastq_demux_split_dev, bg_fastq_qual_cut_dev -----------------------------------
CUT_PARAMS = [dict(method_5p=0, method_3p=1, cutoff_5p=0, cutoff_3p=20, window=0), dict(method_5p=1, method_3p=2, cutoff_5p=20, cutoff_3p=20, window=4)]


class Columns:
    """a fastq_write_cases.Batch on the device: sequences and qualities at a residue, the typed columns at 0"""

    def __init__(self, batch, residue):
        self.n = len(batch)
        self.recs, self.so, self.qo = typed(batch.recs), i64(batch.seq_off), i64(batch.qual_off)
        self.seq, self.qual = shifted_from(batch.seq + b"#", residue), shifted_from(batch.qual + b"#", residue)

    def outputs(self, residue):
        """(recs, seq, seq_off, qual, qual_off) to write into: the byte columns at `residue`"""
        return (shifted(max(1, self.n) * 56, 0), shifted(self.seq.numel(), residue), shifted((self.n + 1) * 8, 0), shifted(self.qual.numel(), residue),
                shifted((self.n + 1) * 8, 0))


def columns_of(outs, n_recs, want_seq, want_qual):
    """the five output columns as the host tests' `same*` helpers take them, after the guards were looked at"""
    assert all(guards_intact(o) for o in outs)
    recs, seq, so, qual, qo = outs
    return (host(recs, _lib.FQREC_DTYPE)[:n_recs], host(seq)[:want_seq], host(so, np.uint64), host(qual)[:want_qual], host(qo, np.uint64))


@functools.lru_cache(maxsize=None)
def column_batch():
    from fastq_write_cases import Batch
    return Batch(dc.column_records())


@pytest.mark.parametrize("r_out", dc.COL_RES)
@pytest.mark.parametrize("r_in", dc.COL_RES)
def test_fastq_trim(r_in, r_out):
    import myers_oracle as mo
    from test_gpu_fastq_trim import expected, same_columns
    b = column_batch()
    hits = dc.trim_hits(b.records)
    parsed = types.SimpleNamespace(recs=b.recs, seq=np.frombuffer(b.seq, np.uint8), seq_off=b.seq_off, qual=np.frombuffer(b.qual, np.uint8),
                                   qual_off=b.qual_off)
    d, d_hits = Columns(b, r_in), typed(hits)
    for mode in (mo.TRIM_3P, mo.TRIM_5P):
        want = expected(mode, hits, 2, parsed)
        outs = d.outputs(r_out)
        totals = myers.trim_dev(mode, d_hits, 2, d.n, d.recs, d.seq, d.so, d.qual, d.qo, stream=stream(), out=outs)[5]
        assert totals == (len(want[1]), len(want[3]))
        same_columns(columns_of(outs, d.n, len(want[1]), len(want[3])), want)


@pytest.mark.parametrize("r_out", dc.COL_RES)
@pytest.mark.parametrize("r_in", dc.COL_RES)
def test_fastq_filter(r_in, r_out):
    import fastq_write_oracle as fw
    from test_gpu_fastq_filter import same
    b = column_batch()
    flt = dict(min_len=10, max_n=6)
    want = fw.filter_columns(*b.columns(), **flt)
    d = Columns(b, r_in)
    outs, d_keep = d.outputs(r_out), shifted(d.n, r_out)
    totals = fastq.filter_dev(d.n, d.recs, d.seq, d.so, d.qual, d.qo, stream=stream(), out=outs + (d_keep,), **flt)[6]
    assert totals == (len(want[0]), len(want[1]), len(want[3])) and guards_intact(d_keep)
    same(columns_of(outs, totals[0], len(want[1]), len(want[3])) + (host(d_keep),), want, d.n)


@pytest.mark.parametrize("r_out", dc.COL_RES)
@pytest.mark.parametrize("r_in", dc.COL_RES)
def test_fastq_demux_split(r_in, r_out):
    import fastq_demux_oracle as dm
    from test_gpu_fastq_demux import same_split
    b = column_batch()
    bins = dc.split_bins(len(b))
    want = dm.split(bins, 3, *b.columns())
    d, d_bin = Columns(b, r_in), typed(bins)
    outs, d_perm, d_boff = d.outputs(r_out), shifted(d.n * 8, 0), shifted(6 * 8, 0)
    boff = fastq.demux_split_dev(d.n, d_bin, 3, d.recs, d.seq, d.so, d.qual, d.qo, stream=stream(), out=outs + (None, d_perm, d_boff))[8]
    assert guards_intact(d_perm) and guards_intact(d_boff) and (host(d_boff, np.uint64) == boff).all()
    same_split(columns_of(outs, d.n, len(want[1]), len(want[3])) + (None, host(d_perm, np.uint64), boff), want, d.n)


@pytest.mark.parametrize("r_in", dc.COL_RES)
def test_fastq_qual_cut(r_in):
    import fastq_qual_oracle as qo
    from fastq_write_cases import Batch
    b = Batch(dc.qual_records())
    n = len(b)
    d_qual, d_qo = shifted_from(b.qual + b"#", r_in), i64(b.qual_off)
    for cp in CUT_PARAMS:
        want, want_tot, points = qo.cut(b.qual, b.qual_off, 33, **cp)
        d_cut = shifted(n * 64, 0)
        tot = fastq.qual_cut_dev(n, d_qual, d_qo, stream=stream(), want_totals=True, out=d_cut, phred_offset=33, **cp)[1]
        assert guards_intact(d_cut) and tot == want_tot
        got = host(d_cut).tobytes()
        bad = [r for r in range(n) if got[64 * r:64 * r + 64] != want[r].tobytes()]
        assert not bad, (r_in, cp, bad[:8], [points[r] for r in bad[:8]])
