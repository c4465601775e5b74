"""`bio::io::fasta` reading side (io/fasta.rs:334-359, 982-1009, 1090-1111) on a FASTA text held in memory, and the
reference text built from its records.  The records are parsed on the device (csrc/fasta_ingest.hip: tile summaries, one
scan, one apply pass) and the sequences land concatenated with 64-bit offsets; `reference_*` turns them into the index
text `S0 $ S1 $ ... $` (or `T $ R $` for an FMD index) with the `sam.Contigs` that `sam.header` / `sam.emit_*` take."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FASTA_REF_FMD as REF_FMD, FASTA_REF_UPPER as REF_UPPER  # noqa: F401
from .sam import Contigs

STATUS = ["ok", "MissingGt", "Io"]
CHECK = ["ok", "EmptyId", "NonAsciiSequence", "InvalidSequence"]
B = _lib.FASTA_TILE  # bytes of the text per block of the device kernels (BG_FASTA_TILE): what tests place their edges around


class ReadError(Exception):
    """the io::Error of fasta::Reader::read (fasta.rs:337-351)"""

    def __init__(self, kind, pos):
        super().__init__(f"{kind} at byte {pos}")
        self.kind, self.pos = kind, pos


class CheckError(Exception):
    """fasta::CheckError (fasta.rs:993-1009)"""

    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


class Record:
    """fasta::Record (fasta.rs:940-1040)"""

    def __init__(self, id_=b"", desc=None, seq=b"", check_code=0):
        self._id, self._desc, self._seq, self._check = id_, desc, seq, check_code

    def id(self):
        return self._id.decode()

    def desc(self):
        return None if self._desc is None else self._desc.decode()

    def seq(self):
        return self._seq

    def is_empty(self):  # fasta.rs:982-984
        return not self._id and self._desc is None and not self._seq

    def check(self):  # fasta.rs:993-1009, evaluated on the device with the parse
        if self._check:
            raise CheckError(CHECK[self._check])

    def __eq__(self, o):
        return (self._id, self._desc, self._seq) == (o._id, o._desc, o._seq)

    def __repr__(self):
        return f"Record(id={self._id!r}, desc={self._desc!r}, seq={self._seq!r})"


class Parsed:
    """columns of one parse: recs (bg_fasta_record_t), seq (concatenated), seq_off (n + 1)"""

    def __init__(self, text, recs, seq, seq_off, status, err_pos):
        self.text, self.recs, self.seq, self.seq_off = text, recs, seq, seq_off
        self.status, self.err_pos = STATUS[status], err_pos

    def __len__(self):
        return len(self.recs)

    def record(self, k):
        r, t = self.recs[k], self.text
        return Record(t[int(r["id_off"]):int(r["id_off"]) + int(r["id_len"])].tobytes(),
                      t[int(r["desc_off"]):int(r["desc_off"]) + int(r["desc_len"])].tobytes() if r["has_desc"] else None,
                      self.seq[int(self.seq_off[k]):int(self.seq_off[k + 1])].tobytes(), int(r["check"]))


def default_rec_cap(ln):
    """records a text of `ln` bytes can hold at most: a record that is not empty takes three bytes, the last one two"""
    return ln // 3 + 2


def parse_arrays(text, ctx=None, rec_cap=None):
    """All records up to the end of the text, the first empty record or the first read error (Parsed.status / err_pos)."""
    ctx = ctx or _lib.default_context()
    t = _lib.as_u8(text)
    cap = default_rec_cap(len(t)) if rec_cap is None else rec_cap
    recs = np.zeros(cap, dtype=_lib.FAREC_DTYPE)
    seq = np.zeros(max(1, len(t)), dtype=np.uint8)
    so = np.zeros(cap + 1, dtype=np.uint64)
    n, st, ep = C.c_uint64(0), C.c_int32(0), C.c_uint64(0)
    rc = _lib.lib().bg_fasta_parse(ctx.h, t.ctypes.data, len(t), recs.ctypes.data, cap, seq.ctypes.data, so.ctypes.data, C.byref(n),
                                   C.byref(st), C.byref(ep))
    if rc == -8:
        raise TooManyRecords(int(n.value))
    _lib.check(rc, "bg_fasta_parse")
    k = int(n.value)
    return Parsed(t, recs[:k], seq[:int(so[k])], so[:k + 1], st.value, int(ep.value))


class TooManyRecords(_lib.BiogpuError):
    """BG_ERR_TOO_LARGE of the parse: `n_records` says how many records rec_cap has to hold"""

    def __init__(self, n_records):
        super().__init__(-8, "bg_fasta_parse")
        self.n_records = n_records


def alloc_dev(ln, device, rec_cap=None):
    """output buffers of parse_dev for a text of `ln` bytes: records, sequences, their offsets"""
    import torch
    cap = default_rec_cap(ln) if rec_cap is None else rec_cap
    return (torch.empty(cap * 48, dtype=torch.uint8, device=device), torch.empty(max(1, ln), dtype=torch.uint8, device=device),
            torch.empty(cap + 1, dtype=torch.int64, device=device))


def parse_dev(d_text, ctx=None, stream=0, bufs=None, rec_cap=None):
    """d_text: uint8 torch tensor on the device.  Returns (n_records, status name, err_pos, d_recs, d_seq, d_seq_off) with
    everything but the first three left in HBM.  `bufs`: the three tensors of `alloc_dev(len, device, rec_cap)` to reuse
    across calls; `rec_cap`: records they hold (default: the most a text of this length can have)."""
    ctx = ctx or _lib.default_context()
    ln = int(d_text.numel())
    cap = default_rec_cap(ln) if rec_cap is None else rec_cap
    d_recs, d_seq, d_so = bufs if bufs is not None else alloc_dev(ln, d_text.device, cap)
    n, st, ep = C.c_uint64(0), C.c_int32(0), C.c_uint64(0)
    rc = _lib.lib().bg_fasta_parse_dev(ctx.h, d_text.data_ptr(), ln, d_recs.data_ptr(), cap, d_seq.data_ptr(), d_so.data_ptr(), C.byref(n),
                                       C.byref(st), C.byref(ep), stream)
    if rc == -8:
        raise TooManyRecords(int(n.value))
    _lib.check(rc, "bg_fasta_parse_dev")
    k = int(n.value)
    return k, STATUS[st.value], int(ep.value), d_recs[:k * 48], d_seq, d_so[:k + 1]


class BadRecord(_lib.BiogpuError, ValueError):
    """the reference builder met a record whose check() is not Ok: `index` is the first one"""

    def __init__(self, index):
        super().__init__(-1, "bg_fasta_reference")
        self.index = index


def reference_arrays(parsed, flags=0):
    """bg_fasta_reference on a Parsed: (text: uint8 array, sam.Contigs).  flags: REF_FMD | REF_UPPER."""
    n = len(parsed)
    recs = np.ascontiguousarray(parsed.recs)
    bufs = [np.ascontiguousarray(x) if len(x) else np.zeros(1, np.uint8) for x in (parsed.text, parsed.seq)]
    nt, nb, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call(out, cap, contigs, names, ncap):
        rc = _lib.lib().bg_fasta_reference(None, n, recs.ctypes.data, bufs[0].ctypes.data, bufs[1].ctypes.data, flags, out, cap, contigs,
                                           names, ncap, C.byref(nt), C.byref(nb), C.byref(bad))
        if rc == -1 and bad.value != 2**64 - 1:
            raise BadRecord(int(bad.value))
        _lib.check(rc, "bg_fasta_reference")

    call(None, 0, None, None, 0)
    text = np.zeros(max(1, nt.value), dtype=np.uint8)
    table = np.zeros(n, dtype=_lib.SAM_CONTIG_DTYPE)
    names = np.zeros(max(1, nb.value), dtype=np.uint8)
    call(text.ctypes.data, nt.value, table.ctypes.data, names.ctypes.data, nb.value)
    return text[:nt.value], Contigs.from_arrays(table, names[:nb.value])


def reference_dev(n_records, d_recs, d_fasta_text, d_seq, flags=0, ctx=None, stream=0):
    """bg_fasta_reference_dev on what parse_dev left in HBM: a sizing call, then the build into fresh tensors.  Returns
    (d_text, d_contigs, d_names, sam.Contigs): the index text, the contig table (bytes) and names on the device, and the
    same table on the host for `sam.header`."""
    import torch
    ctx = ctx or _lib.default_context()
    nt, nb, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call(out, cap, contigs, names, ncap):
        rc = _lib.lib().bg_fasta_reference_dev(ctx.h, n_records, d_recs.data_ptr(), d_fasta_text.data_ptr(), d_seq.data_ptr(), flags, out,
                                               cap, contigs, names, ncap, C.byref(nt), C.byref(nb), C.byref(bad), stream)
        if rc == -1 and bad.value != 2**64 - 1:
            raise BadRecord(int(bad.value))
        _lib.check(rc, "bg_fasta_reference_dev")

    call(None, 0, None, None, 0)
    dev = d_fasta_text.device
    d_text = torch.empty(max(1, nt.value), dtype=torch.uint8, device=dev)
    d_contigs = torch.empty(n_records * 32, dtype=torch.uint8, device=dev)
    d_names = torch.empty(max(1, nb.value), dtype=torch.uint8, device=dev)
    call(d_text.data_ptr(), nt.value, d_contigs.data_ptr(), d_names.data_ptr(), nb.value)
    table = d_contigs.cpu().numpy().view(_lib.SAM_CONTIG_DTYPE)  # (the copy also waits for the write pass)
    return d_text[:nt.value], d_contigs, d_names, Contigs.from_arrays(table, d_names[:nb.value].cpu().numpy())


class Reader:
    """fasta::Reader over an in-memory text (`Reader::new(&[u8])`, fasta.rs:228-240)."""

    def __init__(self, text, ctx=None):
        self._parsed = parse_arrays(text, ctx)

    def records(self):
        """`Reader::records()` (fasta.rs:1090-1111): yields Records; raises ReadError where the iterator yields Err."""
        p = self._parsed
        for k in range(len(p)):
            yield p.record(k)
        if p.status != "ok":
            raise ReadError(p.status, p.err_pos)
