"""The definition `bg_fastq_emit[_dev]` and `bg_fastq_filter[_dev]` (csrc/fastq_emit.hip) are compared with, in a few
lines of Python: `fastq::Writer::write` (io/fastq.rs:573-593, which is also `Display for Record`, 473-485) and the filter
rule, which the reference does not have and include/biogpu.h defines."""
import numpy as np

MIN_SCORE = -858993459
PAIRED, PAIR_BOTH, DISCARD_UNTRIMMED, DISCARD_TRIMMED, CHECK_OK = 1, 2, 4, 8, 16
NO_BOUND = 0xFFFFFFFF


def write(id_, desc, seq, qual):
    """Writer::write: the bytes of one record; desc None is Option::None"""
    out = b"@" + bytes(id_)                      # fastq.rs:580-581
    if desc is not None:
        out += b" " + bytes(desc)                # 582-585
    return out + b"\n" + bytes(seq) + b"\n+\n" + bytes(qual) + b"\n"  # 586-590


def record_fields(text, recs, seq, qual, r):
    """(id, desc, seq, qual) of record r by its own fields, as the emit call takes them"""
    text, seq, qual = bytes(text), bytes(seq), bytes(qual)
    c = recs[r]
    io, il, do, dl = int(c["id_off"]), int(c["id_len"]), int(c["desc_off"]), int(c["desc_len"])
    so, sl, qo, ql = int(c["seq_off"]), int(c["seq_len"]), int(c["qual_off"]), int(c["qual_len"])
    return text[io:io + il], text[do:do + dl] if c["has_desc"] else None, seq[so:so + sl], qual[qo:qo + ql]


def emit(text, recs, seq, qual, first=0, step=1):
    """(text, offsets[m + 1]) of records first, first + step, ..."""
    lines = [write(*record_fields(text, recs, seq, qual, r)) for r in range(first, len(recs), step)]
    off = np.zeros(len(lines) + 1, dtype=np.uint64)
    if lines:
        off[1:] = np.cumsum([len(ln) for ln in lines])
    return b"".join(lines), off


def passes(seq, check, trimmed, flags=0, min_len=0, max_len=NO_BOUND, max_n=NO_BOUND):
    ok = min_len <= len(seq) <= max_len
    if flags & CHECK_OK:
        ok = ok and check == 0
    if flags & DISCARD_UNTRIMMED:
        ok = ok and trimmed
    if flags & DISCARD_TRIMMED:
        ok = ok and not trimmed
    if max_n != NO_BOUND:
        ok = ok and sum(b in b"Nn" for b in bytes(seq)) <= max_n
    return ok


def keep_flags(passed, flags):
    """the pair rule over the pass flags of all records"""
    if not flags & PAIRED:
        return list(passed)
    out = []
    for p in range(0, len(passed), 2):
        a, b = passed[p], passed[p + 1]
        out += [(a or b) if flags & PAIR_BOTH else (a and b)] * 2
    return out


def filter_columns(recs, seq, seq_off, qual, qual_off, flags=0, min_len=0, max_len=NO_BOUND, max_n=NO_BOUND, hits=None, n_pat=0):
    """(recs, seq, seq_off, qual, qual_off, keep) as the filter call must return them"""
    seq, qual = bytes(seq), bytes(qual)
    n = len(recs)
    s = [seq[int(seq_off[r]):int(seq_off[r + 1])] for r in range(n)]
    q = [qual[int(qual_off[r]):int(qual_off[r + 1])] for r in range(n)]
    trimmed = [hits is not None and any(int(h["score"]) != MIN_SCORE for h in hits[r * n_pat:(r + 1) * n_pat]) for r in range(n)]
    keep = keep_flags([passes(s[r], int(recs[r]["check"]), trimmed[r], flags, min_len, max_len, max_n) for r in range(n)], flags)
    kept = [r for r in range(n) if keep[r]]
    out = recs[kept].copy()
    so, qo = [0], [0]
    for k, r in enumerate(kept):
        out[k]["seq_off"], out[k]["qual_off"] = so[-1], qo[-1]
        so.append(so[-1] + len(s[r]))
        qo.append(qo[-1] + len(q[r]))
    return (out, b"".join(s[r] for r in kept), np.array(so, np.uint64), b"".join(q[r] for r in kept), np.array(qo, np.uint64),
            np.array(keep, dtype=np.uint8))
