"""The definition `bg_fastq_demux_assign[_dev]` and `bg_fastq_demux_split[_dev]` (csrc/fastq_demux.hip) are compared with,
in a few lines of Python.  The reference has no demultiplexer: include/biogpu.h defines both rules, `assign` follows its
items 1 to 7 literally, `split` is numpy's stable argsort."""
import numpy as np

from rust_bio_amd import _lib

MIN_SCORE = -858993459
ANCHOR_5P, ANCHOR_3P, PAIRED, MATE1, MATE2 = 1, 2, 4, 8, 16
IGNORE = 0xFFFFFFFF
INF = float("inf")


def no_hit(first):
    """rule 5's no-hit record of a read whose first record is `first`"""
    out = np.zeros(1, dtype=_lib.ALN_DTYPE)[0]
    out["score"], out["ylen"], out["mode"] = MIN_SCORE, first["ylen"], first["mode"]
    return out


def counts(h, b, flags, max_offset):
    """rule 1"""
    if int(h["score"]) == MIN_SCORE or b == IGNORE:
        return False
    if flags & ANCHOR_5P and int(h["ystart"]) > max_offset:
        return False
    if flags & ANCHOR_3P and (int(h["ylen"]) - int(h["yend"])) % 2**32 > max_offset:
        return False
    return True


def verdict(cands, n_bins, min_margin):
    """rules 2 to 4 over candidates (score, p, mate, bin): (bin, winner or None)"""
    if not cands:
        return n_bins, None
    win = min(cands, key=lambda c: c[:3])
    second = min([c[0] for c in cands if c[3] != win[3]], default=INF)
    if second - win[0] < min_margin:
        return n_bins + 1, win
    return win[3], win


def assign(hits, n_pat, pat_bin, n_bins, flags=0, min_margin=0, max_offset=0):
    """(bin uint32[n], hit_out records[n], pat_out uint32[n])"""
    n = len(hits) // n_pat
    bins, hit_out, pat_out = np.zeros(n, np.uint32), np.zeros(n, dtype=_lib.ALN_DTYPE), np.full(n, IGNORE, np.uint32)
    unit = 2 if flags & PAIRED else 1
    for r0 in range(0, n, unit):
        cands = []
        for mate in range(unit):
            if unit == 2 and flags & (MATE1 | MATE2) and not flags & (MATE1, MATE2)[mate]:
                continue  # rule 7: this mate's hits do not count
            r = r0 + mate
            cands += [(int(hits[r * n_pat + p]["score"]), p, mate, int(pat_bin[p])) for p in range(n_pat)
                      if counts(hits[r * n_pat + p], int(pat_bin[p]), flags, max_offset)]
        b, win = verdict(cands, n_bins, min_margin)
        for mate in range(unit):
            r = r0 + mate
            bins[r] = b
            if b < n_bins and win[2] == mate:
                hit_out[r], pat_out[r] = hits[r * n_pat + win[1]], win[1]
            else:
                hit_out[r] = no_hit(hits[r * n_pat])
    return bins, hit_out, pat_out


def split(bins, n_bins, recs, seq, so, qual, qo, hit=None):
    """(recs, seq, seq_off, qual, qual_off, hit_out or None, perm uint64[n], bin_off uint64[n_bins + 3])"""
    seq, qual = bytes(seq), bytes(qual)
    n = len(recs)
    group = np.where(np.asarray(bins, dtype=np.uint64) > n_bins + 1, n_bins, np.asarray(bins, dtype=np.uint64)).astype(np.int64)
    perm = np.argsort(group, kind="stable")
    out = recs[perm].copy()
    s = [seq[int(so[r]):int(so[r + 1])] for r in perm]
    q = [qual[int(qo[r]):int(qo[r + 1])] for r in perm]
    o_so, o_qo = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    if n:
        o_so[1:], o_qo[1:] = np.cumsum([len(x) for x in s]), np.cumsum([len(x) for x in q])
    out["seq_off"], out["qual_off"] = o_so[:n], o_qo[:n]
    bin_off = np.zeros(n_bins + 3, np.uint64)
    bin_off[1:] = np.cumsum(np.bincount(group, minlength=n_bins + 2))
    return out, b"".join(s), o_so, b"".join(q), o_qo, hit[perm].copy() if hit is not None else None, perm.astype(np.uint64), bin_off
