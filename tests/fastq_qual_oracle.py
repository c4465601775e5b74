"""The three quality rules of include/biogpu.h (bg_fastq_qual_cut, bg_fastq_qual_select, bg_fastq_qc_tables) restated
serially on plain Python integers and numpy columns: what the tests compare the kernels, and the lane-parallel bodies of
csrc/fastq_qual_rule.h, against byte for byte."""
import numpy as np

from myers_oracle import ALN_DTYPE

MIN_SCORE = -858993459
NONE, RUNSUM, WINDOW = 0, 1, 2
PAIRED, PAIR_BOTH = 1, 2
STATS_DTYPE = np.dtype([("sum_q", "<u8"), ("weight_sum", "<u8"), ("len", "<u4"), ("n_low", "<u4"), ("min_q", "<u4"), ("_reserved", "<u4")])


def quals(raw, phred_offset=33):
    """q = max(0, c - phred_offset) per byte"""
    return [max(0, c - phred_offset) for c in bytes(raw)]


def reads(col, off):
    col = bytes(col)
    return [col[int(off[r]):int(off[r + 1])] for r in range(len(off) - 1)]


# ---- cut ---------------------------------------------------------------------------------------------------------------
def runsum_3p(q, cutoff):
    """(e, stopped early)"""
    s, best, e = 0, 0, len(q)
    for i in range(len(q) - 1, -1, -1):
        s += cutoff - q[i]
        if s < 0:
            return e, True
        if s > best:
            best, e = s, i
    return e, False


def runsum_5p(q, cutoff):
    """(b, stopped early)"""
    s, best, b = 0, 0, 0
    for i in range(len(q)):
        s += cutoff - q[i]
        if s < 0:
            return b, True
        if s > best:
            best, b = s, i + 1
    return b, False


def window_3p(q, cutoff, window):
    """(e, a failing window was found)"""
    L = len(q)
    W = min(window, L)
    for i in range(0, L - W + 1):
        if sum(q[i:i + W]) < cutoff * W:
            e = i
            while e > 0 and q[e - 1] < cutoff:
                e -= 1
            return e, True
    return L, False


def cut_points(q, method_5p=NONE, method_3p=RUNSUM, cutoff_5p=0, cutoff_3p=0, window=0, events=None):
    """(b, e) of one read's qualities; events (a dict of counters) learns which branches were taken"""
    L = len(q)
    b, e = 0, L
    stopped = found = False
    if method_5p == RUNSUM:
        b, stopped = runsum_5p(q, cutoff_5p)
    if method_3p == RUNSUM:
        e, st = runsum_3p(q, cutoff_3p)
        stopped = stopped or st
    elif method_3p == WINDOW:
        assert window >= 1
        e, found = window_3p(q, cutoff_3p, window)
    if e < b:
        e = b
    if events is not None:
        kind = "no-hit" if L == 0 or (b == 0 and e == L) else "nothing left" if e == b else "both" if b > 0 and e < L else "3p" if e < L else "5p"
        events[kind] = events.get(kind, 0) + 1
        events["stopped"] = events.get("stopped", 0) + stopped
        events["window"] = events.get("window", 0) + found
    return b, e


def cut_record(L, b, e):
    rec = np.zeros(1, dtype=ALN_DTYPE)
    rec["score"], rec["ylen"] = MIN_SCORE, L
    if L != 0 and not (b == 0 and e == L):
        rec["score"], rec["ystart"], rec["yend"] = L - (e - b), e, b
    return rec[0]


def cut(qual, qual_off, phred_offset=33, events=None, **params):
    """(records[n], (reads cut, symbols removed), [(b, e)])"""
    rows = reads(qual, qual_off)
    out = np.zeros(len(rows), dtype=ALN_DTYPE)
    points = []
    for r, raw in enumerate(rows):
        b, e = cut_points(quals(raw, phred_offset), events=events, **params)
        out[r] = cut_record(len(raw), b, e)
        points.append((b, e))
    removed = [len(raw) - (e - b) for raw, (b, e) in zip(rows, points)]
    return out, (sum(x > 0 for x in removed), sum(removed)), points


# ---- select ------------------------------------------------------------------------------------------------------------
def stats_of(raw, phred_offset=33, low_q=0, weight=None):
    q = quals(raw, phred_offset)
    return dict(sum_q=sum(q), weight_sum=sum(int(weight[c]) for c in bytes(raw)) if weight is not None else 0, len=len(q),
                n_low=sum(v < low_q for v in q), min_q=min(q) if q else 0)


def passes(s, min_mean_q=0, max_low_pct=100, max_weight=0, has_weight=False):
    ok = s["sum_q"] >= min_mean_q * s["len"]
    ok = ok and (max_low_pct >= 100 or s["n_low"] * 100 <= max_low_pct * s["len"])
    return ok and (not has_weight or s["weight_sum"] <= max_weight)


def select(qual, qual_off, flags=0, phred_offset=33, min_mean_q=0, low_q=0, max_low_pct=100, max_weight=0, weight=None, events=None):
    """(stats[n], bin uint32[n], records passed)"""
    rows = reads(qual, qual_off)
    stats = np.zeros(len(rows), dtype=STATS_DTYPE)
    own = []
    for r, raw in enumerate(rows):
        s = stats_of(raw, phred_offset, low_q, weight)
        for k, v in s.items():
            stats[r][k] = v
        own.append(passes(s, min_mean_q, max_low_pct, max_weight, weight is not None))
    keep = list(own)
    if flags & PAIRED:
        assert len(rows) % 2 == 0
        for p in range(0, len(rows), 2):
            keep[p] = keep[p + 1] = (own[p] or own[p + 1]) if flags & PAIR_BOTH else (own[p] and own[p + 1])
    if events is not None:
        events["pass"] = events.get("pass", 0) + sum(keep)
        events["fail"] = events.get("fail", 0) + len(keep) - sum(keep)
        events["overruled"] = events.get("overruled", 0) + sum(a != b for a, b in zip(own, keep))
    return stats, np.array([0 if k else 1 for k in keep], dtype=np.uint32), sum(keep)


def ee_weights(phred_offset=33, scale_bits=20):
    return np.array([int(round(10.0 ** (-max(0, c - phred_offset) / 10.0) * (1 << scale_bits))) for c in range(256)], dtype=np.uint32)


# ---- tables ------------------------------------------------------------------------------------------------------------
def tables_words(max_cycles):
    R = max_cycles + 1
    return 5 * R + 64 * R + (R + 1) + 64 + 1


def tables(seq, seq_off, qual, qual_off, max_cycles, first=0, step=1, phred_offset=33):
    """the one buffer (uint64[tables_words]) and its five parts as a dict of views"""
    R = max_cycles + 1
    buf = np.zeros(tables_words(max_cycles), dtype=np.uint64)
    t = dict(base=buf[:5 * R].reshape(R, 5), qhist=buf[5 * R:69 * R].reshape(R, 64), len_hist=buf[69 * R:70 * R + 1],
             meanq_hist=buf[70 * R + 1:70 * R + 65], n_reads=buf[70 * R + 65:])
    s_rows, q_rows = reads(seq, seq_off), reads(qual, qual_off)
    for r in range(first, len(s_rows), step):
        for i, c in enumerate(s_rows[r]):
            t["base"][min(i, max_cycles)]["ACGT".find(chr(c).upper()) if chr(c).upper() in "ACGT" else 4] += 1
        q = quals(q_rows[r], phred_offset)
        for i, v in enumerate(q):
            t["qhist"][min(i, max_cycles)][min(v, 63)] += 1
        t["len_hist"][min(len(s_rows[r]), max_cycles + 1)] += 1
        if q:
            t["meanq_hist"][min(63, sum(q) // len(q))] += 1
        t["n_reads"][0] += 1
    return buf, t


# ---- the composition with the trim ---------------------------------------------------------------------------------------
def trimmed(records, cut_records):
    """(id, desc, seq, qual) records after bg_fastq_trim at the 3' end and then at the 5' end with the same cut records (the
    trim rule of tests/myers_oracle.py, n_pat = 1).  Where a record's two lengths agree that is [b, e) of both."""
    import myers_oracle as mo
    out = []
    for (i, d, s, q), c in zip(records, cut_records):
        hit = [(int(c["score"]), int(c["ystart"]), int(c["yend"]))]
        for mode in (mo.TRIM_3P, mo.TRIM_5P):
            (lo, hi), (qlo, qhi) = mo.trim_range(mode, hit, len(s), len(q))
            s, q = s[lo:hi], q[qlo:qhi]
        out.append((i, d, s, q))
    return out
