"""CPU statement of SMEM-seeded seed-and-extend (include/biogpu.h, bg_seed_extend_smem_batch), for the tests.

Built from the oracle's own calls, like pair_oracle.candidates (restated here, not shared): `oracle_py.FMDIndex.all_smems` on the
caller's read, the oracle suffix array of T$R$ for the rows [lower, lower + size) of every voting record, `propose` for the two
coordinate formulas, and `align_batch(..., "semiglobal")` on every candidate window.  `candidates` returns every candidate per
(read, strand), the rows per half, and which reads were truncated or panicked; `expected` applies the strands rule."""
import numpy as np

from rust_bio_amd.alphabets import dna

MIN_SCORE = -858993459
HIT_FORWARD, HIT_REVERSE, HIT_NONE = 0, 1, 255
STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH = 1, 2, 3
SA_NONE = 0xFFFFFFFFFFFFFFFF


def half(n_t, length, p):
    """the half of T$R$ (n_t: length of T) a match of `length` symbols at text position p lies in: HIT_FORWARD, HIT_REVERSE, or
    None (across a sentinel, or no position at all)"""
    if p < 0 or p >= 2 * n_t + 2:
        return None
    if p + length <= n_t:
        return HIT_FORWARD
    if p >= n_t + 1 and p + length <= 2 * n_t + 1:
        return HIT_REVERSE
    return None


def propose(n_t, L, a, length, p):
    """The proposal of text position p for the record at read position a with `length` symbols, L the read's length:
    (HIT_FORWARD, start of the read on T), (HIT_REVERSE, start of revcomp(read) on T), or None where the rule drops it."""
    h = half(n_t, length, p)
    if h == HIT_FORWARD:
        if p < a:
            return None
        s = p - a
    elif h == HIT_REVERSE:
        q = p - n_t - 1
        if q + L > n_t + a:
            return None
        s = n_t + a - q - L
    else:
        return None
    return None if s >= n_t else (h, s)


def merged(starts, pad):
    """the strands call's merge: sorted, equal starts once, then a start within pad // 2 of the last one kept is dropped"""
    kept = []
    for s in sorted(set(starts)):
        if not kept or s - kept[-1] > pad // 2:
            kept.append(s)
    return kept


def records(ofmd, read, min_seed_len):
    """all_smems(read, min_seed_len) as [(lower, size, a, len)] in push order; None where the reference panics"""
    try:
        recs = ofmd.all_smems(bytes(read), min_seed_len)
    except IndexError:
        return None
    return [(iv[0], iv[2], a, ln) for iv, a, ln in recs]


def candidates(orc, ofmd, sa, fwd, sc, reads, off, strands=STRAND_BOTH, min_seed_len=19, max_smems=16, max_occ=16, pad=25):
    """ofmd: oracle_py.FMDIndex over T$R$, sa: its suffix array, fwd: T (uint8 array).  Returns a dict:
       cands      per read {HIT_FORWARD: [...], HIT_REVERSE: [...]}, candidate dicts as pair_oracle.candidates makes them
       n_hits     per read, the rows of its voting records in the half of a strand that ran
       rows       every row the voting records resolved (totals[0])
       truncated  per read: it has more than max_smems records
       panicked   per read: the reference panics on it"""
    fwd = np.ascontiguousarray(fwd, np.uint8)
    n_t = len(fwd)
    assert len(sa) == 2 * n_t + 2
    R = len(off) - 1
    ran = [h for h, bit in ((HIT_FORWARD, STRAND_FORWARD), (HIT_REVERSE, STRAND_REVERSE)) if strands & bit]
    starts = [{HIT_FORWARD: [], HIT_REVERSE: []} for _ in range(R)]
    n_hits = np.zeros(R, np.int64)
    truncated, panicked = np.zeros(R, bool), np.zeros(R, bool)
    rows = 0
    for r in range(R):
        a0, L = int(off[r]), int(off[r + 1] - off[r])
        recs = records(ofmd, reads[a0:a0 + L], min_seed_len)
        if recs is None:
            panicked[r] = True
            continue
        truncated[r] = len(recs) > max_smems
        for lower, size, a, ln in recs[:max_smems]:
            if not 1 <= size <= max_occ:
                continue
            for row in range(lower, lower + size):
                rows += 1
                p = int(sa[row]) if row < len(sa) else SA_NONE
                h = half(n_t, ln, p)
                if h in ran:
                    n_hits[r] += 1
                    pr = propose(n_t, L, a, ln, p)
                    if pr is not None:
                        starts[r][h].append(pr[1])
    xs, ys, who = [], [], []
    for r in range(R):
        a0, L = int(off[r]), int(off[r + 1] - off[r])
        read = reads[a0:a0 + L]
        for h in ran:
            x = read if h == HIT_FORWARD else dna.revcomp(read)
            for s in merged(starts[r][h], pad):
                lo_w, hi_w = max(0, s - pad), min(n_t, s + L + pad)
                xs.append(x)
                ys.append(fwd[lo_w:hi_w])
                who.append((r, h, s, lo_w))
    cands = [{HIT_FORWARD: [], HIT_REVERSE: []} for _ in range(R)]
    if who:
        x, y = np.concatenate(xs), np.concatenate(ys)
        xo, yo = np.zeros(len(xs) + 1, np.uint64), np.zeros(len(ys) + 1, np.uint64)
        xo[1:] = np.cumsum([len(v) for v in xs])
        yo[1:] = np.cumsum([len(v) for v in ys])
        recs, ops, ostride = orc.align_batch(sc, "semiglobal", x, xo, y, yo, threads=8)
        for c, (r, h, s, lo_w) in enumerate(who):
            rec = recs[c]
            k = int(rec["n_ops"])
            cands[r][h].append({"start": s, "wlo": lo_w, "rec": rec, "score": int(rec["score"]),
                                "ref_start": lo_w + int(rec["ystart"]), "ref_end": lo_w + int(rec["yend"]),
                                "ops": (ops[c * ostride:c * ostride + k] & np.uint64(0xFF)).astype(np.uint8)})
    return {"cands": cands, "n_hits": n_hits, "rows": rows, "truncated": truncated, "panicked": panicked}


def strand_best(fwd, rev):
    """the strands rule over one read's forward and reverse candidate lists (each sorted by start): (strand, index) or None —
    the highest score, the forward strand on a tie, the smallest start within a strand"""
    best = None
    for st, lst in ((HIT_FORWARD, fwd), (HIT_REVERSE, rev)):
        for i, c in enumerate(lst):
            if best is None or c["score"] > best[2]:
                best = (st, i, c["score"])
    return None if best is None else best[:2]


def expected(res):
    """per read (strand, candidate dict or None, n_candidates, n_seed_hits) of a `candidates` result"""
    out = []
    for r, c in enumerate(res["cands"]):
        pk = strand_best(c[HIT_FORWARD], c[HIT_REVERSE])
        out.append((HIT_NONE if pk is None else pk[0], None if pk is None else c[pk[0]][pk[1]],
                    len(c[HIT_FORWARD]) + len(c[HIT_REVERSE]), int(res["n_hits"][r])))
    return out


def compare(hits, strand, ops, want, what=""):
    """every hit field, the strand and the winner's operations of a call (hits[r].aln.ops_off into ops) against `expected`"""
    assert len(hits) == len(want) == len(strand)
    for r, (st, c, nc, nsh) in enumerate(want):
        h = hits[r]
        assert int(strand[r]) == st, (what, r, "strand", int(strand[r]), st)
        assert int(h["n_candidates"]) == nc and int(h["n_seed_hits"]) == nsh, (what, r, "counts", int(h["n_candidates"]), nc, int(h["n_seed_hits"]), nsh)
        if c is None:
            assert int(h["aln"]["score"]) == MIN_SCORE and int(h["aln"]["n_ops"]) == 0, (what, r)
            assert int(h["ref_start"]) == SA_NONE and int(h["ref_end"]) == SA_NONE and int(h["window_start"]) == SA_NONE, (what, r)
            continue
        assert int(h["window_start"]) == c["wlo"] and int(h["ref_start"]) == c["ref_start"] and int(h["ref_end"]) == c["ref_end"], (what, r)
        for f in ("score", "xstart", "xend", "ystart", "yend", "xlen", "ylen", "n_ops"):
            assert int(h["aln"][f]) == int(c["rec"][f]), (what, r, f)
        assert int(h["aln"]["mode"]) == 2, (what, r)
        if ops is not None:
            o, k = int(h["aln"]["ops_off"]), int(h["aln"]["n_ops"])
            assert (ops[o:o + k] == c["ops"]).all(), (what, r, "ops")


def to_arrays(want, hit_dtype):
    """`expected` as the arrays a call returns: (hits of hit_dtype, strand, the winners' operations back to back)"""
    hits = np.zeros(len(want), dtype=hit_dtype)
    strand = np.zeros(len(want), np.uint8)
    ops = []
    for r, (st, c, nc, nsh) in enumerate(want):
        strand[r] = st
        hits[r]["n_candidates"], hits[r]["n_seed_hits"] = nc, nsh
        a = hits[r]["aln"]
        if c is None:
            a["score"] = MIN_SCORE
            hits[r]["window_start"] = hits[r]["ref_start"] = hits[r]["ref_end"] = SA_NONE
            a["ops_off"] = sum(len(o) for o in ops)
            continue
        for f in ("score", "xstart", "xend", "ystart", "yend", "xlen", "ylen", "n_ops"):
            a[f] = int(c["rec"][f])
        a["mode"], a["ops_off"] = 2, sum(len(o) for o in ops)
        hits[r]["window_start"], hits[r]["ref_start"], hits[r]["ref_end"] = c["wlo"], c["ref_start"], c["ref_end"]
        ops.append(c["ops"])
    return hits, strand, np.concatenate(ops) if ops else np.zeros(0, np.uint8)
