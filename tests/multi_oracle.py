"""CPU statement of the multi-locus rule of seed-and-extend (include/biogpu.h, bg_seed_extend_multi_batch), for the tests.

The candidate lists come from `pair_oracle.candidates` on `pair_oracle.virtual_reads` (the oracle's own backward_search_batch,
suffix array and align_batch semiglobal); `multi_rule` applies the rule to one read's forward and reverse lists, `expected`
to a batch."""
from pair_oracle import HIT_FORWARD, HIT_NONE, HIT_REVERSE, MIN_SCORE, candidates, virtual_reads  # noqa: F401

INT32_MIN = -2**31


def ranked(fwd, rev):
    """one read's candidates as (strand, index, candidate), in rank order: score descending, then candidate number (forward strand
    first, list order within a strand)"""
    numbered = [(HIT_FORWARD, i, c) for i, c in enumerate(fwd)] + [(HIT_REVERSE, i, c) for i, c in enumerate(rev)]
    order = sorted(range(len(numbered)), key=lambda n: (-numbered[n][2]["score"], n))
    return [numbered[n] for n in order]


def touches(a, b):
    return a["ref_start"] <= b["ref_end"] and b["ref_start"] <= a["ref_end"]


def mapq_of(s1, s2, mapq_cap):
    """s1: score of locus 0 or None; s2: score of locus 1 or None.  Python integers: no overflow to model."""
    if s1 is None:
        return 0
    s2 = 0 if s2 is None else s2
    if s1 <= 0 or s2 >= s1:
        return 0
    return min(mapq_cap, mapq_cap * (s1 - max(s2, 0)) // s1)


def multi_rule(fwd, rev, K, min_score=INT32_MIN, mapq_cap=60):
    """The rule on one read's candidate lists (dicts with score, ref_start, ref_end).
    Returns (picks: [(strand, index)] of the reported loci, sub_score, n_loci, mapq)."""
    kept = []
    for st, i, c in ranked(fwd, rev):
        if len(kept) == max(K, 2):
            break
        if c["score"] < min_score or any(touches(c, k[2]) for k in kept):
            continue
        kept.append((st, i, c))
    s1 = kept[0][2]["score"] if kept else None
    s2 = kept[1][2]["score"] if len(kept) > 1 else None
    return [(st, i) for st, i, _ in kept[:K]], (MIN_SCORE if s2 is None else s2), len(kept), mapq_of(s1, s2, mapq_cap)


def top_k(fwd, rev, K, min_score=INT32_MIN):
    """the plain top K by rank, without suppression (what the rule must differ from where loci overlap)"""
    return [(st, i) for st, i, c in ranked(fwd, rev) if c["score"] >= min_score][:K]


def expected(cands, n_hits, n_reads, strands, K, min_score=INT32_MIN, mapq_cap=60):
    """cands / n_hits of the virtual reads (2 per read with strands = 3: read, revcomp; otherwise 1 per read, on the strand that
    ran) -> per read: (slots: K of (strand, candidate dict or None), n_candidates, n_seed_hits, sub_score, n_loci, mapq)"""
    out = []
    for r in range(n_reads):
        if strands == 3:
            f, v, nh = cands[2 * r], cands[2 * r + 1], int(n_hits[2 * r] + n_hits[2 * r + 1])
        elif strands == 2:
            f, v, nh = [], cands[r], int(n_hits[r])
        else:
            f, v, nh = cands[r], [], int(n_hits[r])
        picks, sub, n_loci, mapq = multi_rule(f, v, K, min_score, mapq_cap)
        slots = [(st, (f if st == HIT_FORWARD else v)[i]) for st, i in picks] + [(HIT_NONE, None)] * (K - len(picks))
        out.append((slots, len(f) + len(v), nh, sub, n_loci, mapq))
    return out

