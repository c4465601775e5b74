"""CPU statement of the mapping quality of read pairs (include/biogpu.h, bg_seed_extend_pairs_mapq_batch), for the tests.

Composed from `pair_oracle.pair_rule` (which combination is chosen, proper or not), `multi_oracle.multi_rule` (a mate of a pair
that is not proper is a single read at K = 1), `multi_oracle.touches` / `mapq_of`, and the definition of the header, in Python
integers.  `pairq_rule` applies the rule to the four candidate lists of one pair, `expected` to a batch."""
from multi_oracle import INT32_MIN, mapq_of, multi_rule, touches
from pair_oracle import HIT_FORWARD, MIN_SCORE, pair_rule

# the classes a mate can fall into (the GPU test counts them before it compares anything)
PROPER_ALT_PAIRED, PROPER_ALT_UNPAIRED, PROPER_UNIQUE, SINGLE_RUNNER_UP, SINGLE_UNIQUE, NO_CANDIDATES = range(6)
CLASS_NAMES = ("proper, alternative in a proper combination", "proper, unpaired alternatives only", "proper, no alternative",
               "not proper, runner-up", "not proper, no runner-up", "no candidates")


def proper_combinations(v, min_span, max_span):
    """every proper combination of one pair's lists v = [m1 fwd, m1 rev, m2 fwd, m2 rev] as (mate 1's candidate, mate 2's)"""
    out = []
    for fa, fb, a_is_m1 in ((v[0], v[3], True), (v[2], v[1], False)):
        for a in fa:
            for b in fb:
                span = max(a["ref_end"], b["ref_end"]) - a["ref_start"]
                if a["ref_start"] <= b["ref_start"] and min_span <= span <= max_span:
                    out.append((a, b) if a_is_m1 else (b, a))
    return out


def pairq_rule(m1f, m1r, m2f, m2r, min_span, max_span, pen, min_score=INT32_MIN, mapq_cap=60):
    """Returns (records, detail): records = per mate (sub_score, n_loci, n_reported, mapq); detail = per mate a dict with the
    mate's class and, for a proper pair, S1, S2 (None without an alternative) and the two kinds' maxima."""
    v = [m1f, m1r, m2f, m2r]
    pk1, pk2, proper, _, _ = pair_rule(m1f, m1r, m2f, m2r, min_span, max_span, pen)
    recs, detail = [], []
    if not proper:
        for m in range(2):
            picks, sub, n_loci, mapq = multi_rule(v[2 * m], v[2 * m + 1], 1, min_score, mapq_cap)
            recs.append((sub, n_loci, len(picks), mapq))
            cls = NO_CANDIDATES if not v[2 * m] and not v[2 * m + 1] else SINGLE_RUNNER_UP if n_loci > 1 else SINGLE_UNIQUE
            detail.append({"class": cls})
        return recs, detail
    chosen = [(v[2 * m] if pk[0] == HIT_FORWARD else v[2 * m + 1])[pk[1]] for m, pk in enumerate((pk1, pk2))]
    S1 = chosen[0]["score"] + chosen[1]["score"]
    combos = proper_combinations(v, min_span, max_span)
    for i in range(2):
        j = 1 - i
        ci, cj = chosen[i], chosen[j]
        alts = [x for x in v[2 * i] + v[2 * i + 1] if x["score"] >= min_score and not touches(x, ci)]
        kind_a = [c[0]["score"] + c[1]["score"] for c in combos if c[i]["score"] >= min_score and not touches(c[i], ci)]
        kind_b = [x["score"] + cj["score"] - pen for x in alts]
        sub = max((x["score"] for x in alts), default=MIN_SCORE)
        S2 = max(kind_a + kind_b, default=None)
        if ci["score"] <= 0:
            mapq = 0
        elif not alts:
            mapq = mapq_cap
        else:
            mapq = min(mapq_cap, mapq_cap * min(S1 - S2, ci["score"]) // ci["score"])
        recs.append((sub, 2 if alts else 1, 1, mapq))
        detail.append({"class": PROPER_UNIQUE if not alts else PROPER_ALT_PAIRED if kind_a else PROPER_ALT_UNPAIRED, "S1": S1, "S2": S2,
                       "a": max(kind_a, default=None), "b": max(kind_b, default=None)})
    return recs, detail


def expected(cands, n_hits, n_pairs, min_span, max_span, pen, min_score=INT32_MIN, mapq_cap=60):
    """cands / n_hits of the 4 n_pairs virtual reads -> (per read: (sub_score, n_loci, n_reported, mapq), per read: its class)"""
    recs, classes = [], []
    for p in range(n_pairs):
        r, d = pairq_rule(*[cands[4 * p + k] for k in range(4)], min_span, max_span, pen, min_score, mapq_cap)
        recs += r
        classes += [x["class"] for x in d]
    return recs, classes


__all__ = ["pairq_rule", "expected", "proper_combinations", "mapq_of"]
