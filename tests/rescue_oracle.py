"""CPU statement of mate rescue (include/biogpu.h, "Mate rescue": bg_seed_extend_pairs_rescue_batch), for the tests.

Built on tests/pair_oracle.py (`candidates`, `pair_rule`, `strand_best`) and, for the rescue windows, the oracle's
`align_batch(..., "semiglobal", ...)`.  `plan` picks a pair's anchors and windows, `decide` applies acceptance, choice and "paired or
not" to the aligned windows, `rescue_rule` is both around any aligner (the rule tests pass a stub), `expected` runs a batch of
interleaved mates with all rescue windows of the batch aligned in one oracle call."""
import numpy as np

import pair_oracle as po

HIT_FORWARD, HIT_REVERSE, HIT_NONE = po.HIT_FORWARD, po.HIT_REVERSE, po.HIT_NONE
MAX_ANCHORS = 4


def ranked(fwd, rev):
    """a mate's candidates over both strands in the multi call's rank order: [(strand, index)], score descending, then candidate
    number (forward strand first, ascending proposed start)"""
    allc = [(HIT_FORWARD, i) for i in range(len(fwd))] + [(HIT_REVERSE, i) for i in range(len(rev))]
    score = [c["score"] for c in fwd] + [c["score"] for c in rev]
    return [allc[k] for k in sorted(range(len(allc)), key=lambda k: (-score[k], k))]


def plan(v, lens, n_text, max_span, A):
    """The rescue alignments of one pair whose pair rule found nothing proper.  v = [m1f, m1r, m2f, m2r] candidate lists, lens =
    the two mates' lengths.  A list of requests: mate (the anchoring mate, 0 / 1), rank, strand and index of the anchor, xv (which
    virtual read of the pair is x: 2 * other + (1 if its revcomp)), lo, hi (the window)."""
    out = []
    for m in (0, 1):
        f, r = v[2 * m], v[2 * m + 1]
        other = 1 - m
        for rank, (st, i) in enumerate(ranked(f, r)[:A]):
            c = (f if st == HIT_FORWARD else r)[i]
            if c["ref_end"] - c["ref_start"] > max_span:
                continue
            if st == HIT_FORWARD:
                lo, hi = c["ref_start"], min(n_text, c["ref_start"] + max_span)
            else:
                lo, hi = max(0, c["ref_end"] - max_span), c["ref_end"]
            if hi - lo < 1 or lens[other] == 0:
                continue
            out.append({"mate": m, "rank": rank, "strand": st, "index": i, "xv": 2 * other + (1 if st == HIT_FORWARD else 0),
                        "lo": lo, "hi": hi})
    return out


def own_score(fwd, rev):
    pk = po.strand_best(fwd, rev)
    return 0 if pk is None else (fwd if pk[0] == HIT_FORWARD else rev)[pk[1]]["score"]


def decide(v, reqs, res, min_span, max_span, pen, min_score):
    """Acceptance, choice and "paired or not" over a pair's requests and their alignments (res[k]: a candidate-like dict with
    score, ref_start, ref_end).  None, or (request, rescued hit, span)."""
    best = None
    for q, h in zip(reqs, res):
        c = v[2 * q["mate"] + q["strand"]][q["index"]]
        a, b = (c, h) if q["strand"] == HIT_FORWARD else (h, c)  # the forward one is a, the reverse one b
        span = max(a["ref_end"], b["ref_end"]) - a["ref_start"]
        if h["score"] < min_score or not (a["ref_start"] <= b["ref_start"] and min_span <= span <= max_span):
            continue
        orient_a = (q["strand"] == HIT_FORWARD) == (q["mate"] == 0)  # m1 forward
        key = (c["score"] + h["score"], int(orient_a), int(q["mate"] == 0), -q["rank"])
        if best is None or key > best[0]:
            best = (key, q, h, span)
    if best is None:
        return None
    if best[0][0] + pen < own_score(v[0], v[1]) + own_score(v[2], v[3]):
        return None
    return best[1:]


def rescue_rule(v, lens, n_text, min_span, max_span, pen, A, min_score, align):
    """The whole rule on one pair.  align(request) -> candidate-like dict.  Returns (pick1, pick2, proper, span, n_proper, rescued,
    n_alignments); pick = (strand, index) of a seeded candidate, (strand, hit dict) for the rescued mate, or None."""
    pk1, pk2, proper, span, n_proper = po.pair_rule(v[0], v[1], v[2], v[3], min_span, max_span, pen)
    if n_proper > 0 or not (v[0] or v[1] or v[2] or v[3]):
        return pk1, pk2, proper, span, n_proper, 0, 0
    reqs = plan(v, lens, n_text, max_span, A)
    res = [align(q) for q in reqs]
    got = decide(v, reqs, res, min_span, max_span, pen, min_score)
    if got is None:
        return pk1, pk2, False, 0, 0, 0, len(reqs)
    q, h, span = got
    anchor = (q["strand"], q["index"])
    resc = (HIT_REVERSE if q["strand"] == HIT_FORWARD else HIT_FORWARD, h)
    picks = (anchor, resc) if q["mate"] == 0 else (resc, anchor)
    return picks[0], picks[1], True, span, 0, 2 - q["mate"], len(reqs)


def expected(orc, sc, cands, n_hits, vreads, voff, text, n_text, n_pairs, min_span, max_span, pen, A, min_score):
    """cands / n_hits of the 4 n_pairs virtual reads (pair_oracle.candidates on pair_oracle.virtual_reads) -> (per read: (strand,
    candidate dict or None, n_candidates, n_seed_hits), per pair: (proper, span, n_proper), rescued uint8[n_pairs], alignments run).
    A rescued mate's dict has the fields of a candidate's (rec, ops, wlo, score, ref_start, ref_end)."""
    plans = {}
    xs, ys, who = [], [], []
    for p in range(n_pairs):
        v = [cands[4 * p + k] for k in range(4)]
        n_proper = po.pair_rule(v[0], v[1], v[2], v[3], min_span, max_span, pen)[4]
        if n_proper > 0 or not any(v):
            continue
        lens = [int(voff[4 * p + 2 * m + 1] - voff[4 * p + 2 * m]) for m in (0, 1)]
        plans[p] = plan(v, lens, n_text, max_span, A)
        for k, q in enumerate(plans[p]):
            a, e = int(voff[4 * p + q["xv"]]), int(voff[4 * p + q["xv"] + 1])
            xs.append(vreads[a:e])
            ys.append(text[q["lo"]:q["hi"]])
            who.append((p, k))
    results = {}
    if who:
        x, y = np.concatenate(xs), np.concatenate(ys)
        xo = np.zeros(len(xs) + 1, np.uint64)
        yo = np.zeros(len(ys) + 1, np.uint64)
        xo[1:] = np.cumsum([len(s) for s in xs])
        yo[1:] = np.cumsum([len(s) for s in ys])
        recs, ops, ostride = orc.align_batch(sc, "semiglobal", x, xo, y, yo, threads=8)
        for c, (p, k) in enumerate(who):
            rec = recs[c]
            lo = plans[p][k]["lo"]
            n = int(rec["n_ops"])
            results[(p, k)] = {"wlo": lo, "rec": rec, "score": int(rec["score"]), "ref_start": lo + int(rec["ystart"]),
                               "ref_end": lo + int(rec["yend"]),
                               "ops": (ops[c * ostride:c * ostride + n] & np.uint64(0xFF)).astype(np.uint8)}
    reads, pairs = [], []
    rescued = np.zeros(n_pairs, np.uint8)
    for p in range(n_pairs):
        v = [cands[4 * p + k] for k in range(4)]
        lens = [int(voff[4 * p + 2 * m + 1] - voff[4 * p + 2 * m]) for m in (0, 1)]
        reqs = plans.get(p, [])
        by_key = {(q["mate"], q["rank"]): results[(p, k)] for k, q in enumerate(reqs)}
        pk1, pk2, proper, span, n_proper, resc, n_al = rescue_rule(v, lens, n_text, min_span, max_span, pen, A, min_score,
                                                                   lambda q: by_key[(q["mate"], q["rank"])])
        assert n_al == len(reqs), p
        rescued[p] = resc
        for m, pk in ((0, pk1), (1, pk2)):
            f, r = v[2 * m], v[2 * m + 1]
            if pk is None:
                c = None
            elif isinstance(pk[1], dict):
                c = pk[1]
            else:
                c = (f if pk[0] == HIT_FORWARD else r)[pk[1]]
            reads.append((HIT_NONE if pk is None else pk[0], c, len(f) + len(r), int(n_hits[4 * p + 2 * m] + n_hits[4 * p + 2 * m + 1])))
        pairs.append((proper, span, n_proper))
    return reads, pairs, rescued, len(who)
