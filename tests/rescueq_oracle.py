"""CPU statement of the mapping quality of rescued read pairs (include/biogpu.h, bg_seed_extend_pairs_rescue_mapq_batch), for
the tests, in Python integers.

Composed from `rescue_oracle` (`plan`, the acceptance of `decide`, `rescue_rule`), `pairq_oracle.pairq_rule` (a pair that is not
rescued) and `multi_oracle.touches`.  `rescueq_rule` applies the rule to the four candidate lists of one pair around any aligner
(the rule tests pass a stub), `expected` to a batch with all rescue windows aligned in one oracle call."""
import numpy as np

import pairq_oracle as qo
import rescue_oracle as ro
from multi_oracle import INT32_MIN, touches
from pair_oracle import MIN_SCORE

# the classes a mate of a RESCUED pair can fall into (a mate of any other pair keeps its class of pairq_oracle, 0 .. 5)
(ANCHOR_UNIQUE, ANCHOR_SEEDED_ALT, ANCHOR_RESCUED_ALT, ANCHOR_CLAMPED, RESCUED_UNIQUE, RESCUED_SEEDED_ALT,
 RESCUED_RESCUED_ALT) = range(6, 13)
RESCUED_CLASSES = tuple(range(6, 13))
CLASS_NAMES = qo.CLASS_NAMES + ("anchor, no alternative", "anchor, seeded alternatives only", "anchor, alternative with its own accepted rescue",
                                "anchor, S2 > S1 (clamped)", "rescued, no alternative", "rescued, seeded alternative",
                                "rescued, alternative through another accepted rescue")
NEVER = 1 << 62  # a pen_unpaired under which "paired or not" turns nothing down


def accepted(v, q, h, min_span, max_span, min_score):
    """the rescue rule's acceptance of one planned rescue q with its alignment h: decide's, without "paired or not\""""
    return ro.decide(v, [q], [h], min_span, max_span, NEVER, min_score) is not None


def members(v, q, h):
    """(mate 1's member, mate 2's member) of a rescue: its anchor for the anchoring mate, its hit for the other"""
    anchor = v[2 * q["mate"] + q["strand"]][q["index"]]
    return (anchor, h) if q["mate"] == 0 else (h, anchor)


def rescueq_rule(v, lens, n_text, min_span, max_span, pen, A, rescue_min_score, min_score, mapq_cap, align):
    """The whole rule on one pair.  v = [m1f, m1r, m2f, m2r] candidate lists, align(request) -> candidate-like dict.  Returns
    (records, detail, rescued): records = per mate (sub_score, n_loci, n_reported, mapq); detail = per mate a dict with the mate's
    class and, in a rescued pair, S1, S2 and the two kinds' maxima; rescued = the rescue rule's byte."""
    reqs, res = [], []
    n_proper = ro.po.pair_rule(v[0], v[1], v[2], v[3], min_span, max_span, pen)[4]
    if n_proper == 0 and any(v):
        reqs = ro.plan(v, lens, n_text, max_span, A)
        res = [align(q) for q in reqs]
    by_key = {(q["mate"], q["rank"]): h for q, h in zip(reqs, res)}
    pk1, pk2, _, _, _, rescued, _ = ro.rescue_rule(v, lens, n_text, min_span, max_span, pen, A, rescue_min_score,
                                                   lambda q: by_key[(q["mate"], q["rank"])])
    if not rescued:
        recs, detail = qo.pairq_rule(v[0], v[1], v[2], v[3], min_span, max_span, pen, min_score, mapq_cap)
        return recs, detail, 0
    r = rescued - 1  # the rescued mate; the other one anchors
    chosen = [pk[1] if isinstance(pk[1], dict) else v[2 * m + pk[0]][pk[1]] for m, pk in enumerate((pk1, pk2))]
    S1 = chosen[0]["score"] + chosen[1]["score"]
    acc = [members(v, q, h) for q, h in zip(reqs, res) if accepted(v, q, h, min_span, max_span, rescue_min_score)]
    recs, detail = [], []
    for i in range(2):
        j = 1 - i
        ci, cj = chosen[i], chosen[j]
        seeded = [x for x in v[2 * i] + v[2 * i + 1] if x["score"] >= min_score and not touches(x, ci)]
        through = [mem for mem in acc if mem[i]["score"] >= min_score and not touches(mem[i], ci)]
        alts = seeded + [mem[i] for mem in through]
        kind_a = [mem[0]["score"] + mem[1]["score"] for mem in through]
        kind_b = [x["score"] + cj["score"] - pen for x in seeded]
        sub = max((x["score"] for x in alts), default=MIN_SCORE)
        S2 = max(kind_a + kind_b, default=None)
        if ci["score"] <= 0:
            mapq = 0
        elif not alts:
            mapq = mapq_cap
        else:
            mapq = min(mapq_cap, mapq_cap * min(max(S1 - S2, 0), ci["score"]) // ci["score"])
        recs.append((sub, 2 if alts else 1, 1, mapq))
        if i == r:
            cls = RESCUED_UNIQUE if not alts else RESCUED_RESCUED_ALT if kind_a else RESCUED_SEEDED_ALT
        else:
            cls = (ANCHOR_UNIQUE if not alts else ANCHOR_CLAMPED if S2 > S1 else ANCHOR_RESCUED_ALT if kind_a else ANCHOR_SEEDED_ALT)
        detail.append({"class": cls, "S1": S1, "S2": S2, "a": max(kind_a, default=None), "b": max(kind_b, default=None)})
    return recs, detail, rescued


def expected(orc, sc, cands, voff, vreads, text, n_text, n_pairs, min_span, max_span, pen, A, rescue_min_score, min_score=INT32_MIN,
             mapq_cap=60, aligned=None):
    """cands of the 4 n_pairs virtual reads (pair_oracle.candidates on pair_oracle.virtual_reads) -> (per read: (sub_score, n_loci,
    n_reported, mapq), per read: its class, rescued uint8[n_pairs], aligned).  `aligned` caches the rescue alignments by (pair,
    anchoring mate, rank): they depend on max_span and A alone, so one set serves every (min_score, mapq_cap)."""
    if aligned is None:
        aligned = {}
        xs, ys, who = [], [], []
        for p in range(n_pairs):
            v = [cands[4 * p + k] for k in range(4)]
            if ro.po.pair_rule(v[0], v[1], v[2], v[3], min_span, max_span, pen)[4] > 0 or not any(v):
                continue
            lens = [int(voff[4 * p + 2 * m + 1] - voff[4 * p + 2 * m]) for m in (0, 1)]
            for q in ro.plan(v, lens, n_text, max_span, A):
                a, e = int(voff[4 * p + q["xv"]]), int(voff[4 * p + q["xv"] + 1])
                xs.append(vreads[a:e])
                ys.append(text[q["lo"]:q["hi"]])
                who.append((p, q["mate"], q["rank"], q["lo"]))
        if who:
            x, y = np.concatenate(xs), np.concatenate(ys)
            xo = np.zeros(len(xs) + 1, np.uint64)
            yo = np.zeros(len(ys) + 1, np.uint64)
            xo[1:] = np.cumsum([len(s) for s in xs])
            yo[1:] = np.cumsum([len(s) for s in ys])
            recs, _, _ = orc.align_batch(sc, "semiglobal", x, xo, y, yo, threads=8)
            for c, (p, m, rank, lo) in enumerate(who):
                aligned[(p, m, rank)] = {"score": int(recs[c]["score"]), "ref_start": lo + int(recs[c]["ystart"]),
                                         "ref_end": lo + int(recs[c]["yend"])}
    out, classes = [], []
    rescued = np.zeros(n_pairs, np.uint8)
    for p in range(n_pairs):
        v = [cands[4 * p + k] for k in range(4)]
        lens = [int(voff[4 * p + 2 * m + 1] - voff[4 * p + 2 * m]) for m in (0, 1)]
        recs, detail, rescued[p] = rescueq_rule(v, lens, n_text, min_span, max_span, pen, A, rescue_min_score, min_score, mapq_cap,
                                                lambda q: aligned[(p, q["mate"], q["rank"])])
        out += recs
        classes += [d["class"] for d in detail]
    return out, classes, rescued, aligned


__all__ = ["rescueq_rule", "expected", "accepted", "members"]
