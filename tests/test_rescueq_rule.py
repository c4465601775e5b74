"""The mapping quality of rescued read pairs (include/biogpu.h, "Mapping quality of rescued read pairs") as
tests/rescueq_oracle.py states it, on hand-made candidate lists and a stubbed aligner: one case per class of mate with the
expected record worked out by hand, the clamp, the edges of min_score and mapq_cap, and the pairs that are not rescued.  No GPU."""
import pairq_oracle as qo
import rescueq_oracle as rq
from pair_oracle import MIN_SCORE

N_TEXT = 10_000
INT32_MIN = -2**31


def cand(score, start, end):
    return {"score": score, "ref_start": start, "ref_end": end}


def rule(v, align, pen=17, A=2, rescue_min_score=0, min_score=INT32_MIN, cap=60, max_span=500):
    return rq.rescueq_rule(v, (150, 150), N_TEXT, 0, max_span, pen, A, rescue_min_score, min_score, cap, align)


def beside(scores):
    """an aligner that places the sought mate 250 .. 400 behind a forward anchor's start, with the score of the anchor's rank"""
    return lambda q: cand(scores[q["rank"]], q["lo"] + 250, q["lo"] + 400)


def classes(detail):
    return [d["class"] for d in detail]


def test_unique_anchor_and_unique_rescued_mate():
    v = [[cand(150, 1000, 1150)], [], [], []]
    recs, detail, rescued = rule(v, beside([120]))
    assert rescued == 2
    assert recs == [(MIN_SCORE, 1, 1, 60), (MIN_SCORE, 1, 1, 60)]
    assert classes(detail) == [rq.ANCHOR_UNIQUE, rq.RESCUED_UNIQUE]
    # the same with the mates swapped: mate 2 anchors, mate 1 is rescued
    recs, detail, rescued = rule([[], [], [cand(150, 1000, 1150)], []], beside([120]))
    assert rescued == 1 and recs == [(MIN_SCORE, 1, 1, 60)] * 2 and classes(detail) == [rq.RESCUED_UNIQUE, rq.ANCHOR_UNIQUE]


def test_an_anchor_inside_a_far_repeat_costs_pen_unpaired():
    """the anchor has an equal copy far away whose own rescue fails: the anchor's mate is ahead by pen_unpaired alone"""
    v = [[cand(150, 1000, 1150), cand(150, 5000, 5150)], [], [], []]
    recs, detail, rescued = rule(v, beside([120, -60]))
    assert rescued == 2
    # S1 = 150 + 120 = 270; (b): 150 + 120 - 17 = 253; 60 * 17 // 150 = 6
    assert (detail[0]["S1"], detail[0]["S2"], detail[0]["a"], detail[0]["b"]) == (270, 253, None, 253)
    assert recs == [(150, 2, 1, 6), (MIN_SCORE, 1, 1, 60)]
    assert classes(detail) == [rq.ANCHOR_SEEDED_ALT, rq.RESCUED_UNIQUE]
    # mapq_cap at its ends: 254 * 17 // 150 = 28
    assert rule(v, beside([120, -60]), cap=254)[0] == [(150, 2, 1, 28), (MIN_SCORE, 1, 1, 254)]
    assert rule(v, beside([120, -60]), cap=0)[0] == [(150, 2, 1, 0), (MIN_SCORE, 1, 1, 0)]
    # pen_unpaired above the anchor's score: the quotient is capped by c_i.score, so by mapq_cap
    assert rule(v, beside([120, -60]), pen=200)[0][0] == (150, 2, 1, 60)


def test_two_anchors_that_rescue_the_same_placement():
    """both anchors of mate 1 lie within max_span of the one placement of mate 2: the anchor's mate cannot be told apart, the
    rescued mate has no alternative because the two hits touch"""
    same = lambda q: cand(120, 1400, 1500)
    v = [[cand(150, 1000, 1150), cand(150, 1200, 1350)], [], [], []]
    recs, detail, rescued = rule(v, same)
    assert rescued == 2
    # (a): 150 + 120 = 270 = S1; (b): 253
    assert (detail[0]["S1"], detail[0]["a"], detail[0]["b"]) == (270, 270, 253)
    assert recs == [(150, 2, 1, 0), (MIN_SCORE, 1, 1, 60)]
    assert classes(detail) == [rq.ANCHOR_RESCUED_ALT, rq.RESCUED_UNIQUE]
    # the second anchor ten below: S2 = 140 + 120 = 260 through (a), 60 * 10 // 150 = 4
    v = [[cand(150, 1000, 1150), cand(140, 1200, 1350)], [], [], []]
    assert rule(v, same)[0] == [(140, 2, 1, 4), (MIN_SCORE, 1, 1, 60)]


def test_a_fragment_wholly_inside_a_two_copy_repeat():
    v = [[cand(150, 1000, 1150), cand(150, 5000, 5150)], [], [], []]
    recs, detail, rescued = rule(v, beside([120, 120]))
    assert rescued == 2
    # both rescues are accepted and sum to 270: each mate's other copy is an alternative through (a)
    assert [(d["S1"], d["S2"], d["a"]) for d in detail] == [(270, 270, 270), (270, 270, 270)] and detail[1]["b"] is None
    assert recs == [(150, 2, 1, 0), (120, 2, 1, 0)]
    assert classes(detail) == [rq.ANCHOR_RESCUED_ALT, rq.RESCUED_RESCUED_ALT]
    # the far copy's mate scores 30 less, (a) = 240: the anchor's mate does better unpaired, (b) = 253, 60 * 17 // 150 = 6; the
    # rescued mate has (a) alone, 60 * 30 // 120 = 15
    recs, detail, _ = rule(v, beside([120, 90]))
    assert recs == [(150, 2, 1, 6), (90, 2, 1, 15)] and (detail[0]["a"], detail[0]["b"], detail[1]["a"]) == (240, 253, 240)
    # ... at pen_unpaired 40 it is (a) for both: 60 * 30 // 150 = 12
    assert rule(v, beside([120, 90]), pen=40)[0] == [(150, 2, 1, 12), (90, 2, 1, 15)]
    # ... and below the rescue's min_score it is no accepted rescue: the anchor's mate falls back on (b), the rescued mate is unique
    assert rule(v, beside([120, 90]), rescue_min_score=91)[0] == [(150, 2, 1, 6), (MIN_SCORE, 1, 1, 60)]


def seeded_copy_case():
    """mate 2's true placement beside mate 1 has no seed (score 130); an exact copy of it far away is a seeded candidate, whose
    own rescue of mate 1 finds nothing"""
    v = [[cand(150, 1000, 1150)], [], [], [cand(150, 7000, 7150)]]
    align = lambda q: cand(130, 1250, 1400) if q["mate"] == 0 else cand(-50, q["lo"], q["lo"] + 150)
    return v, align


def test_a_rescued_mate_with_a_seeded_copy_elsewhere():
    v, align = seeded_copy_case()
    # "paired or not" accepts at pen 25: 150 + 130 + 25 >= 150 + 150; at pen 19 it does not, and the records are the pairs-mapq call's
    recs, detail, rescued = rule(v, align, pen=25)
    assert rescued == 2
    # S1 = 280; (b) of mate 2: 150 + 150 - 25 = 275; 60 * 5 // 130 = 2
    assert (detail[1]["S1"], detail[1]["S2"], detail[1]["a"], detail[1]["b"]) == (280, 275, None, 275)
    assert recs == [(MIN_SCORE, 1, 1, 60), (150, 2, 1, 2)]
    assert classes(detail) == [rq.ANCHOR_UNIQUE, rq.RESCUED_SEEDED_ALT]
    recs, detail, rescued = rule(v, align, pen=19)
    assert rescued == 0 and (recs, detail) == qo.pairq_rule(v[0], v[1], v[2], v[3], 0, 500, 19)
    assert recs == [(MIN_SCORE, 1, 1, 60), (MIN_SCORE, 1, 1, 60)]


def test_min_score_one_either_side_of_an_alternative():
    v, align = seeded_copy_case()
    assert rule(v, align, pen=25, min_score=150)[0][1] == (150, 2, 1, 2)
    recs, detail, _ = rule(v, align, pen=25, min_score=151)
    assert recs[1] == (MIN_SCORE, 1, 1, 60) and detail[1]["class"] == rq.RESCUED_UNIQUE
    # the member of an accepted rescue is held to the same bound: the far copy's mate (90) in a two-copy fragment
    v = [[cand(150, 1000, 1150), cand(150, 5000, 5150)], [], [], []]
    assert rule(v, beside([120, 90]), min_score=90)[0][1] == (90, 2, 1, 15)
    assert rule(v, beside([120, 90]), pen=40, min_score=91)[0] == [(150, 2, 1, 12), (MIN_SCORE, 1, 1, 60)]
    # ... and so is the anchor: with min_score 151 the far anchor is no alternative of mate 1, its rescue no kind (a)
    assert rule(v, beside([120, 90]), min_score=151)[0] == [(MIN_SCORE, 1, 1, 60), (MIN_SCORE, 1, 1, 60)]


def test_the_clamp():
    """mate 1 is exact on the far copy (rank 0, its rescue fails) and has substitutions on the copy beside mate 2 (rank 1, the
    chosen anchor); with pen_unpaired below the score gap the mate unpaired at the far copy beats the pair: S2 > S1"""
    v = [[cand(140, 1000, 1150), cand(150, 5000, 5150)], [], [], []]
    by_anchor = lambda q: cand(120, 1250, 1400) if q["lo"] == 1000 else cand(-40, q["lo"] + 250, q["lo"] + 400)
    recs, detail, rescued = rule(v, by_anchor, pen=2)
    assert rescued == 2
    # S1 = 140 + 120 = 260; (b): 150 + 120 - 2 = 268
    assert (detail[0]["S1"], detail[0]["S2"]) == (260, 268)
    assert recs == [(150, 2, 1, 0), (MIN_SCORE, 1, 1, 60)]
    assert classes(detail) == [rq.ANCHOR_CLAMPED, rq.RESCUED_UNIQUE]
    # at pen 10 the two are level (0, not clamped), at pen 17 the pair is ahead by 7: 60 * 7 // 140 = 3
    recs, detail, _ = rule(v, by_anchor, pen=10)
    assert recs[0] == (150, 2, 1, 0) and detail[0]["class"] == rq.ANCHOR_SEEDED_ALT
    assert rule(v, by_anchor, pen=17)[0][0] == (150, 2, 1, 3)
    # A = 1 tries the far copy alone: nothing is rescued
    assert rule(v, by_anchor, pen=2, A=1)[2] == 0


def test_a_placement_that_scores_nothing():
    v = [[cand(150, 1000, 1150), cand(150, 5000, 5150)], [], [], []]
    for score in (0, -5):
        recs, detail, rescued = rule(v, beside([score, -60]), rescue_min_score=-10)
        assert rescued == 2
        assert recs[1] == (MIN_SCORE, 1, 1, 0)  # c_i.score <= 0, even without an alternative
        assert recs[0] == (150, 2, 1, 6)        # the anchor's mate: (b) against the same partner
    # an anchor that scores 0 (its mate has nothing better): 0 as well
    recs, _, rescued = rule([[cand(0, 1000, 1150)], [], [], []], beside([120]))
    assert rescued == 2 and recs == [(MIN_SCORE, 1, 1, 0), (MIN_SCORE, 1, 1, 60)]


def test_64_bit_sums():
    big = 2**31 - 1
    v = [[cand(big, 1000, 1150), cand(big, 5000, 5150)], [], [], []]
    recs, detail, rescued = rule(v, beside([big, big - 1]), pen=5)
    assert rescued == 2 and detail[0]["S1"] == 2 * big and detail[0]["S2"] == 2 * big - 1
    assert recs == [(big, 2, 1, 60 * 1 // big), (big - 1, 2, 1, 0)]


def test_pairs_that_are_not_rescued_keep_the_pairs_mapq_records():
    calls = []
    never = lambda q: calls.append(q) or cand(-50, q["lo"], q["lo"] + 150)
    # a proper seeded combination: no rescue alignment is run
    v = [[cand(90, 1000, 1100), cand(90, 5000, 5100)], [], [], [cand(90, 1200, 1300)]]
    recs, detail, rescued = rule(v, never)
    assert rescued == 0 and not calls
    assert (recs, detail) == qo.pairq_rule(v[0], v[1], v[2], v[3], 0, 500, 17)
    assert recs == [(90, 2, 1, 60 * 17 // 90), (MIN_SCORE, 1, 1, 60)]
    # rescue alignments run and none accepted: the multi rule at K = 1, 60 * (90 - 80) // 90 = 6
    v = [[cand(90, 1000, 1100), cand(80, 5000, 5100)], [], [], []]
    recs, detail, rescued = rule(v, never, min_score=10, cap=60)
    assert rescued == 0 and len(calls) == 2
    assert (recs, detail) == qo.pairq_rule(v[0], v[1], v[2], v[3], 0, 500, 17, 10, 60)
    assert recs == [(80, 2, 1, 6), (MIN_SCORE, 0, 0, 0)]
    assert classes(detail) == [qo.SINGLE_RUNNER_UP, qo.NO_CANDIDATES]
    # no candidate at all
    assert rule([[], [], [], []], never)[0] == [(MIN_SCORE, 0, 0, 0)] * 2
