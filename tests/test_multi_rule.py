"""The multi-locus rule of include/biogpu.h (bg_seed_extend_multi_batch) as tests/multi_oracle.py states it, pinned on hand-built
candidate lists: locus suppression, rank and ties, min_score and the integer MAPQ formula."""
import multi_oracle as mo
from multi_oracle import HIT_FORWARD as F, HIT_REVERSE as R, MIN_SCORE


def c(score, a, e):
    return {"score": score, "ref_start": a, "ref_end": e}


def test_touching_intervals_are_one_locus_and_a_base_apart_two():
    # [100, 250] and [250, 400] share position 250: one locus
    assert mo.multi_rule([c(100, 100, 250), c(90, 250, 400)], [], 4) == ([(F, 0)], MIN_SCORE, 1, 60)
    # [100, 250] and [251, 400]: two
    assert mo.multi_rule([c(100, 100, 250), c(90, 251, 400)], [], 4) == ([(F, 0), (F, 1)], 90, 2, 6)
    # containment and the mirrored order
    assert mo.multi_rule([c(90, 0, 1000), c(100, 400, 500)], [], 4)[0] == [(F, 1)]
    assert mo.multi_rule([c(90, 251, 400), c(100, 100, 250)], [], 4)[0] == [(F, 1), (F, 0)]


def test_suppression_is_by_kept_loci_only():
    # A = [0, 100] suppresses B = [100, 200]; B would have suppressed C = [200, 300], but B was not kept: C is locus 1
    A, B, C = c(100, 0, 100), c(99, 100, 200), c(98, 200, 300)
    picks, sub, n_loci, mapq = mo.multi_rule([A, B, C], [], 4)
    assert picks == [(F, 0), (F, 2)] and sub == 98 and n_loci == 2 and mapq == 60 * 2 // 100
    assert mo.top_k([A, B, C], [], 2) == [(F, 0), (F, 1)]  # the plain top 2 differs


def test_equal_scores_go_to_the_lower_candidate_number_forward_first():
    fwd, rev = [c(80, 1000, 1150), c(80, 5000, 5150)], [c(80, 300, 450), c(81, 9000, 9150)]
    picks, sub, n_loci, mapq = mo.multi_rule(fwd, rev, 4)
    assert picks == [(R, 1), (F, 0), (F, 1), (R, 0)] and sub == 80 and n_loci == 4 and mapq == 60 * 1 // 81
    # equal best scores: MAPQ 0, the forward one reported first
    assert mo.multi_rule([c(80, 1000, 1150)], [c(80, 300, 450)], 2) == ([(F, 0), (R, 0)], 80, 2, 0)


def test_the_same_interval_on_opposite_strands_is_one_locus():
    assert mo.multi_rule([c(70, 2000, 2150)], [c(70, 2000, 2150)], 4) == ([(F, 0)], MIN_SCORE, 1, 60)
    assert mo.multi_rule([c(70, 2000, 2150)], [c(75, 2100, 2250)], 4) == ([(R, 0)], MIN_SCORE, 1, 60)


def test_min_score_removes_a_runner_up():
    fwd = [c(100, 0, 150), c(40, 1000, 1150)]
    assert mo.multi_rule(fwd, [], 2, min_score=40) == ([(F, 0), (F, 1)], 40, 2, 36)
    assert mo.multi_rule(fwd, [], 2, min_score=41) == ([(F, 0)], MIN_SCORE, 1, 60)
    # below min_score, a candidate suppresses nothing either
    fwd = [c(100, 0, 150), c(90, 100, 250), c(80, 200, 350)]
    assert mo.multi_rule(fwd, [], 2, min_score=95)[0] == [(F, 0)]
    assert mo.multi_rule([c(90, 100, 250), c(80, 100, 250)], [], 2, min_score=95) == ([], MIN_SCORE, 0, 0)


def test_mapq_edges():
    assert mo.mapq_of(None, None, 60) == 0            # no locus
    assert mo.mapq_of(100, 100, 60) == 0              # s2 >= s1
    assert mo.mapq_of(0, None, 60) == 0               # s1 <= 0
    assert mo.mapq_of(-5, -9, 60) == 0
    assert mo.mapq_of(100, -30, 60) == 60             # a negative s2 counts as 0
    assert mo.mapq_of(100, None, 60) == 60
    assert mo.mapq_of(150, 149, 60) == 0              # 60 / 150 truncates
    assert mo.mapq_of(150, 75, 60) == 30
    assert mo.mapq_of(150, 1, 60) == 59               # 60 * 149 // 150
    assert mo.mapq_of(150, 1, 254) == 252             # 254 * 149 // 150
    assert mo.mapq_of(150, 0, 254) == 254
    assert mo.mapq_of(150, 75, 0) == 0
    # near 2^31: 254 * (s1 - s2) needs more than 32 bits
    s1 = 2**31 - 1
    assert mo.mapq_of(s1, 1, 254) == 253 and mo.mapq_of(s1, s1 - 1, 254) == 0 and mo.mapq_of(s1, 2**30, 254) == 126
    assert (254 * (s1 - 1)) >> 32 > 0
    assert mo.mapq_of(s1, -2**31, 60) == 60


def test_k_1_still_reports_the_runner_up():
    fwd = [c(100, 0, 150), c(90, 1000, 1150), c(80, 2000, 2150)]
    assert mo.multi_rule(fwd, [], 1) == ([(F, 0)], 90, 2, 6)


def test_the_walk_stops_at_max_k_2():
    fwd = [c(100 - k, 1000 * k, 1000 * k + 150) for k in range(12)]
    for K in (1, 2, 4, 8):
        picks, sub, n_loci, mapq = mo.multi_rule(fwd, [], K)
        assert len(picks) == K and n_loci == max(K, 2) and sub == 99
    exp = mo.expected([fwd, []], [7, 2], 1, 3, 4)
    slots, nc, nh, sub, n_loci, mapq = exp[0]
    assert [s[0] for s in slots] == [F] * 4 and nc == 12 and nh == 9 and n_loci == 4
    slots = mo.expected([fwd[:2]], [7], 1, 2, 4)[0][0]
    assert [s[0] for s in slots] == [R, R, mo.HIT_NONE, mo.HIT_NONE] and slots[2][1] is None
