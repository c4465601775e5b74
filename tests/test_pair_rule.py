"""The CPU statement of the read-pair rule (tests/pair_oracle.py, include/biogpu.h) on hand-built candidate lists: the
GPU tests hold the device to it, so it is pinned here on its own."""
import pair_oracle as po

F, R = po.HIT_FORWARD, po.HIT_REVERSE


def c(start, score, length=100):
    return {"ref_start": start, "ref_end": start + length, "score": score}


def test_orientation_a_and_b():
    # A: m1 forward with m2 reverse
    assert po.pair_rule([c(1000, 100)], [], [], [c(1300, 100)], 0, 1000, 0) == ((F, 0), (R, 0), True, 400, 1)
    # B: m2 forward with m1 reverse
    assert po.pair_rule([], [c(1300, 100)], [c(1000, 100)], [], 0, 1000, 0) == ((R, 0), (F, 0), True, 400, 1)


def test_rf_ff_rr_are_never_proper():
    # the reverse mate starts before the forward one (RF)
    assert po.pair_rule([c(1300, 100)], [], [], [c(1000, 100)], 0, 1000, 0)[2:] == (False, 0, 0)
    # both forward, both reverse
    assert po.pair_rule([c(1000, 100)], [], [c(1300, 100)], [], 0, 1000, 0)[2:] == (False, 0, 0)
    assert po.pair_rule([], [c(1000, 100)], [], [c(1300, 100)], 0, 1000, 0)[2:] == (False, 0, 0)


def test_equal_starts_and_overlapping_mates():
    # a.ref_start == b.ref_start is proper; the span is the longer mate's end
    assert po.pair_rule([c(1000, 90, 80)], [], [], [c(1000, 90, 120)], 0, 1000, 0) == ((F, 0), (R, 0), True, 120, 1)
    # a reverse mate inside the forward one: span = a's length
    assert po.pair_rule([c(1000, 90, 150)], [], [], [c(1020, 90, 50)], 150, 150, 0)[2:] == (True, 150, 1)


def test_span_limits_are_inclusive():
    m1, m2 = [c(1000, 100)], [c(1300, 100)]
    assert po.pair_rule(m1, [], [], m2, 400, 400, 0)[2] is True
    assert po.pair_rule(m1, [], [], m2, 401, 900, 0)[2] is False
    assert po.pair_rule(m1, [], [], m2, 0, 399, 0)[2] is False


def test_ties():
    # orientation A wins a tie with B
    got = po.pair_rule([c(1000, 100)], [c(5300, 100)], [c(5000, 100)], [c(1300, 100)], 0, 1000, 0)
    assert got == ((F, 0), (R, 0), True, 400, 2)
    # then the smaller index of the forward mate, then of the reverse mate
    got = po.pair_rule([c(1000, 100), c(2000, 100)], [], [], [c(2100, 100), c(2200, 100)], 0, 2000, 0)
    assert got[:2] == ((F, 0), (R, 0)) and got[4] == 4
    got = po.pair_rule([c(1000, 90), c(2000, 100)], [], [], [c(2100, 100), c(2200, 100)], 0, 2000, 0)
    assert got[:2] == ((F, 1), (R, 0))
    got = po.pair_rule([c(1000, 100)], [], [], [c(2100, 90), c(2200, 100)], 0, 2000, 0)
    assert got[:2] == ((F, 0), (R, 1))


def test_pen_unpaired_and_fallback():
    # m2's own best is far away (improper) and scores 6 more than its proper candidate
    m1f, m2r = [c(1000, 100)], [c(1300, 94), c(90_000, 100)]
    assert po.pair_rule(m1f, [], [], m2r, 0, 1000, 6)[:3] == ((F, 0), (R, 0), True)
    assert po.pair_rule(m1f, [], [], m2r, 0, 1000, 5) == ((F, 0), (R, 1), False, 0, 1)
    # no candidate for one mate: its own (none), and never proper
    assert po.pair_rule([c(1000, 100)], [], [], [], 0, 1000, 100) == ((F, 0), None, False, 0, 0)
    # the strands rule: forward strand on an equal score, then the smallest index
    assert po.strand_best([c(5, 10), c(9, 10)], [c(1, 10)]) == (F, 0)
    assert po.strand_best([c(5, 9)], [c(1, 10), c(2, 10)]) == (R, 0)
