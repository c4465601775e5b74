"""The mate rescue rule (include/biogpu.h, "Mate rescue") as tests/rescue_oracle.py states it, on hand-made candidate lists and a
stubbed aligner: anchors, windows, acceptance, choice and "paired or not" at their edges.  No GPU."""
import rescue_oracle as ro

F, R = ro.HIT_FORWARD, ro.HIT_REVERSE
N_TEXT = 10_000


def cand(score, start, end):
    return {"score": score, "ref_start": start, "ref_end": end}


def fixed(score, start=None, end=None):
    """an aligner that places x at [start, end) (default: the last / first 100 bytes of the window, towards the far end from the anchor)"""
    def align(q):
        if start is not None:
            return cand(score, start, end)
        return cand(score, q["hi"] - 100, q["hi"]) if q["strand"] == F else cand(score, q["lo"], q["lo"] + 100)
    return align


def rule(v, align, lens=(100, 100), n_text=N_TEXT, min_span=0, max_span=500, pen=0, A=2, min_score=0):
    return ro.rescue_rule(v, lens, n_text, min_span, max_span, pen, A, min_score, align)


def test_a_proper_seeded_pair_or_no_candidate_is_left_alone():
    calls = []
    align = lambda q: calls.append(q) or cand(100, 0, 100)
    v = [[cand(90, 1000, 1100)], [], [], [cand(90, 1200, 1300)]]
    assert rule(v, align) == ((F, 0), (R, 0), True, 300, 1, 0, 0)
    # a proper combination that "paired or not" turns down is still not rescued
    v = [[cand(90, 1000, 1100)], [cand(200, 5000, 5100)], [], [cand(90, 1200, 1300)]]
    assert rule(v, align) == ((R, 0), (R, 0), False, 0, 1, 0, 0)
    assert rule([[], [], [], []], align) == (None, None, False, 0, 0, 0, 0)
    assert not calls


def test_anchor_order_and_the_cut_off():
    # rank: score descending, then forward strand first, ascending start
    f = [cand(50, 100, 200), cand(80, 3000, 3100), cand(80, 4000, 4100)]
    r = [cand(80, 2000, 2100), cand(90, 6000, 6100)]
    assert ro.ranked(f, r) == [(R, 1), (F, 1), (F, 2), (R, 0), (F, 0)]
    v = [f, r, [], []]
    for A in (1, 2, 4):
        reqs = ro.plan(v, (100, 100), N_TEXT, 500, A)
        assert [(q["strand"], q["index"], q["rank"], q["mate"]) for q in reqs] == [(R, 1, 0, 0), (F, 1, 1, 0), (F, 2, 2, 0), (R, 0, 3, 0)][:A]
    # the other mate is sought on the opposite strand: its revcomp (virtual read 3) for a forward anchor, itself (2) for a reverse one
    assert [q["xv"] for q in ro.plan(v, (100, 100), N_TEXT, 500, 4)] == [2, 3, 3, 2]
    assert [q["xv"] for q in ro.plan([[], [], f, r], (100, 100), N_TEXT, 500, 2)] == [0, 1]
    assert [q["mate"] for q in ro.plan([f, [], [], r], (100, 100), N_TEXT, 500, 1)] == [0, 1]  # both mates anchor


def test_windows_at_the_ends_of_the_text():
    w = lambda c_f, c_r, span=500: [(q["lo"], q["hi"]) for q in ro.plan([c_f, c_r, [], []], (100, 100), N_TEXT, span, 4)]
    assert w([cand(9, 1000, 1100)], []) == [(1000, 1500)]
    assert w([cand(9, 9700, 9800)], []) == [(9700, N_TEXT)]            # min(n_text, ...)
    assert w([cand(9, 9500, 9600)], []) == [(9500, N_TEXT)]            # exactly at the end
    assert w([], [cand(9, 1000, 1100)]) == [(600, 1100)]
    assert w([], [cand(9, 300, 400)]) == [(0, 400)]                    # saturating
    assert w([], [cand(9, 400, 500)]) == [(0, 500)]
    assert w([], [cand(9, 0, 0)]) == []                                # an empty window gives no alignment
    # an anchor longer than max_span is skipped and keeps its rank
    reqs = ro.plan([[cand(9, 1000, 1501), cand(8, 2000, 2500)], [], [], []], (100, 100), N_TEXT, 500, 2)
    assert [(q["index"], q["rank"]) for q in reqs] == [(1, 1)]
    assert ro.plan([[cand(9, 1000, 1100)], [], [], []], (100, 0), N_TEXT, 500, 2) == []  # an x of length 0


def test_span_edges_and_order():
    v = [[cand(90, 1000, 1100)], [], [], []]
    hit = fixed(80, 1300, 1400)  # span 400
    for lo, hi, ok in ((400, 400, True), (401, 500, False), (0, 399, False), (0, 400, True)):
        got = rule(v, hit, min_span=lo, max_span=hi)
        assert got[2] == ok and got[5] == (2 if ok else 0) and got[3] == (400 if ok else 0), (lo, hi)
    assert rule(v, hit)[:2] == ((F, 0), (R, cand(80, 1300, 1400)))
    # a reverse anchor: the rescued forward mate must not start behind it (a.ref_start <= b.ref_start)
    v = [[], [cand(90, 1300, 1400)], [], []]
    assert rule(v, fixed(80, 1300, 1350))[2:6] == (True, 100, 0, 2)
    assert rule(v, fixed(80, 1301, 1350))[2:6] == (False, 0, 0, 0)
    assert rule(v, fixed(80, 1000, 1100))[:4] == ((R, 0), (F, cand(80, 1000, 1100)), True, 400)
    # ... and the span reaches the farther end
    assert rule([[cand(90, 1000, 1500)], [], [], []], fixed(80, 1100, 1200))[3] == 500


def test_min_score_at_its_edge():
    v = [[], [], [cand(90, 1000, 1100)], []]
    assert rule(v, fixed(40), min_score=40)[5] == 1
    assert rule(v, fixed(40), min_score=41)[5] == 0
    assert rule(v, fixed(-7), min_score=-7, pen=7)[5] == 1


def test_pen_unpaired_at_its_edge():
    # own = 0 for the mate without candidates: sum + pen >= own(m1) + 0
    v = [[cand(90, 1000, 1100)], [], [], []]
    assert rule(v, fixed(-30), min_score=-100, pen=30)[5] == 2
    assert rule(v, fixed(-30), min_score=-100, pen=29)[5] == 0
    # both mates have candidates at unrelated loci: the rescue gives up own(m2) - rescued score
    v = [[cand(90, 1000, 1100)], [], [cand(70, 8000, 8100)], []]
    best = lambda q: cand(60, q["hi"] - 100, q["hi"]) if q["mate"] == 0 else cand(10, q["hi"] - 100, q["hi"])
    assert rule(v, best, pen=10)[2:6] == (True, 500, 0, 2)
    got = rule(v, best, pen=9)
    assert got == ((F, 0), (F, 0), False, 0, 0, 0, 2)  # the paired call's output: each mate's own best


def test_choice_and_its_tie_breaks():
    # the highest sum wins
    v = [[cand(90, 1000, 1100), cand(80, 3000, 3100)], [], [], []]
    by_rank = lambda scores: (lambda q: cand(scores[q["rank"]], q["hi"] - 100, q["hi"]))
    assert rule(v, by_rank([50, 70]))[0] == (F, 1)
    assert rule(v, by_rank([50, 60]))[0] == (F, 0)   # a tie of the sums: the smaller anchor rank
    # orientation A (m1 forward) before B on a tie: m1 anchors forward (A) or in reverse (B)
    v = [[cand(90, 1000, 1100)], [cand(90, 5000, 5100)], [], []]
    assert rule(v, fixed(50))[:2] == ((F, 0), (R, cand(50, 1400, 1500)))
    # ... whichever mate anchors: m2's reverse anchor (A, anchored on m2) beats m1's reverse anchor (B, anchored on m1)
    v = [[], [cand(90, 5000, 5100)], [], [cand(90, 2000, 2100)]]
    got = rule(v, fixed(50), pen=40)
    assert got[:2] == ((F, cand(50, 1600, 1700)), (R, 0)) and got[5] == 1
    # orientation A both ways: the rescue anchored on m1 wins
    v = [[cand(90, 1000, 1100)], [], [], [cand(90, 7000, 7100)]]
    got = rule(v, fixed(50), max_span=400, pen=40)
    assert got[:2] == ((F, 0), (R, cand(50, 1300, 1400))) and got[5] == 2 and got[6] == 2
    # 64-bit sums
    big = 2**31 - 1
    v = [[cand(big, 1000, 1100)], [], [], []]
    assert rule(v, fixed(big), pen=0)[5] == 2
