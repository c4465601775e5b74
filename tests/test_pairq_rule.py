"""The mapping quality of read pairs (include/biogpu.h, bg_seed_extend_pairs_mapq_batch) on hand-made candidate lists: the CPU
statement of tests/pairq_oracle.py against values worked out by hand, its agreement with the multi rule where the two must
agree, S1 >= S2 over a random sweep, and the layers that expose the call (header, ctypes prototypes, generated Rust)."""
import ctypes as C
import os
import re

import numpy as np

import multi_oracle as mo
import pairq_oracle as qo
from pair_oracle import MIN_SCORE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAN = (0, 1000)


def c(score, start, length=100):
    return {"score": score, "ref_start": start, "ref_end": start + length}


def rule(m1f, m1r, m2f, m2r, pen=17, min_score=mo.INT32_MIN, cap=60, span=SPAN):
    return qo.pairq_rule(m1f, m1r, m2f, m2r, span[0], span[1], pen, min_score, cap)


def test_two_copies_inside_the_span_range():
    """both copies of mate 2 pair properly with mate 1: nothing tells them apart, and mate 1 itself is unique"""
    recs, det = rule([c(100, 1000)], [], [], [c(100, 1300), c(100, 1600)])
    assert recs[0] == (MIN_SCORE, 1, 1, 60)
    assert recs[1] == (100, 2, 1, 0)
    assert det[1]["class"] == qo.PROPER_ALT_PAIRED and det[1]["S1"] == det[1]["S2"] == 200
    assert det[0]["class"] == qo.PROPER_UNIQUE


def test_an_equal_copy_far_away_costs_pen_unpaired():
    lists = ([c(100, 1000)], [], [], [c(100, 1300), c(100, 50_000)])
    for pen, s in ((17, 100), (0, 100), (150, 100)):
        recs, det = rule(*lists, pen=pen)
        assert recs[1] == (100, 2, 1, 60 * min(pen, s) // s), pen
        assert det[1]["class"] == qo.PROPER_ALT_UNPAIRED and det[1]["S1"] - det[1]["S2"] == pen
        assert recs[0] == (MIN_SCORE, 1, 1, 60)
    assert rule(*lists, pen=0)[0][1][3] == 0
    assert rule(*lists, pen=17)[0][1][3] == 10


def test_a_touching_candidate_is_no_alternative():
    recs, _ = rule([c(100, 1000)], [], [], [c(100, 1300), c(90, 1350)])
    assert recs[1] == (MIN_SCORE, 1, 1, 60)
    recs, _ = rule([c(100, 1000)], [], [], [c(100, 1300), c(90, 1400)])  # ref_end 1400 == ref_start 1400: still touching
    assert recs[1] == (MIN_SCORE, 1, 1, 60)
    recs, _ = rule([c(100, 1000)], [], [], [c(100, 1300), c(90, 1401)])
    assert recs[1] == (90, 2, 1, 60 * 10 // 100)  # (a): 190 against S1 = 200


def test_an_alternative_on_the_other_strand_counts():
    recs, det = rule([c(100, 1000)], [], [c(100, 70_000)], [c(100, 1300)])
    assert recs[1] == (100, 2, 1, 10) and det[1]["class"] == qo.PROPER_ALT_UNPAIRED
    # and one on the other strand at the same place touches the chosen one whatever the strands
    recs, _ = rule([c(100, 1000)], [], [c(100, 1320)], [c(100, 1300)])
    assert recs[1] == (MIN_SCORE, 1, 1, 60)


def test_min_score_removes_an_alternative():
    lists = ([c(100, 1000)], [], [], [c(100, 1300), c(50, 50_000)])
    assert rule(*lists, min_score=51)[0][1] == (MIN_SCORE, 1, 1, 60)
    assert rule(*lists, min_score=50)[0][1] == (50, 2, 1, 60 * (200 - 133) // 100)
    # it removes the member of a proper combination as well: kind (a) goes with it
    lists = ([c(100, 1000)], [], [], [c(100, 1300), c(50, 1600)])
    assert rule(*lists, min_score=51)[0][1] == (MIN_SCORE, 1, 1, 60)
    assert rule(*lists, min_score=50)[0][1] == (50, 2, 1, 60 * 50 // 100)
    # the chosen candidate itself may lie below min_score: it is still reported and judged
    recs, _ = rule(*lists, min_score=150)
    assert recs == [(MIN_SCORE, 1, 1, 60), (MIN_SCORE, 1, 1, 60)]


def test_a_chosen_candidate_scoring_nothing_has_no_quality():
    recs, _ = rule([c(100, 1000)], [], [], [c(0, 1300)])
    assert recs[1] == (MIN_SCORE, 1, 1, 0) and recs[0] == (MIN_SCORE, 1, 1, 60)
    recs, _ = rule([c(100, 1000)], [], [], [c(-3, 1300)], pen=17)
    assert recs[1] == (MIN_SCORE, 1, 1, 0)


def test_caps():
    lists = ([c(100, 1000)], [], [], [c(100, 1300), c(100, 50_000)])
    assert [r[3] for r in rule(*lists, cap=0)[0]] == [0, 0]
    assert [r[3] for r in rule(*lists, cap=254)[0]] == [254, 254 * 17 // 100]
    assert [r[3] for r in rule(*lists, cap=254, pen=1000)[0]] == [254, 254]


def test_kind_a_and_kind_b_each_decide():
    # (a) above (b): the other copy pairs properly too, five below
    recs, det = rule([c(100, 1000)], [], [], [c(100, 1300), c(95, 1600)])
    assert (det[1]["a"], det[1]["b"]) == (195, 178) and recs[1] == (95, 2, 1, 60 * 5 // 100)
    # (b) above (a): the other copy's own proper partner is poor, so leaving the pair costs less than that combination
    recs, det = rule([c(100, 1000), c(50, 40_000)], [], [], [c(100, 1300), c(98, 40_300)])
    assert (det[1]["a"], det[1]["b"]) == (148, 181) and recs[1] == (98, 2, 1, 60 * 19 // 100)
    assert (det[0]["a"], det[0]["b"]) == (148, 133) and recs[0] == (50, 2, 1, 60 * 52 // 100)
    # where the partner is the same in both sums the formula is the multi rule's on the mate's own scores
    recs, det = rule([c(100, 1000)], [], [], [c(80, 1300), c(30, 1600)])
    assert recs[1][3] == mo.mapq_of(80, 30, 60) == 60 * 50 // 80


def test_a_pair_that_is_not_proper_is_two_single_reads():
    m1f, m1r, m2f, m2r = [c(100, 1000), c(80, 5000)], [c(80, 5050), c(70, 9000)], [], [c(100, 90_000)]
    for min_score in (mo.INT32_MIN, 75, 90, 101):
        recs, det = rule(m1f, m1r, m2f, m2r, min_score=min_score)
        for m, (f, r) in enumerate(((m1f, m1r), (m2f, m2r))):
            picks, sub, n_loci, mapq = mo.multi_rule(f, r, 1, min_score, 60)
            assert recs[m] == (sub, n_loci, len(picks), mapq), (min_score, m)
    assert rule(m1f, m1r, m2f, m2r, min_score=101)[0] == [(MIN_SCORE, 0, 0, 0)] * 2
    assert rule(m1f, m1r, m2f, m2r)[0] == [(80, 2, 1, 12), (MIN_SCORE, 1, 1, 60)]
    recs, det = rule(m1f, m1r, [], [])
    assert recs[1] == (MIN_SCORE, 0, 0, 0) and det[1]["class"] == qo.NO_CANDIDATES and det[0]["class"] == qo.SINGLE_RUNNER_UP


def test_s1_is_never_below_s2_random_sweep():
    rng = np.random.default_rng(20)
    n_proper = n_alt = 0
    for _ in range(3000):
        lists = []
        for _v in range(4):
            n = int(rng.integers(0, 5))
            lists.append([c(int(rng.integers(-20, 151)), int(rng.integers(0, 3000)), int(rng.integers(60, 160))) for _ in range(n)])
            lists[-1].sort(key=lambda x: x["ref_start"])
        pen = int(rng.integers(0, 60))
        min_score = int(rng.choice([mo.INT32_MIN, 0, 40, 90]))
        cap = int(rng.choice([0, 1, 60, 254]))
        recs, det = rule(*lists, pen=pen, min_score=min_score, cap=cap, span=(int(rng.integers(0, 300)), int(rng.integers(300, 1500))))
        for m in range(2):
            sub, n_loci, n_rep, mapq = recs[m]
            assert 0 <= mapq <= cap and n_rep <= 1 and n_loci <= 2
            assert (sub == MIN_SCORE) == (n_loci < 2)
            if "S1" in det[m]:
                n_proper += 1
                if det[m]["S2"] is not None:
                    n_alt += 1
                    assert det[m]["S1"] >= det[m]["S2"], (lists, pen)
            else:
                picks, msub, mloci, mmapq = mo.multi_rule(lists[2 * m], lists[2 * m + 1], 1, min_score, cap)
                assert recs[m] == (msub, mloci, len(picks), mmapq)
    assert n_proper > 500 and n_alt > 200  # the sweep met what it is about


def header_struct(name):
    text = open(os.path.join(ROOT, "include", "biogpu.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*" + name + ";", text)
    assert m, name + " is not in include/biogpu.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return re.findall(r"(\w+)\s+(\w+);", body)


def test_the_call_is_exposed_through_every_layer():
    """fails before the feature: the header, the ctypes prototypes and the generated Rust declarations of the new call"""
    from rust_bio_amd import _lib, pipeline
    names = ("bg_seed_extend_pairs_mapq_batch", "bg_seed_extend_pairs_mapq_batch_dev")
    fields = header_struct("bg_pairq_params_t")
    assert fields == [("int32_t", "min_score"), ("uint32_t", "mapq_cap")]
    qp = pipeline.PairQualityParams(min_score=-7, mapq_cap=42).to_c()
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32}
    assert [(n, t) for n, t in qp._fields_] == [(n, ctype[t]) for t, n in fields]
    assert C.sizeof(qp) == 8 and (qp.min_score, qp.mapq_cap) == (-7, 42)
    d = pipeline.PairQualityParams()
    assert (d.min_score, d.mapq_cap) == (-2**31, 60)
    header = open(os.path.join(ROOT, "include", "biogpu.h")).read()
    rust = open(os.path.join(ROOT, "rust", "biogpu-sys", "src", "lib.rs")).read()
    lib = _lib.lib()
    for n in names:
        assert n in _lib.SYMBOLS and re.search(r"\bint " + n + r"\(", header), n
        assert re.search(r"pub fn " + n + r"\(", rust), n
        assert len(getattr(lib, n).argtypes) == (15 if n.endswith("_batch") else 17), n
    assert "pub struct bg_pairq_params_t" in rust
    assert callable(pipeline.seed_extend_pairs_mapq_arrays) and callable(pipeline.seed_extend_pairs_mapq_dev)
