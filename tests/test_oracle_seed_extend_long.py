"""The cases of tests/test_gpu_seed_extend_long.py without a GPU: tests/seed_long_cases.py held to the oracle's composition
(oracle/pipeline.cpp; tests/pair_oracle.py and tests/rescue_oracle.py for every candidate, pairs and rescue) before any kernel
sees it.  Every planted read is placed at its locus with the score its edits imply, its operations hold the planted indel,
the clipped windows are clipped, the repeat reads have two candidates of distinct scores, and no two candidates of a read tie
for its best score."""
import numpy as np
import pytest

import pair_oracle as po
import seed_long_cases as lc
from rescue_cases import oracle_rescue
from rust_bio_amd.pipeline import PairParams, RescueParams
from test_gpu_score_edges import F, k1p_admits
from test_gpu_seed_extend_pairs import oracle_pairs

MIN_SCORE = po.MIN_SCORE
NAMES = list(lc.CLASSES)
PP = PairParams(0, lc.MAX_SPAN, 17)


def rescue_params(L):
    """a placed mate with a substitution every 15 bases scores about 0.87 L; a random mate scores below 0"""
    return RescueParams(2, L // 2)


def test_each_class_lands_where_the_table_says():
    got = {n: lc.fill_of(c.get("sc", lc.SC), c["L"], c["L"] + 2 * c["pad"]) for n, c in lc.CLASSES.items()}
    assert got == {"A": F["K1P"], "B": F["K1P"], "C": F["K1P"], "D": F["K1_NARROW"], "E": F["K1_NARROW"], "F512": F["K1_NARROW"],
                   "F513": F["K1_NARROW"], "G": F["K1_NARROW"], "H": F["K1_NARROW"], "W": F["K1_WIDE"]}
    c, d = lc.CLASSES["C"], lc.CLASSES["D"]
    assert 5 * (c["L"] + 2 * c["pad"] + 2) == 2040 and k1p_admits(5, c["L"], c["L"] + 2 * c["pad"])
    assert not k1p_admits(5, d["L"], d["L"] + 2 * d["pad"]) and k1p_admits(5, d["L"], d["L"] + 2 * d["pad"] - 2)
    assert 9000 * (1500 + 1564 + 8) >= 1 << 24 > 5 * (2049 + 2113 + 8)
    # the rescue alignments of the pair classes (a mate against a window of max_span)
    assert lc.fill_of(lc.SC, 193, lc.MAX_SPAN) == F["K1_NARROW"]
    for name in NAMES:
        cs = lc.case(name)
        assert (cs.L - cs.seed_len) // cs.stride + 1 <= 64 and ((cs.L - cs.seed_len) // cs.stride + 1) * cs.max_occ <= 1024
        assert len(cs.items) <= 8 if name == "H" else 30 <= len(cs.items) <= 60


def long_run(ops, kind):
    """the longest run of `kind` in a list of operations"""
    best = run = 0
    for o in ops:
        run = run + 1 if o == kind else 0
        best = max(best, run)
    return best


@pytest.mark.parametrize("name", NAMES)
def test_oracle_places_every_planted_read(name):
    cs = lc.case(name)
    h, ops, ostride = lc.oracle_single(name)
    bh, bstrand, bops, _ = lc.oracle_both(name)
    kinds = {it.kind for it in cs.items}
    want = {"exact", "subs", "rep_a", "right0", "random"} | ({"del_last", "ins_first", "rev_subs"} if name == "H" else
                                                              {"del_first", "del_middle", "del_last", "ins_first", "ins_middle", "ins_last",
                                                               "left0", "left2", "right3", "over_right", "over_left", "rev", "rev_subs", "rep_b"})
    assert want <= kinds
    n_planted = 0
    for r, it in enumerate(cs.items):
        for hits, o, fwd_only in ((h, ops, True), (bh, bops, False)):
            a = hits[r]
            if it.s is None or (fwd_only and it.strand == 1):
                assert a["aln"]["score"] == MIN_SCORE and a["n_candidates"] == 0, (r, it.kind)
                continue
            n_planted += 1
            if it.score is None:  # (class W: placed, within the indel's length of the locus)
                assert a["aln"]["score"] > MIN_SCORE, (r, it.kind)
                assert abs(int(a["ref_start"]) - it.s) <= lc.INDEL and abs(int(a["ref_end"]) - it.e) <= lc.INDEL, (r, it.kind)
                continue
            assert (int(a["ref_start"]), int(a["ref_end"]), int(a["aln"]["score"])) == (it.s, it.e, it.score), (r, it.kind)
            if not fwd_only:
                assert bstrand[r] == it.strand, (r, it.kind)
            if it.indel:
                k = int(a["aln"]["n_ops"])
                got = (o[r * ostride:r * ostride + k] & np.uint64(0xFF)).tolist()
                assert long_run(got, it.indel[0]) == it.indel[1] >= min(lc.INDEL, cs.pad), (r, it.kind)
    assert n_planted >= (10 if name == "H" else 50)
    # the ends: windows clipped at 0 and at n_text
    for r in cs.of_kind("left"):
        assert h["window_start"][r] == 0 and cs.items[r].s < cs.pad
        assert int(h["aln"]["ylen"][r]) == cs.items[r].s + len(cs.items[r].x) + cs.pad
    for r in cs.of_kind("right", "over_right"):
        assert int(h["window_start"][r]) + int(h["aln"]["ylen"][r]) == lc.N_TEXT
        assert int(h["aln"]["ylen"][r]) < len(cs.items[r].x) + 2 * cs.pad
    for r in cs.of_kind("over_left"):
        assert h["n_seed_hits"][r] > 0 and h["n_candidates"][r] == 0  # every proposal is negative: counted, dropped
    # the longest window of the class is reached: the fill family is decided by lengths that occur
    assert int(h["aln"]["ylen"].max()) == cs.L + 2 * cs.pad and int(h["aln"]["xlen"].max()) == cs.L
    if name == "G":
        lens = np.diff(cs.off).astype(int).tolist()
        assert set(lc.G_LENGTHS) <= set(lens) and min(lens) == 1
        assert all(h["n_seed_hits"][r] == 0 for r in cs.of_kind("short"))


@pytest.mark.parametrize("name", NAMES)
def test_candidates_never_tie_and_the_repeat_gives_two(name):
    cs = lc.case(name)
    cands, nh, _, _ = lc.candidates(name)
    for r, it in enumerate(cs.items):
        sc = sorted((c["score"] for c in cands[2 * r] + cands[2 * r + 1]), reverse=True)
        assert len(sc) < 2 or sc[0] > sc[1], (r, it.kind, sc)
        if it.kind.startswith("rep_"):
            mine = cands[2 * r]
            assert len(mine) >= 2 and len({c["score"] for c in mine}) >= 2, (r, sc)
            assert {c["ref_start"] for c in mine} >= {it.s, it.s + (lc.REP_B - lc.REP_A) * (1 if it.kind == "rep_a" else -1)}
        if it.indel:
            assert len(cands[2 * r]) == 1, (r, it.kind)  # the broken side proposes nothing
    if lc.CLASSES[name]["fill"] == "K1P":  # enough candidates in one pass for K1p to pair its jobs by length, of several lengths
        fwd = [c for r in range(len(cs.items)) for c in cands[2 * r]]
        assert len(fwd) >= 64 and len({int(c["rec"]["xlen"]) for c in fwd}) >= 5


@pytest.mark.parametrize("name", lc.PAIR_CLASSES)
def test_pairs_and_rescue_on_the_pair_batches(name):
    cs = lc.pair_case(name)
    g, text = lc.genome()
    sa, b, ls = lc.index()
    cands = lc.candidates(name, paired=True)[0]
    for v in range(0, len(cands), 2):
        sc = sorted((c["score"] for c in cands[v] + cands[v + 1]), reverse=True)
        assert len(sc) < 2 or sc[0] > sc[1], (v // 2, sc)
    er, ep, _ = oracle_pairs(b, ls, sa, text, lc.N_TEXT, cs.reads, cs.off, PP, scores=cs.sc, **cs.seed_kw)
    want = oracle_rescue(b, ls, sa, text, lc.N_TEXT, cs.reads, cs.off, PP, rescue_params(cs.L), scores=cs.sc, **cs.seed_kw)
    rr, rp, rescued = want[:3]
    seen = set()
    for p, (kind, a, f, bad) in enumerate(cs.info):
        seen.add(kind)
        if kind in ("frag", "overlap", "end"):
            assert ep[p][0] and ep[p][1] == f and rescued[p] == 0, (p, kind)
            assert min(er[2 * p + m][1]["ref_start"] for m in (0, 1)) == a and max(er[2 * p + m][1]["ref_end"] for m in (0, 1)) == a + f, (p, kind)
            if kind == "overlap":
                assert f < cs.L and er[2 * p][1]["ref_start"] == er[2 * p + 1][1]["ref_start"] == a
                assert er[2 * p][1]["ref_end"] == er[2 * p + 1][1]["ref_end"] == a + f
        elif kind in ("broken", "end_broken"):
            assert not ep[p][0] and er[2 * p + bad][1] is None, (p, kind)  # no seed of the broken mate survives
            assert rescued[p] == bad + 1 and rp[p][0] and rp[p][1] == f, (p, kind)
            m = rr[2 * p + bad][1]
            n_sub = len(np.arange(7, len(cs.items[2 * p + bad].x), 15))
            assert m["score"] == len(cs.items[2 * p + bad].x) - 2 * n_sub and m["ref_end"] - m["ref_start"] == len(cs.items[2 * p + bad].x)
        else:
            assert not ep[p][0] and rescued[p] == 0 and want[3] > 0, (p, kind)
    assert seen == {"frag", "overlap", "broken", "random", "end", "end_broken"}
    assert max(int(c["rec"]["ylen"]) for r in rr for c in [r[1]] if c is not None) == lc.MAX_SPAN  # a rescue window of max_span
