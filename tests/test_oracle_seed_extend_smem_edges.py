"""The cases of tests/test_gpu_seed_extend_smem_edges.py without a GPU: every read of tests/smem_edges.py is held to what it was
built for under the oracle's statement of the call (tests/smem_seed_oracle.py: all_smems, the suffix array of T$R$,
Aligner::semiglobal) — record count, rows per half, rows counted but dropped as proposals, kept starts, truncation — and the
statement's three rules (`half`, `propose`, `merged`) to hand-worked numbers at every equality of the header's conditions."""
import functools

import numpy as np
import pytest

import oracle_py as orc
import smem_edges as se
import smem_seed_oracle as sso

F, R, NONE = sso.HIT_FORWARD, sso.HIT_REVERSE, sso.HIT_NONE
SC = (-5, -1, 1, -1)


@functools.lru_cache(maxsize=None)
def oracle(name, strands=sso.STRAND_BOTH, pad=25, only=None):
    """the statement on a batch (`only`: on the reads of these kinds)"""
    c = se.corpus()
    cs = c.cases[name]
    buf, off = c.reads[name]
    if only is not None:
        cs = [x for x in cs if x["kind"].split("/")[0] in only]
        buf, off = se.fc.concat([x["x"].tobytes() for x in cs])
    return cs, buf, off, sso.candidates(orc, c.ofmd, c.sa, c.fwd, orc.make_scoring(*SC), buf, off, strands=strands, **c.params(name, pad))


# ------------------------------------------------------------------------------------------------------------- the corpus


def test_every_listed_case_is_present():
    """100 % of the cases, counted on the restatement (records and suffix array), not on the planting's bookkeeping"""
    c = se.corpus()
    for name in se.SHAPES:
        cs, rs = c.cases[name], c.restate(name)
        P, cap = se.SHAPES[name]["max_smems"], se.SHAPES[name]["max_occ"]
        assert P * cap == 1024
        by = {}
        for x, d in zip(cs, rs):
            by.setdefault(x["kind"], []).append(d)
        # distinct: nh hits, nh candidates, one per count up to 129 and one at 1024
        nh = sorted(d["nh"] for d in by["distinct"])
        assert nh == sorted(v for v in se.NH_VALUES if v <= 129) + [1024]
        assert all(d["n_candidates"] == d["nh"] for d in by["distinct"])
        # stacked: P rows per start, both strands
        assert sorted(d["nh"] for d in by["stacked"]) == [512, 513, 1023, 1024, 1024]
        for d in by["stacked"]:
            assert d["n_candidates"] == -(-d["nh"] // P) and d["kept"][F] and d["kept"][R]
        # the halves
        halves = {(d["rows"][F], d["rows"][R]) for d in by["split"]}
        assert halves == {(700, 324), (1, 1023), (1023, 1), (512, 512)}
        # truncation at the limit: one record more than max_smems, 1024 rows from the first max_smems
        (d,) = by["truncated"]
        assert d["truncated"] and d["n_records"] == P + 1 and d["nh"] == 1024
        assert not any(d["truncated"] for k, ds in by.items() if k != "truncated" for d in ds)
        # the ends of T, each with its reverse complement: a start at 0, a window clipped at n_t, rows counted and dropped
        for kind, start, dropped in (("head", 0, 0), ("tail", c.n_t - se.END_L, 0), ("over_head_10", None, 1), ("over_head_1", None, 1),
                                     ("over_tail_10", c.n_t - se.END_L + 10, 0), ("over_tail_1", c.n_t - se.END_L + 1, 0),
                                     ("at_head", 0, 0), ("at_tail", c.n_t - se.END_L, 0)):
            for k, h in ((kind, F), (kind + "/rc", R)):
                (d,) = by[k]
                assert d["rows"][h] == 1 and d["rows"][1 - h] == 0 and d["dropped"][h] == dropped, k
                assert d["kept"][h] == ([] if start is None else [start]) and d["n_seed_hits"] == 1, k
        (d,) = by["sentinel"]
        assert d["rows"] == {F: 0, R: 0, None: 1} and d["n_seed_hits"] == 0 and d["nh"] == 1
        # heavy reads next to the pass boundaries of the device flavour, ordinary reads among the others
        i, j, k = c.heavy(name)
        assert rs[i]["nh"] == rs[j]["nh"] == rs[k]["nh"] == 1024 and k == len(cs) - 1 and len(by["ordinary"]) >= 24
    # the merge cases under every pad, on both strands
    for pad in se.PADS:
        m = pad // 2
        rs = c.restate("merge", pad)
        gaps = {h: set() for h in (F, R)}
        for x, d in zip(c.cases["merge"], rs):
            for h in (F, R):
                p = sorted(set(d["props"][h]))
                gaps[h] |= {(b - a, b in d["kept"][h]) for a, b in zip(p, p[1:])}
                if "kept" in x:
                    assert len(d["kept"][h]) == x["kept"][pad][h]
        for h in (F, R):
            if m:  # proposals pad / 2 apart merge, pad / 2 + 1 apart do not
                assert (m, False) in gaps[h] and (m + 1, True) in gaps[h], (pad, h)
            assert (1, m == 0) in gaps[h]  # one apart: kept only where pad / 2 is 0
        by = {}
        for x, d in zip(c.cases["merge"], rs):
            by.setdefault(x["kind"], []).append(d)
        for d in by["chain_12"]:  # s, s + 12, s + 24, ..: the third start is kept
            h = F if d["props"][F] else R
            s = min(d["props"][h])
            assert sorted(d["props"][h]) == [s + 12 * i for i in range(5)]
            assert d["kept"][h] == ([s, s + 24, s + 48] if m == 12 else sorted(d["props"][h]))
        for d in by["gap_0_1"]:  # equal proposals of different rows merge whatever the pad
            h = F if d["props"][F] else R
            assert len(d["props"][h]) == 10 and len(set(d["props"][h])) == 7
        (d,) = by["palindrome"]
        assert d["n_records"] == 1 and d["kept"][F] == d["kept"][R] and len(d["kept"][F]) == 1
        apart = sorted(d["kept"][R][0] - d["kept"][F][0] for d in by["strands_5_apart"])
        assert apart == [-5, 5] and all(d["kept"][F] == d["kept"][R] for d in by["strands_equal"])


# ------------------------------------------------------------------------------------------------ the oracle on the cases


def hold(cs, res, rs, what):
    """a `candidates` result against the restatement, read by read"""
    want = sso.expected(res)
    assert not res["panicked"].any()
    for r, (x, d) in enumerate(zip(cs, rs)):
        got = res["cands"][r]
        assert int(res["n_hits"][r]) == d["n_seed_hits"], (what, r, x["kind"])
        for h in (F, R):
            assert [v["start"] for v in got[h]] == d["kept"][h], (what, r, x["kind"], h)
        assert bool(res["truncated"][r]) == d["truncated"], (what, r)
        assert want[r][2] == d["n_candidates"] and want[r][3] == d["n_seed_hits"]
        assert (want[r][0] == NONE) == (d["n_candidates"] == 0)
    assert res["rows"] == sum(d["nh"] for d in rs)
    return want


@pytest.mark.parametrize("name", list(se.SHAPES))
def test_oracle_on_the_count_cases(name):
    c = se.corpus()
    cs, buf, off, res = oracle(name)
    rs = c.restate(name)
    want = hold(cs, res, rs, name)
    for r, (x, d) in enumerate(zip(cs, rs)):
        if x["kind"] == "ordinary":  # placed where it was cut, on the strand it was cut from
            assert want[r][0] == x["truth"][0] and want[r][1]["ref_start"] == x["truth"][1], r
        if x["kind"].startswith(("head", "tail")):  # exact reads: the full score at the start the case names
            h = R if x["kind"].endswith("/rc") else F
            assert want[r][0] == h and want[r][1]["score"] == len(x["x"]) and want[r][1]["ref_start"] == d["kept"][h][0], r
        if x["kind"].startswith("over_tail"):  # the window is clipped at n_t, the bases that hang over are not aligned to T
            cand = want[r][1]
            assert cand["wlo"] + int(cand["rec"]["ylen"]) == c.n_t and cand["start"] + len(x["x"]) > c.n_t, r
        if x["kind"].startswith("over_head") or x["kind"] == "sentinel":  # a row, counted or not, and no candidate
            assert want[r][0] == NONE and want[r][2] == 0 and want[r][3] == (0 if x["kind"] == "sentinel" else 1), r


@pytest.mark.parametrize("strands", [sso.STRAND_FORWARD, sso.STRAND_REVERSE])
def test_oracle_one_strand_at_a_time(strands):
    """n_seed_hits counts the rows in the half of a strand that ran, dropped proposals included; the other half's do not count"""
    c = se.corpus()
    kinds = ("head", "tail", "over_head_10", "over_head_1", "over_tail_10", "over_tail_1", "at_head", "at_tail", "sentinel", "ordinary")
    cs, buf, off, res = oracle("s64", strands, only=kinds)
    rs = se.restate(c.ofmd, c.sa, c.n_t, buf, off, strands=strands, **c.params("s64"))
    hold(cs, res, rs, strands)
    h = F if strands == sso.STRAND_FORWARD else R
    both = se.restate(c.ofmd, c.sa, c.n_t, buf, off, **c.params("s64"))
    assert [d["n_seed_hits"] for d in rs] == [d["rows"][h] for d in both]
    assert sum(d["n_seed_hits"] > d["n_candidates"] for d in rs) >= 2  # counted, dropped
    cs, buf, off, res = oracle("merge", strands)
    hold(cs, res, se.restate(c.ofmd, c.sa, c.n_t, buf, off, strands=strands, **c.params("merge")), strands)


@pytest.mark.parametrize("pad", se.PADS)
def test_oracle_on_the_merge_cases(pad):
    c = se.corpus()
    cs, buf, off, res = oracle("merge", pad=pad)
    want = hold(cs, res, c.restate("merge", pad), pad)
    for r, x in enumerate(cs):
        if x["kind"] in ("palindrome", "strands_equal"):  # the same start on both strands: two candidates
            assert want[r][2] == 2
        if x["kind"] == "palindrome":                      # ... of equal score, and the forward one wins
            got = res["cands"][r]
            assert got[F][0]["score"] == got[R][0]["score"] == 60 and want[r][0] == F


# ------------------------------------------------------------------------------------------------------------- the rules


def test_half_at_its_equalities():
    n_t = 10  # T at 0 .. 9, '$' at 10, R at 11 .. 20, '$' at 21
    assert sso.half(n_t, 4, 6) == F       # p + len == n_t
    assert sso.half(n_t, 4, 7) is None    # one past: the match holds the sentinel at 10
    assert sso.half(n_t, 4, 10) is None   # p == n_t: starts on the sentinel
    assert sso.half(n_t, 4, 11) == R      # p == n_t + 1
    assert sso.half(n_t, 4, 17) == R      # p + len == 2 n_t + 1
    assert sso.half(n_t, 4, 18) is None   # one past: holds the last sentinel
    assert sso.half(n_t, 10, 0) == F and sso.half(n_t, 10, 11) == R and sso.half(n_t, 11, 0) is None and sso.half(n_t, 11, 11) is None
    assert sso.half(n_t, 1, 21) is None and sso.half(n_t, 1, 22) is None and sso.half(n_t, 1, sso.SA_NONE) is None


def test_propose_at_its_equalities():
    n_t, L = 10, 6
    # forward: s = p - a; p == a is start 0, one less is dropped
    assert sso.propose(n_t, L, 2, 3, 2) == (F, 0) and sso.propose(n_t, L, 2, 3, 1) is None and sso.propose(n_t, L, 2, 3, 5) == (F, 3)
    # ... the read may hang over the end of T: the piece ends at n_t, the start stays below it
    assert sso.propose(n_t, L, 0, 3, 7) == (F, 7)
    # reverse, q = p - n_t - 1: s = n_t + a - q - L; q + L == n_t + a is start 0, one past is dropped
    assert sso.propose(n_t, L, 2, 3, 11 + 6) == (R, 0) and sso.propose(n_t, L, 2, 3, 11 + 7) is None
    assert sso.propose(n_t, L, 2, 3, 11 + 0) == (R, 6)
    # ... the largest start a reverse row can propose: the read's last bases at R's first (a + len == L, q == 0)
    assert sso.propose(n_t, L, 3, 3, 11) == (R, 7)
    # rows in neither half propose nothing
    assert sso.propose(n_t, L, 0, 3, 8) is None and sso.propose(n_t, L, 0, 3, 10) is None and sso.propose(n_t, L, 0, 3, sso.SA_NONE) is None


def test_merged_compares_with_the_last_start_kept():
    assert sso.merged([0, 12], 25) == [0] and sso.merged([0, 13], 25) == [0, 13]
    assert sso.merged([0, 12], 24) == [0] and sso.merged([0, 13], 24) == [0, 13]
    assert sso.merged([24, 0, 12], 25) == [0, 24]                      # 24 is 12 from the start before it, 24 from the last one kept
    assert sso.merged([0, 12, 24, 36, 48], 25) == [0, 24, 48]
    assert sso.merged([5, 5, 6], 1) == [5, 6] and sso.merged([5, 5, 6], 0) == [5, 6] and sso.merged([5, 5, 5], 0) == [5]
    assert sso.merged([0, 1], 2) == [0] and sso.merged([0, 1], 3) == [0] and sso.merged([], 25) == []
    for pad in se.PADS:
        starts = list(np.random.default_rng(pad).integers(0, 400, size=200))
        assert sso.merged(starts, pad) == se.merged(starts, pad)
