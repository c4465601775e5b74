"""The CPU statement of SMEM-seeded seed-and-extend (tests/smem_seed_oracle.py, include/biogpu.h) on hand-made cases: the GPU
tests hold the device to it, so it is pinned here on its own — the two coordinate formulas against a brute-force search of the
read and of its reverse complement in T, a reverse-palindromic read, and reads hanging off either end of T."""
import functools

import numpy as np

import fmd_cases as fc
import oracle_py as orc
import smem_seed_oracle as sso

F, R = sso.HIT_FORWARD, sso.HIT_REVERSE
SC = (-5, -1, 1, -1)


@functools.lru_cache(maxsize=None)
def index(fwd):
    """(oracle FMDIndex over T$R$, its suffix array, T as an array)"""
    text = fc.full_text(fwd)
    sa = np.asarray(orc.suffix_array(text), np.uint64)
    b = np.frombuffer(bytes(orc.bwt(text, sa)), np.uint8)
    ls = np.asarray(orc.less(b, fc.ALPHA), np.uint64)
    return orc.FMDIndex(b, ls, orc.Occ(b, 3, fc.ALPHA)), sa, np.frombuffer(fwd, np.uint8)


def run(fwd, reads, **kw):
    ofmd, sa, t = index(fwd)
    buf, off = fc.concat(reads)
    return sso.candidates(orc, ofmd, sa, t, orc.make_scoring(*SC), buf, off, **kw)


def find_all(text, pat):
    out, at = [], text.find(pat)
    while at >= 0:
        out.append(at)
        at = text.find(pat, at + 1)
    return out


GENOME = fc.random_dna(3_000, 11)


def test_half_and_proposal_formulas_on_small_numbers():
    n_t = 100  # T at 0 .. 99, '$' at 100, R at 101 .. 200, '$' at 201
    assert sso.half(n_t, 10, 90) == F and sso.half(n_t, 10, 91) is None and sso.half(n_t, 10, 100) is None
    assert sso.half(n_t, 10, 101) == R and sso.half(n_t, 10, 191) == R and sso.half(n_t, 10, 192) is None
    assert sso.half(n_t, 10, 202) is None and sso.half(n_t, 10, sso.SA_NONE) is None and sso.half(n_t, 10, sso.SA_NONE - 1) is None
    # forward: s = p - a, dropped if negative
    assert sso.propose(n_t, 30, 5, 10, 25) == (F, 20) and sso.propose(n_t, 30, 5, 10, 5) == (F, 0) and sso.propose(n_t, 30, 5, 10, 4) is None
    # reverse: R[q ..] holds read[a ..]; the read covers R[q - a .. q - a + L), which is T[n_t - (q - a + L) .. n_t - (q - a))
    assert sso.propose(n_t, 30, 5, 10, 101 + 25) == (R, 100 - (20 + 30))
    assert sso.propose(n_t, 30, 5, 10, 101 + 75) == (R, 0) and sso.propose(n_t, 30, 5, 10, 101 + 76) is None
    # the last start a reverse hit can propose: the match at R's first symbol and the read's last ones
    assert sso.propose(n_t, 30, 25, 5, 101 + 0) == (R, 95)


def test_coordinates_against_a_brute_force_search():
    """exact reads and reads with one substitution, from both strands: every candidate start is where str.find puts the read (or
    its revcomp) in T, on the strand it was drawn from; every occurrence is proposed"""
    rng = np.random.default_rng(5)
    reads, truth = [], []
    for k in range(24):
        L = int(rng.integers(40, 120))
        s = int(rng.integers(0, len(GENOME) - L))
        piece = GENOME[s:s + L]
        if k % 3 == 1:
            piece = fc.with_byte(piece, L // 2, fc.other_base(piece[L // 2]))
        reads.append(fc.revcomp(piece) if k % 2 else piece)
        truth.append((R if k % 2 else F, s))
    res = run(GENOME, reads, min_seed_len=15, pad=10)
    assert not res["panicked"].any() and not res["truncated"].any()
    exp = sso.expected(res)
    for r, (read, (strand, s)) in enumerate(zip(reads, truth)):
        c = res["cands"][r]
        assert [x["start"] for x in c[strand]] == [s] and c[1 - strand] == [], r
        assert exp[r][0] == strand and exp[r][1]["start"] == s
        if r % 3 != 1:  # exact: the brute-force positions of the read / its revcomp in T, and a full-score alignment there
            assert find_all(GENOME, read if strand == F else fc.revcomp(read)) == [s]
            assert exp[r][1]["score"] == len(read) and exp[r][1]["ref_start"] == s
        assert exp[r][3] >= 1 and exp[r][2] == 1
    assert res["rows"] == int(res["n_hits"].sum())


def test_one_strand_at_a_time_drops_the_other_half():
    reads = [GENOME[500:580], fc.revcomp(GENOME[900:980])]
    both = run(GENOME, reads)
    fwd, rev = run(GENOME, reads, strands=sso.STRAND_FORWARD), run(GENOME, reads, strands=sso.STRAND_REVERSE)
    assert [x["start"] for x in both["cands"][0][F]] == [500] and [x["start"] for x in both["cands"][1][R]] == [900]
    assert fwd["cands"][0][F][0]["start"] == 500 and fwd["cands"][1] == {F: [], R: []}
    assert rev["cands"][1][R][0]["start"] == 900 and rev["cands"][0] == {F: [], R: []}
    assert list(fwd["n_hits"]) == [1, 0] and list(rev["n_hits"]) == [0, 1] and list(both["n_hits"]) == [1, 1]
    assert fwd["rows"] == rev["rows"] == both["rows"] == 2  # every row K6 resolves is counted, whichever strand runs


def test_a_reverse_palindrome_starts_at_the_same_place_on_both_strands_and_forward_wins():
    g = bytearray(GENOME)
    s = GENOME[100:130]
    pal = s + fc.revcomp(s)
    g[1_000:1_060] = pal
    g = bytes(g)
    assert fc.revcomp(pal) == pal and find_all(g, pal) == [1_000]
    res = run(g, [pal])
    c = res["cands"][0]
    assert [x["start"] for x in c[F]] == [1_000] and [x["start"] for x in c[R]] == [1_000]
    assert c[F][0]["score"] == c[R][0]["score"] == 60
    assert sso.expected(res)[0][0] == F and sso.expected(res)[0][2] == 2


def test_reads_hanging_off_either_end_are_dropped_on_the_right_side():
    """a read whose first 20 bases lie in front of T (the rest is T's head), and one whose last 20 lie behind T's end: the forward
    strand drops the first (p < a) and keeps the second; of their revcomps the reverse strand drops the second's — the start of
    revcomp(read) would be negative — and keeps the first's (a start whose window is clipped at n_t)"""
    n_t = len(GENOME)
    junk = fc.random_dna(20, 99)
    head, tail = junk + GENOME[:60], GENOME[-60:] + junk
    res = run(GENOME, [head, tail, fc.revcomp(head), fc.revcomp(tail)], min_seed_len=19)
    c = res["cands"]
    assert c[0] == {F: [], R: []} and list(res["n_hits"][:1]) == [1]  # the row counts, the proposal is dropped
    assert [x["start"] for x in c[1][F]] == [n_t - 60] and c[1][R] == []
    assert c[1][F][0]["wlo"] == n_t - 60 - 25
    # revcomp(head) = revcomp(T[:60]) + revcomp(junk): on R it matches at q = n_t - 60 with a = 0; revcomp of it is `head`, whose
    # start on T would be -20
    assert c[2] == {F: [], R: []} and int(res["n_hits"][2]) == 1
    # revcomp(tail) = revcomp(junk) + revcomp(T[-60:]): a = 20, q = 0; its revcomp `tail` starts at n_t - 60
    assert [x["start"] for x in c[3][R]] == [n_t - 60] and c[3][F] == []
    exp = sso.expected(res)
    assert [e[0] for e in exp] == [sso.HIT_NONE, F, sso.HIT_NONE, R]


def test_votes_cap_and_panic_flags():
    seg = GENOME[200:260]
    g = GENOME[:1_000] + seg + GENOME[1_000:2_000] + seg + GENOME[2_000:]
    # three copies of seg: a read inside it votes with max_occ = 3 and not with 2
    assert len(run(g, [seg], max_occ=3)["cands"][0][F]) == 3
    low = run(g, [seg], max_occ=2)
    assert low["cands"][0] == {F: [], R: []} and low["rows"] == 0
    # a chimera of three loci has three records; max_smems = 2 uses the first two in push order and says so
    chim = GENOME[300:330] + GENOME[1_500:1_530] + GENOME[2_500:2_530]
    full, cut = run(GENOME, [chim], max_smems=3), run(GENOME, [chim], max_smems=2)
    assert not full["truncated"][0] and cut["truncated"][0]
    assert len(full["cands"][0][F]) == 3 and len(cut["cands"][0][F]) == 2
    assert {x["start"] for x in cut["cands"][0][F]} < {x["start"] for x in full["cands"][0][F]}
    # a byte beyond `less` panics in the reference: no candidates, flagged
    bad = run(GENOME, [fc.with_byte(GENOME[400:460], 30, 0xFF), GENOME[400:460]])
    assert list(bad["panicked"]) == [True, False] and bad["cands"][0] == {F: [], R: []} and len(bad["cands"][1][F]) == 1
