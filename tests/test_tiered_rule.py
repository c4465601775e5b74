"""The tiered seed-and-extend call without a GPU: its two entry points in the library and the header, the choice between a read's
two tier winners as the device states it (csrc/seed_tier_rule.h, compiled here with the host compiler into a stand-alone program,
under the address and undefined-behaviour sanitizers) against the Python statement (tests/tiered_seed_oracle.py: better), and the
CPU statement of the whole call held to what it must do on its own."""
import functools
import itertools
import os
import shutil
import subprocess

import numpy as np

import fmd_cases as fc
import oracle_py as orc
import smem_seed_oracle as sso
import tiered_seed_oracle as tso
from rust_bio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, R, NONE = sso.HIT_FORWARD, sso.HIT_REVERSE, sso.HIT_NONE
SC = (-5, -1, 1, -1)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "seed_tier_rule.h"
// stdin: lines of "score1 strand1 window1 score2 strand2 window2"; stdout: 1 where tier 2's winner is the answer, else 0
int main() {
    long long s1, s2;
    unsigned st1, st2;
    unsigned long long w1, w2;
    while (std::scanf("%lld %u %llu %lld %u %llu", &s1, &st1, &w1, &s2, &st2, &w2) == 6) {
        const bgtier::TierHit a{(int32_t)s1, (uint8_t)st1, (uint64_t)w1}, b{(int32_t)s2, (uint8_t)st2, (uint64_t)w2};
        std::printf("%d\n", bgtier::tier2_wins(a, b) ? 1 : 0);
    }
    return 0;
}
"""


def test_the_library_exports_and_the_header_declares_the_tiered_call():
    hdr = open(os.path.join(ROOT, "include", "biogpu.h")).read()
    for name in ("bg_seed_extend_tiered_batch", "bg_seed_extend_tiered_batch_dev"):
        assert hasattr(_lib.lib(), name), name
        assert name + "(" in hdr and name in _lib.SYMBOLS
    assert "bg_tiered_seed_params_t" in hdr and (_lib.TIER_NONE, _lib.TIER_FIRST, _lib.TIER_SECOND) == (0, 1, 2)


def test_the_device_rule_header_agrees_with_the_python_statement(tmp_path):
    """every pair of tier winners over scores {MIN, -1, 0, 5} x both strands x window_start {0, 1}, and either tier (or both) absent"""
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "tier_rule.cpp", tmp_path / "tier_rule"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "rust-bio_amd", "csrc"), str(src), "-o", str(exe)])
    present = list(itertools.product((tso.MIN_SCORE, -1, 0, 5), (F, R), (0, 1)))
    sides = [tso.ABSENT] + present
    grid = list(itertools.product(sides, sides))
    assert len(grid) == 17 * 17
    text = "".join("%d %d %d %d %d %d\n" % (a + b) for a, b in grid)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stderr
    got = [int(v) for v in out.stdout.split()]
    assert got == [int(tso.better(a, b)) for a, b in grid]
    # the order of the rule, spelled out
    assert not tso.better((5, F, 0), (5, F, 0)) and tso.better((5, R, 0), (5, F, 1)) and not tso.better((5, F, 1), (5, R, 0))
    assert tso.better((5, R, 1), (5, R, 0)) and tso.better((0, F, 0), (5, R, 1)) and not tso.better(tso.ABSENT, tso.ABSENT)
    assert tso.better(tso.ABSENT, (tso.MIN_SCORE, R, 1)) and not tso.better((tso.MIN_SCORE, R, 1), tso.ABSENT)


GENOME = fc.random_dna(4_000, 23)


@functools.lru_cache(maxsize=None)
def index(fwd):
    text = np.frombuffer(fc.full_text(fwd), np.uint8)
    sa = np.asarray(orc.suffix_array(text), np.uint64)
    b = np.frombuffer(bytes(orc.bwt(text, sa)), np.uint8)
    ls = np.asarray(orc.less(b, fc.ALPHA), np.uint64)
    occ = orc.Occ(b, 3, fc.ALPHA)
    return (b, ls, occ, sa), orc.FMDIndex(b, ls, occ), np.frombuffer(fwd, np.uint8)


def run(reads, **kw):
    idx, ofmd, t = index(GENOME)
    buf, off = fc.concat(reads)
    return tso.tiered(orc, idx, ofmd, t, orc.make_scoring(*SC), buf, off, **kw)


def brief(want):
    """an `expected` list as plain values: (strand, the candidate's start, score, reference interval and operations, the counts)"""
    return [(st, None if c is None else (c["start"], c["score"], c["ref_start"], c["ref_end"], c["ops"].tobytes()), nc, nsh)
            for st, c, nc, nsh in want]


def reads_of_both_strands(n, seed, sub=None):
    rng = np.random.default_rng(seed)
    reads, truth = [], []
    for k in range(n):
        L = int(rng.integers(40, 151))
        s = int(rng.integers(0, len(GENOME) - L))
        piece = GENOME[s:s + L]
        if sub:
            piece = fc.substituted(piece, 20, start=15)
        reads.append(fc.revcomp(piece) if k % 2 else piece)
        truth.append((R if k % 2 else F, s, L))
    return reads, truth


def test_without_substitutions_tier_one_places_every_read_at_its_origin_on_both_strands():
    reads, truth = reads_of_both_strands(40, 1)
    res = run(reads)
    assert res["status"] == tso.OK and res["totals"][2] == 0 and not res["tier"].any()
    for (strand, cand, nc, nsh), (st, s, L) in zip(res["want"], truth):
        assert strand == st and cand["ref_start"] == s and cand["ref_end"] == s + L and cand["score"] == L and nc == 1
        assert nsh == (L - 20) // 10 + 1  # one row per window, all in the half of the read's strand


def test_reseeding_nobody_is_tier_one_and_reseeding_everybody_places_the_reads_no_window_survives_on():
    reads, truth = reads_of_both_strands(24, 2)
    hard, hard_truth = reads_of_both_strands(12, 3, sub=True)
    reads, truth = reads + hard, truth + hard_truth
    none = run(reads, reseed_below=tso.MIN_SCORE)
    assert brief(none["want"]) == brief(none["first"]) and none["totals"][2] == 0 and not none["tier"].any()
    n_easy = 24
    assert all(w[0] == NONE and w[2] == 0 for w in none["want"][n_easy:])  # a substitution in every window: tier 1 finds nothing
    every = run(reads, reseed_below=tso.INT32_MAX)
    assert every["totals"][2] == len(reads) and (every["tier"][:n_easy] == tso.TIER_FIRST).all()  # an equal hit: tier 1 is kept
    assert (every["tier"][n_easy:] == tso.TIER_SECOND).all()
    for (strand, cand, _, _), (st, s, L) in zip(every["want"], truth):
        assert strand == st and cand["ref_start"] == s and cand["ref_end"] == s + L
    for w1, w2 in zip(none["want"][:n_easy], every["want"][:n_easy]):
        assert w2[2] == 2 * w1[2] and w2[3] > w1[3] and w2[1]["score"] == w1[1]["score"]  # the counts are sums over the tiers
    # in between: only the reads below the threshold
    some = run(reads, reseed_below=1)
    assert list(np.nonzero(some["tier"])[0]) == list(range(n_easy, len(reads))) and some["totals"][2] == len(reads) - n_easy
    assert brief(some["want"])[n_easy:] == brief(every["want"])[n_easy:] and brief(some["want"])[:n_easy] == brief(none["want"])[:n_easy]


def test_a_window_out_of_the_alphabet_does_not_vote_and_the_others_do():
    base = GENOME[1_000:1_100]
    res = run([fc.with_byte(base, 40, 0xFF), base])
    assert res["status"] == tso.OUT_OF_ALPHABET
    (st0, c0, nc0, nsh0), (st1, c1, nc1, nsh1) = res["want"]
    assert st0 == st1 == F and c0["ref_start"] == c1["ref_start"] == 1_000 and nc0 == nc1 == 1
    assert nsh1 == 9 and nsh0 == 7  # the windows at 30 and 40 hold byte 40 and reach it
