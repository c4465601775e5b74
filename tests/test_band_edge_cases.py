"""The pairs of tests/band_edge_cases.py hold what they are for — shown with the CPU oracle alone, without a GPU: match
totals and per-position maxima on the builder's caps, the no-match family's buffer residues, the join flavour every
length selects, the order the sub-batch tests rely on.  The case file's copies of the limits are compared with the
sources, and the product's host builder — what tests/test_gpu_band_builder_edges.py compares the device builder with —
is compared with the oracle's Band::create column by column on every pair."""
import os
import re

import numpy as np
import pytest

import band_edge_cases as ec
import oracle_py as orc
from rust_bio_amd import _lib
from rust_bio_amd.banded import Aligner
from rust_bio_amd.pairwise import MIN_SCORE, Scoring

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rust-bio_amd", "csrc")


@pytest.fixture(scope="module")
def short():
    return ec.short_batch()


@pytest.fixture(scope="module")
def longs():
    return [ec.long_pair(length) for length in ec.LONG_L]


@pytest.fixture(scope="module")
def stats(short, longs):
    return {p.name: ec.match_stats(orc.find_kmer_matches, p.x, p.y) for p in short + longs}


def expected_handed_over(pairs, k=ec.K):
    return sum(ec.handed_over(*ec.match_stats(orc.find_kmer_matches, p.x, p.y, k)) for p in pairs)


def test_constants_equal_the_sources():
    with open(os.path.join(CSRC, "band_device.h")) as f:
        hdr = f.read()
    with open(os.path.join(CSRC, "band_device.hip")) as f:
        src = f.read()

    def one(pattern, text):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return int(found[0])

    assert one(r"constexpr uint32_t kMaxChainMatches = (\d+);", hdr) == ec.MAX_CHAIN_MATCHES == 4095
    assert one(r"constexpr uint32_t kSmallChainMatches = (\d+);", hdr) == ec.SMALL_CHAIN_MATCHES == 2047
    assert one(r"constexpr uint32_t kMaxMatchesPerKmer = (\d+);", hdr) == ec.MAX_MATCHES_PER_KMER == 32
    assert one(r"constexpr uint32_t kChainGlobalMinPairs = (\d+);", hdr) == ec.CHAIN_GLOBAL_MIN_PAIRS == 1024
    assert one(r"#define BG_BAND_TILE (\d+)", src) == ec.BAND_TILE == 2048
    assert one(r"constexpr uint32_t kStageMaxBytes = (\d+);", src) == ec.STAGE_MAX_BYTES == 40960
    assert one(r"lds_bytes <= (\d+) \* 1024 &&", src) * 1024 == ec.LDS_JOIN_MAX_BYTES == 150 * 1024
    assert one(r"constexpr uint32_t kLdsJoinTable = (\d+);", src) == ec.LDS_JOIN_TABLE == 8192
    # both joins test the caps the way handed_over() does: more than, not at least
    assert len(re.findall(r"> kMaxChainMatches\b", src)) == 2 and len(re.findall(r"> kMaxMatchesPerKmer\b", src)) == 2


def test_generators_are_deterministic(short):
    again = ec.short_batch()
    assert [(p.name, p.kind, p.x, p.y) for p in again] == [(p.name, p.kind, p.x, p.y) for p in short]
    assert ec.long_pair(20465).x == ec.long_pair(20465).x
    a, b = ec.many_small_pairs(1023), ec.many_small_pairs(1024)
    assert [(p.x, p.y) for p in a] == [(p.x, p.y) for p in b[:1023]]
    assert all(60 <= len(p.y) <= 120 and len(p.x) == len(p.y) for p in b)


def test_match_count_family(stats):
    for c in ec.MATCH_COUNTS:
        p = ec.match_count_pair(c)
        assert len(p.x) == c + ec.K - 1 and p.x == p.y
        assert ec.match_stats(orc.find_kmer_matches, p.x, p.y) == (c, 1), c
        assert ec.handed_over(c, 1) == (c == 4096)
    assert [stats[f"matches{c}.0"] for c in (1, 2047, 2048)] == [(1, 1), (2047, 1), (2048, 1)]


def test_per_kmer_family():
    for r in ec.PER_KMER_COPIES:
        p = ec.per_kmer_pair(r)
        total, per_x = ec.match_stats(orc.find_kmer_matches, p.x, p.y)
        assert per_x == r and total < 1000, (r, total, per_x)  # the list of one position decides, not the total
        assert len(p.x) == 300 + ec.K + 300 and ec.handed_over(total, per_x) == (r == 33)
        # exactly one x position carries the long list
        mm = orc.find_kmer_matches(p.x, p.y, ec.K)
        assert sorted(np.bincount(mm[:, 0].astype(np.int64)))[-2] == 1


def test_every_pair_of_the_short_batch_is_of_its_kind(short, stats):
    assert len(short) == 129 and len({p.name for p in short}) == 129
    for p in short:
        total, per_x = stats[p.name]
        if p.kind == "zero":
            assert total == 0, p
        elif p.kind == "full":
            assert (total, per_x) == (4095, 1), p
        elif p.kind == "handed":
            assert (total, per_x) == (4096, 1) or (per_x == 33 and total < 1000), (p, total, per_x)
        else:
            assert 0 < total <= 4095 and per_x <= 32, (p, total, per_x)
        assert ec.handed_over(total, per_x) == (p.kind == "handed"), p
    assert sum(p.kind == "handed" for p in short) == ec.N_QUADS + ec.HANDED_RUN == expected_handed_over(short)


def test_no_match_family_and_its_residues(short):
    zero = [p for p in short if p.kind == "zero"]
    shapes = {(len(p.x), len(p.y)) for p in zero}
    assert shapes == {(m, n) for m in ec.NO_MATCH_M for n in ec.NO_MATCH_N} | {(300, 300)}
    assert sum(len(p.x) == 300 for p in zero) == 2
    assert any(len(p.x) < ec.K for p in zero) and any(len(p.y) < ec.K for p in zero)
    starts = ec.zero_match_starts(short)
    assert len(starts) == len(zero) == 26
    assert {s[0] for s in starts} == set(range(16)) and {s[1] for s in starts} == set(range(16))
    # a long pair goes behind the short batch: the starts stay
    assert ec.zero_match_starts(short + [ec.long_pair(20128)]) == starts


def test_raster_tile_family(short, stats):
    tiles = [p for p in short if p.kind == "tile"]
    assert sorted(len(p.y) for p in tiles) == sorted(2 * list(ec.TILE_N))
    for p in tiles:
        n = len(p.y)
        mm = orc.find_kmer_matches(p.x, p.y, ec.K).astype(np.int64)
        if p.x == p.y:
            assert stats[p.name] == (n - ec.K + 1, 1)  # one diagonal: one anchor, n - k continuations
        else:
            assert len(p.x) < n and 300 < len(mm) < 1000
            assert len(set((mm[:, 0] - mm[:, 1]).tolist())) >= n // 160  # a new diagonal behind every deleted base
        for col in (ec.BAND_TILE, 2 * ec.BAND_TILE):  # a match covers the first column of the second / third tile
            if n >= col:
                assert ((mm[:, 1] <= col) & (col <= mm[:, 1] + ec.K)).any(), (p, col)
        assert (mm[:, 1] + ec.K == n).any()  # and the last column


def test_long_pairs_and_the_join_each_selects(short, longs, stats):
    assert ec.lds_join_bytes(20128, 20128) == 153600 == ec.LDS_JOIN_MAX_BYTES
    assert ec.lds_join_bytes(20129, 20129) > ec.LDS_JOIN_MAX_BYTES
    assert ec.stage_bytes(20464, 20464) == 40944 <= ec.STAGE_MAX_BYTES < ec.stage_bytes(20465, 20465) == 40961
    longest = max(max(len(p.x), len(p.y)) for p in short)
    assert ec.join_flavour(longest, longest) == "lds" and ec.join_flavour(longest, longest, True) == "staged"
    for p in longs:
        length = len(p.x)
        assert len(p.y) == length > longest
        assert ec.join_flavour(length, length) == ec.LONG_FLAVOUR[length]
        total, per_x = stats[p.name]
        # (the large LDS size class of the chaining, and never handed over)
        assert ec.SMALL_CHAIN_MATCHES < total <= ec.MAX_CHAIN_MATCHES and per_x <= 2, (p, total, per_x)
    assert [ec.LONG_FLAVOUR[length] for length in ec.LONG_L] == ["lds", "staged", "staged", "unstaged"]


def test_order_of_the_short_batch(short):
    kinds = [p.kind for p in short]
    for i in range(4 * ec.N_QUADS - 3):  # every run of four: a zero-match, a handed-over, a 4095 and a small pair
        assert sorted(kinds[i:i + 4]) == ["full", "handed", "small", "zero"], i
    assert len(short) % 4 == 1 and (len(short) + 1) % 4 == 2 and (ec.CHAIN_GLOBAL_MIN_PAIRS - 1) % 4 == 3
    for chunk in (4, 5):
        subs = ec.sub_batches(len(short), chunk)
        assert sum(w for _, w in subs) == len(short) and all(0 < w <= chunk for _, w in subs)
        handed = [sum(k == "handed" for k in kinds[p0:p0 + w]) for p0, w in subs]
        assert any(h == w == chunk for h, (_, w) in zip(handed, subs)), chunk  # only handed-over pairs
        assert any(h == 0 and w == chunk for h, (_, w) in zip(handed, subs)), chunk  # none
    assert ec.sub_batches(129, 4)[0] == (0, 1) and ec.sub_batches(129, 5)[0] == (0, 4)  # the remainder goes first


def test_k8_run_has_both_outcomes(short):
    """with k = 8 the same pairs fall on either side of the caps for other reasons (random 8-mers repeat)"""
    flags = [ec.handed_over(*ec.match_stats(orc.find_kmer_matches, p.x, p.y, 8)) for p in short]
    assert 0 < sum(flags) < len(short)
    assert any(ec.match_stats(orc.find_kmer_matches, p.x, p.y, 8)[0] == 0 for p in short)


def check_host_builder(pairs, k, w):
    """bg_band_create_batch (band_host.cpp) against the oracle's Band::create, semiglobal clipping"""
    al = Aligner.with_scoring(Scoring.from_scores(-5, -1, 1, -1), k, w, ctx=False)
    x, xo = _lib.concat([p.x for p in pairs])
    y, yo = _lib.concat([p.y for p in pairs])
    boff, st, en, cells = al.band_create_arrays(2, x, xo, y, yo)
    osc = orc.make_scoring(-5, -1, 1, -1, xclip_prefix=MIN_SCORE, xclip_suffix=MIN_SCORE, yclip_prefix=0, yclip_suffix=0)
    for i, p in enumerate(pairs):
        ost, oen, ocells = orc.band_create(osc, k, w, p.x, p.y)
        lo, hi = int(boff[i]), int(boff[i + 1])
        assert (st[lo:hi] == ost).all() and (en[lo:hi] == oen).all() and int(cells[i]) == ocells, (p, k, w)
        if ec.match_stats(orc.find_kmer_matches, p.x, p.y, k)[0] == 0:  # banded.rs:1309-1313: the full matrix
            assert (ost == 0).all() and (oen == len(p.x) + 1).all() and ocells == (len(p.x) + 1) * (len(p.y) + 1)


def test_host_builder_equals_oracle_on_the_short_batch(short):
    check_host_builder(short, ec.K, ec.W)


def test_host_builder_equals_oracle_on_the_short_batch_k8(short):
    check_host_builder(short, 8, 6)


def test_host_builder_equals_oracle_on_the_long_pairs(longs):
    check_host_builder(longs, ec.K, ec.W)


def test_host_builder_equals_oracle_on_many_small_pairs():
    check_host_builder(ec.many_small_pairs(ec.CHAIN_GLOBAL_MIN_PAIRS), ec.K, ec.W)
