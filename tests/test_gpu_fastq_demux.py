"""`bg_fastq_demux_assign[_dev]` and `bg_fastq_demux_split[_dev]` (csrc/fastq_demux.hip) byte for byte against the two rules
as a few lines of Python (tests/fastq_demux_oracle.py; include/biogpu.h defines them): the device flavour with and without
its optional outputs and the host flavour.  Assign: the margin at its edge, ties, ignored patterns, the anchors at their edge,
pattern counts at the edges of the lane group and at the cap with the winner at the group's edges, 1 and 1024 bins, the pair
rule, scores of the long call's range.  Split: record counts around the tile and the scan's block (both 2048), one group, a
group per record, empty groups, bin values above n_bins + 1, empty records, stability, perm, determinism, source alignments."""
import random

import numpy as np
import pytest
import torch

import fastq_demux_oracle as dm
from fastq_demux_cases import LEGAL_FLAGS, blank_hits, random_hits, random_pat_bin, set_hit
from fastq_write_cases import Batch, random_records
from rust_bio_amd import _lib, fastq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 2048  # the split's tile and the scan's block
X = None


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(DEV)


def u32(t, n):
    return t.cpu().numpy().view(np.uint32)[:n]


def assign_checked(hits, n_pat, pat_bin, n_bins, **prm):
    """the device flavour with and without pat_out and the host flavour against the rule; returns the rule's (bin, hit_out, pat_out)"""
    n = len(hits) // n_pat
    want = dm.assign(hits, n_pat, pat_bin, n_bins, **prm)
    stream = torch.cuda.current_stream().cuda_stream
    d_hits = up(hits)
    for want_pat in (True, False):
        d_bin, d_hit, d_pat = fastq.demux_assign_dev(n, d_hits, n_pat, pat_bin, n_bins, stream=stream, want_pat=want_pat, **prm)
        torch.cuda.synchronize()
        assert (u32(d_bin, n) == want[0]).all(), np.flatnonzero(u32(d_bin, n) != want[0])[:8]
        assert d_hit.cpu().numpy().tobytes() == want[1].tobytes()
        assert (d_pat is None) if not want_pat else (u32(d_pat, n) == want[2]).all()
    h_bin, h_hit, h_pat = fastq.demux_assign_arrays(hits, n_pat, pat_bin, n_bins, **prm)
    assert (h_bin == want[0]).all() and h_hit.tobytes() == want[1].tobytes() and (h_pat == want[2]).all()
    assert fastq.demux_assign_arrays(hits, n_pat, pat_bin, n_bins, want_pat=False, **prm)[2] is None
    return want


def rows(table, n_pat=None, ylen=30):
    """hit records of a table: a row holds per pattern None, a score, or (score, ystart, yend); padded to n_pat patterns"""
    n_pat = n_pat or len(table[0])
    hits = blank_hits(len(table), n_pat, ylen)
    for r, row in enumerate(table):
        for p, h in enumerate(row):
            if h is not None:
                set_hit(hits, n_pat, r, p, *(h if isinstance(h, tuple) else (h,)))
    return hits


@pytest.mark.parametrize("n_pat", [3, 19])  # one lane and sixteen lanes per read
def test_margin_ties_and_ignored_patterns(n_pat):
    pat_bin = np.array([0, 1, 1] + [dm.IGNORE] * (n_pat - 3), dtype=np.uint32)
    table = [[0, 2, X], [0, 1, X], [0, 3, X],   # second - best equal to min_margin = 2, one below, one above
             [1, 1, X], [X, 1, 1], [2, X, 2],   # ties: between two bins, inside one bin, between two bins
             [X, X, X], [5, 4, 4]]
    hits = rows(table, n_pat)
    assert list(assign_checked(hits, n_pat, pat_bin, 2, min_margin=2)[0]) == [0, 3, 0, 3, 1, 3, 2, 3]
    b, _, p = assign_checked(hits, n_pat, pat_bin, 2, min_margin=0)  # a tie between bins goes to the lower pattern
    assert list(b) == [0, 0, 0, 0, 1, 0, 2, 1] and list(p) == [0, 0, 0, 0, 1, 0, dm.IGNORE, 1]
    # only ignored patterns hit; with them ignored nothing is ambiguous either
    only = np.array([dm.IGNORE] * n_pat, dtype=np.uint32)
    b, h, p = assign_checked(hits, n_pat, only, 2, min_margin=1)
    assert (b == 2).all() and (p == dm.IGNORE).all() and (h["score"] == dm.MIN_SCORE).all() and (h["ylen"] == 30).all() and (h["mode"] == 2).all()
    half = np.array([0, dm.IGNORE, dm.IGNORE] + [dm.IGNORE] * (n_pat - 3), dtype=np.uint32)
    assert list(assign_checked(hits, n_pat, half, 2, min_margin=2)[0]) == [0, 0, 0, 0, 2, 0, 2, 0]
    # no hits at all
    b, h, _ = assign_checked(blank_hits(5, n_pat, ylen=77), n_pat, pat_bin, 2, min_margin=1)
    assert (b == 2).all() and (h["ylen"] == 77).all() and (h["xlen"] == 0).all()


def test_anchors_at_their_edge():
    # ylen 30, max_offset 3: ystart 3 / 4 under ANCHOR_5P, ylen - yend 3 / 4 under ANCHOR_3P
    hits = rows([[(0, 3, 11)], [(0, 4, 12)], [(0, 19, 27)], [(0, 18, 26)], [(0, 0, 30)], [X]])
    assert list(assign_checked(hits, 1, [0], 1, flags=dm.ANCHOR_5P, max_offset=3)[0]) == [0, 1, 1, 1, 0, 1]
    assert list(assign_checked(hits, 1, [0], 1, flags=dm.ANCHOR_3P, max_offset=3)[0]) == [1, 1, 0, 1, 0, 1]
    assert list(assign_checked(hits, 1, [0], 1, flags=dm.ANCHOR_5P, max_offset=0)[0]) == [1, 1, 1, 1, 0, 1]
    assert list(assign_checked(hits, 1, [0], 1, max_offset=0)[0]) == [0, 0, 0, 0, 0, 1]  # no anchor: anywhere
    # the better hit is out of reach: the anchored one wins
    two = rows([[(0, 9, 17), (1, 0, 8)]])
    assert list(assign_checked(two, 2, [0, 1], 2, flags=dm.ANCHOR_5P, max_offset=2, min_margin=1)[2]) == [1]
    assert list(assign_checked(two, 2, [0, 1], 2, min_margin=1)[2]) == [0]


@pytest.mark.parametrize("n_pat", [1, 15, 16, 17, 1024])
def test_pattern_counts_at_the_group_edges_and_the_cap(n_pat):
    """the winner at pattern 0, 15, 16 and n_pat - 1, alone and among worse hits of other bins; 1 bin, a few, and 1024"""
    rng = random.Random(n_pat)
    spots = sorted({p for p in (0, 15, 16, n_pat - 1) if p < n_pat})
    for n_bins in sorted({1, min(5, n_pat), n_pat}):
        pat_bin = np.arange(n_pat, dtype=np.uint32) % n_bins
        hits = blank_hits(3 * len(spots), n_pat)
        for i, w in enumerate(spots):
            set_hit(hits, n_pat, 3 * i, w, 1)                       # alone
            set_hit(hits, n_pat, 3 * i + 1, w, 1)                   # a runner-up two away: assigned at min_margin 2
            set_hit(hits, n_pat, 3 * i + 2, w, 1)                   # ... and one away: ambiguous if it is in another bin
            for r, s in ((3 * i + 1, 3), (3 * i + 2, 2)):
                for p in rng.sample(range(n_pat), min(n_pat, 6)):
                    if p != w:
                        set_hit(hits, n_pat, r, p, s + rng.randint(0, 1) * (p % 2))
        b, h, p = assign_checked(hits, n_pat, pat_bin, n_bins, min_margin=2)
        assert list(p[0::3]) == spots and list(p[1::3]) == spots and list(b[0::3]) == [w % n_bins for w in spots]
        if n_bins == n_pat and n_pat > 1:
            assert (b[2::3] == n_bins + 1).all()


@pytest.mark.parametrize("n_pat", [2, 17])
def test_pair_rule(n_pat):
    # pattern p -> bin p; winner on mate 1 only, on mate 2 only, on both with equal (score, p), a better one on mate 2, nothing
    table = [[0, X], [X, X],   [X, X], [X, 1],   [1, X], [1, X],   [X, X], [0, X],   [2, X], [X, 0],   [X, X], [X, X]]
    hits = rows(table, n_pat)
    pat_bin = np.array([0, 1] + [dm.IGNORE] * (n_pat - 2), dtype=np.uint32)
    b, h, p = assign_checked(hits, n_pat, pat_bin, 2, flags=dm.PAIRED)
    assert list(b) == [0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 2, 2]
    assert list(p) == [0, dm.IGNORE, dm.IGNORE, 1, 0, dm.IGNORE, dm.IGNORE, 0, dm.IGNORE, 1, dm.IGNORE, dm.IGNORE]
    assert h[4].tobytes() == hits[4 * n_pat].tobytes() and int(h[5]["score"]) == dm.MIN_SCORE
    # MATE1 / MATE2 exclude the only hit
    assert list(assign_checked(hits, n_pat, pat_bin, 2, flags=dm.PAIRED | dm.MATE1)[0]) == [0, 0, 2, 2, 0, 0, 2, 2, 0, 0, 2, 2]
    assert list(assign_checked(hits, n_pat, pat_bin, 2, flags=dm.PAIRED | dm.MATE2)[0]) == [2, 2, 1, 1, 0, 0, 0, 0, 1, 1, 2, 2]
    assert list(assign_checked(hits, n_pat, pat_bin, 2, flags=dm.PAIRED | dm.MATE1 | dm.MATE2)[0]) == list(b)
    # the runner-up on the other mate: margin 2 between the mates' hits
    assert list(assign_checked(hits, n_pat, pat_bin, 2, flags=dm.PAIRED, min_margin=2)[0]) == [0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 2, 2]
    assert list(assign_checked(hits, n_pat, pat_bin, 2, flags=dm.PAIRED, min_margin=3)[0]) == [0, 0, 1, 1, 0, 0, 0, 0, 3, 3, 2, 2]
    assert list(assign_checked(hits, n_pat, pat_bin, 2, min_margin=3)[0]) == [0, 2, 2, 1, 0, 0, 2, 0, 0, 1, 2, 2]


def test_scores_of_the_long_call():
    hits = rows([[300, 301, X], [300, 302, X], [1000, X, 256], [70000, 70000, 69999]])
    b, h, p = assign_checked(hits, 3, [0, 1, 2], 3, min_margin=2)
    assert list(b) == [4, 0, 2, 4] and list(p) == [dm.IGNORE, 0, 2, dm.IGNORE]
    assert list(assign_checked(hits, 3, [0, 1, 2], 3, min_margin=0)[2]) == [0, 0, 2, 2]
    neg = rows([[-5, -3, X]])  # any score but BG_MIN_SCORE is a hit
    assert list(assign_checked(neg, 3, [0, 1, 2], 3, min_margin=2)[0]) == [0]


@pytest.mark.parametrize("n_pat, n_bins", [(3, 2), (40, 5), (96, 96)])
def test_random_batches_over_every_legal_flag_combination(n_pat, n_bins):
    rng = random.Random(n_pat)
    seen = set()
    for flags in LEGAL_FLAGS:
        n = 2 * rng.randint(130, 400)  # several blocks at either group width
        hits = random_hits(rng, n, n_pat, p_hit=min(0.5, 1.5 / n_pat))
        b = assign_checked(hits, n_pat, random_pat_bin(rng, n_pat, n_bins), n_bins, flags=flags, min_margin=rng.choice([0, 1, 2]),
                           max_offset=rng.choice([0, 2, 3]))[0]
        seen |= {"assigned" if x < n_bins else "unassigned" if x == n_bins else "ambiguous" for x in b}
    assert seen == {"assigned", "unassigned", "ambiguous"}


# ---- split ----------------------------------------------------------------------------------------------------------------
def same_split(got, want, n):
    recs, seq, so, qual, qo, hit, perm, boff = got
    w_recs, w_seq, w_so, w_qual, w_qo, w_hit, w_perm, w_boff = want
    assert (np.asarray(boff, dtype=np.uint64) == w_boff).all(), (boff, w_boff)
    if perm is not None:
        assert (np.asarray(perm[:n], dtype=np.uint64) == w_perm).all()
    assert recs[:n].tobytes() == w_recs.tobytes()
    assert (np.asarray(so[:n + 1], dtype=np.uint64) == w_so).all() and (np.asarray(qo[:n + 1], dtype=np.uint64) == w_qo).all()
    assert bytes(seq[:len(w_seq)]) == w_seq and bytes(qual[:len(w_qual)]) == w_qual
    if hit is not None:
        assert hit[:n].tobytes() == w_hit.tobytes()


def host(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def split_checked(batch, bins, n_bins, hit=None):
    """the device flavour with every optional output (twice: the same bytes), without any, and the host flavour, against the rule"""
    n = len(batch)
    bins = np.asarray(bins, dtype=np.uint32)
    want = dm.split(bins, n_bins, *batch.columns(), hit=hit)
    _, d_recs, d_seq, d_so, d_qual, d_qo = batch.to_dev(DEV)
    d_bin = up(bins) if n else torch.zeros(4, dtype=torch.uint8, device=DEV)
    hit = hit if n else None  # no record: no tensor to point at
    d_hit = up(hit) if hit is not None else None
    stream = torch.cuda.current_stream().cuda_stream
    first = None
    for _ in range(2):
        res = fastq.demux_split_dev(n, d_bin, n_bins, d_recs, d_seq, d_so, d_qual, d_qo, d_hit=d_hit, stream=stream, want_perm=True)
        o_recs, o_seq, o_so, o_qual, o_qo, o_hit, d_perm, d_boff, boff = res
        assert (host(d_boff).view(np.uint64) == boff).all()
        got = (host(o_recs, _lib.FQREC_DTYPE), host(o_seq)[:len(want[1])], host(o_so), host(o_qual)[:len(want[3])], host(o_qo),
               host(o_hit, _lib.ALN_DTYPE) if o_hit is not None else None, host(d_perm), boff)
        same_split(got, want, n)
        again = [x.tobytes() for x in got if x is not None]
        assert first is None or again == first  # the same call twice gives the same bytes
        first = again
    # nothing optional: no hit, no perm, no host offsets — the call does not wait
    res = fastq.demux_split_dev(n, d_bin, n_bins, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream, want_bin_off=False)
    torch.cuda.synchronize()
    assert res[5] is None and res[6] is None and res[8] is None
    same_split((host(res[0], _lib.FQREC_DTYPE), host(res[1]), host(res[2]), host(res[3]), host(res[4]), None, None, host(res[7]).view(np.uint64)),
               want, n)
    same_split(fastq.demux_split_arrays(bins, n_bins, *batch.columns(), hit=hit), want, n)
    return want


def ids_of(batch, recs):
    return [batch.text[int(c["id_off"]):int(c["id_off"] + c["id_len"])] for c in recs]


@pytest.mark.parametrize("n", [0, 1, T - 1, T, T + 1, 2 * T + 1])
def test_counts_around_the_tile_and_the_scan_block(n):
    rng = random.Random(n)
    b = Batch(random_records(rng, n, 0, 8), a_seq=n % 16, a_qual=(n * 7 + 5) % 16)  # empty records, unequal lengths, every alignment
    n_bins = 3
    bins = [rng.choice([0, 1, 2, 3, 4, 4, n_bins + 2, 0xFFFFFFFF]) for _ in range(n)]  # the last two are unassigned
    hit = random_hits(rng, n, 1, p_hit=0.6)
    want = split_checked(b, bins, n_bins, hit)
    recs, perm, boff = want[0], want[6], want[7]
    assert sorted(perm.tolist()) == list(range(n)) and int(boff[-1]) == n
    group = [min(x, n_bins) if x > n_bins + 1 else x for x in bins]
    for g in range(n_bins + 2):  # ids in input order inside every group
        lo, hi = int(boff[g]), int(boff[g + 1])
        assert ids_of(b, recs[lo:hi]) == [rec[0] for rec, x in zip(b.records, group) if x == g]
    if n > 1:
        assert boff[n_bins + 1] - boff[n_bins] > sum(x == n_bins for x in bins)  # the out-of-range values went to unassigned


def test_one_group_empty_groups_and_a_group_per_record():
    rng = random.Random(9)
    b = Batch(random_records(rng, 300, 0, 30), a_seq=3, a_qual=11)
    hit = random_hits(rng, 300, 1, p_hit=0.5)
    for g in (0, 4, 5, 6):  # everything in one group: the first sample, the last, unassigned, ambiguous
        want = split_checked(b, [g] * 300, 5, hit)
        assert list(want[6]) == list(range(300)) and want[1] == b.seq[3:] and want[3] == b.qual[11:]
        assert list(want[7]) == [0] * (g + 1) + [300] * (7 - g)
    # empty groups at the start, in the middle and at the end
    bins = [rng.choice([2, 3, 6, 7]) for _ in range(300)]
    boff = split_checked(b, bins, 8, hit)[7]
    assert boff[2] == 0 and boff[4] == boff[6] and boff[8] == boff[10] == 300 and 0 < boff[3] < boff[4] < boff[7] < 300
    # 1026 records, each in its own group, n_bins 1024: in reversed order, so that every record moves
    b = Batch(random_records(rng, 1026, 0, 6))
    bins = list(range(1025, -1, -1))
    want = split_checked(b, bins, 1024, random_hits(rng, 1026, 1, p_hit=0.5))
    assert list(want[6]) == list(range(1025, -1, -1)) and list(want[7]) == list(range(1027))
    # ... and all of them, and many per group, over several tiles
    b = Batch(random_records(rng, 2 * T + 77, 0, 4))
    split_checked(b, [rng.randrange(1026) for _ in range(2 * T + 77)], 1024)
    split_checked(b, [rng.choice([0, 1023, 1024, 1025]) for _ in range(2 * T + 77)], 1024)
    split_checked(b, [rng.randrange(3) for _ in range(2 * T + 77)], 1)


def test_records_trimmed_to_nothing_and_pairs_stay_adjacent():
    rng = random.Random(4)
    recs = [(b"p%d" % (i // 2), b"%d" % (i % 2 + 1), b"" if i % 5 == 0 else b"ACGTN"[:1 + i % 5], b"" if i % 5 == 0 else b"IIIII"[:1 + i % 5])
            for i in range(200)]
    b = Batch(recs)
    pair_bin = [rng.randrange(6) for _ in range(100)]
    want = split_checked(b, [pair_bin[i // 2] for i in range(200)], 4)
    ids = ids_of(b, want[0])
    assert ids[0::2] == ids[1::2] and all(int(x) % 2 == 0 for x in want[7])
    assert sum(int(c["seq_len"]) == 0 for c in want[0]) == 40
    # all records empty
    e = Batch([(b"e%d" % i, None, b"", b"") for i in range(50)])
    w = split_checked(e, [i % 3 for i in range(50)], 2)
    assert list(w[2]) == [0] * 51 and w[1] == b""


def test_sources_behind_prefixes():
    rng = random.Random(16)
    for a in range(16):
        b = Batch(random_records(rng, 60, 0, 70), a_seq=a, a_qual=(a * 5 + 3) % 16)
        split_checked(b, [rng.randrange(5) for _ in range(60)], 3, random_hits(rng, 60, 1))
