"""bg_sam_markdup[_dev] against the CPU statement of its rule (tests/sam_sort_oracle.py): the duplicate byte of every read and the
four counts, single-end and paired, host and device flavours.  The batches are synthetic hit records (tests/sam_sort_cases.py),
shaped so that runs of equal keys have the sizes at which a pass over runs can go wrong — 1, 2, and around the width of a
wavefront and of a block — that one run spans several blocks, that every score ties, that coordinates differ only above bit 32,
and that secondary slots sit on a winner's coordinate."""
import random

import numpy as np
import pytest
import torch

import sam_oracle as so
import sam_sort_oracle as sso
from rust_bio_amd import _lib, sam
from sam_sort_cases import BIG_CONTIGS, CONTIGS, MIN_QUAL, PHRED, arrays, make_hit, random_batch, read_of, runs_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RUNS = (1, 2, 63, 64, 65, 255, 256, 257)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def check(fq, hits, strand, flags=0, K=1, contigs=CONTIGS, min_qual=MIN_QUAL):
    """both flavours against the oracle; returns the oracle's (dup, counts)"""
    want, counts = sso.markdup(contigs, fq, hits, strand, flags, K, PHRED, min_qual)
    table = sam.Contigs(contigs)
    mp = sam.MarkdupParams(flags, K, PHRED, min_qual)
    got, got_counts = sam.markdup_arrays(mp, table, fq, hits, strand)
    assert got_counts == counts and got.tobytes() == want.tobytes()
    n = len(fq.recs)
    d = [dev(x) for x in (table.table, hits, strand, fq.recs, fq.qual if len(fq.qual) else np.zeros(1, np.uint8))]
    d_dup = torch.full((n + 16,), 0x7e, dtype=torch.uint8, device=DEV)
    got_counts = sam.markdup_dev(mp, n, d[0].data_ptr(), len(table), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                 d_dup.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    out = d_dup.cpu().numpy()
    assert got_counts == counts and out[:n].tobytes() == want.tobytes() and (out[n:] == 0x7e).all()
    return want, counts


@pytest.mark.parametrize("paired", [False, True])
def test_runs_of_every_size(paired):
    fq, hits, strand = runs_batch(RUNS, paired=paired)
    dup, counts = check(fq, hits, strand, so.PAIRED if paired else 0)
    losers = sum(RUNS) - len(RUNS)
    assert counts == ([2 * sum(RUNS), 2 * losers, losers, 0] if paired else [sum(RUNS), losers, 0, 0])


@pytest.mark.parametrize("paired", [False, True])
def test_one_run_holds_the_whole_batch(paired):
    fq, hits, strand = runs_batch((1500 if paired else 3000,), paired=paired, seed=5)
    dup, counts = check(fq, hits, strand, so.PAIRED if paired else 0)
    assert counts[:2] == [3000, 2998 if paired else 2999]


@pytest.mark.parametrize("paired", [False, True])
def test_all_scores_equal(paired):
    fq, hits, strand = runs_batch((5, 70, 1, 300, 2), paired=paired, equal_scores=True, seed=7)
    dup, counts = check(fq, hits, strand, so.PAIRED if paired else 0)
    # the smallest index of every group stays: the first member met in index order
    step = 2 if paired else 1
    seen, want = set(), []
    for r in range(0, len(dup), step):
        want.append(int(hits["ref_start"][r]) in seen)
        seen.add(int(hits["ref_start"][r]))
    assert [bool(x) for x in dup[::step]] == want


def test_coordinates_above_2_32():
    lo, hi, far = (c[1] for c in BIG_CONTIGS)
    at = [lo + 100, hi + 100, hi + 100, far + 9, far + 9, lo + 100, far + 9 + 2**32 - 2**32, hi + 100 - 2**32 + 2**32]
    assert hi + 100 - (lo + 100) == 2**32  # differ only above bit 32
    reads = [read_of(r, 24, 20) for r in range(len(at))]
    fq, hits, strand = arrays(reads, [make_hit(40, 0, a, a + 24, 0, 24, 24) for a in at])
    dup, counts = check(fq, hits, strand, contigs=BIG_CONTIGS)
    assert dup.tolist() == [0, 0, 1, 0, 1, 1, 1, 1] and counts == [8, 5, 0, 0]
    # pairs whose hi ends differ only above bit 32
    pairs = [(lo + 100, lo + 400), (lo + 100, lo + 400), (hi + 100, hi + 400), (hi + 100, hi + 400), (far + 100, far + 400)]
    reads = [read_of(r, 24, 20, True) for r in range(2 * len(pairs))]
    hl = [h for a, b in pairs for h in (make_hit(40, 0, a, a + 24, 0, 24, 24), make_hit(40, 1, b - 24, b, 0, 24, 24))]
    fq, hits, strand = arrays(reads, hl)
    dup, counts = check(fq, hits, strand, so.PAIRED, contigs=BIG_CONTIGS)
    assert dup.tolist() == [0, 0, 1, 1, 0, 0, 1, 1, 0, 0] and counts == [10, 4, 2, 0]


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_batches(n):
    for paired in (False, True):
        if paired and n % 2:
            continue
        reads = [read_of(r, 24, 20 + r, paired) for r in range(n)]
        fq, hits, strand = arrays(reads, [make_hit(40, 0, 100, 124, 0, 24, 24)] * n)
        dup, counts = check(fq, hits, strand, so.PAIRED if paired else 0)
        assert dup.tolist() == ([0, 1][::-1] if n == 2 and not paired else [0] * n)


def test_secondary_slots_take_no_part():
    """K = 4: the secondary slots of every read sit on read 0's coordinate"""
    at = [100, 300, 500, 100, 700, 300]
    reads = [read_of(r, 24, 30 - r) for r in range(len(at))]
    hl = []
    for a in at:
        hl += [make_hit(40, 0, a, a + 24, 0, 24, 24)] + [make_hit(30, 0, 100, 124, 0, 24, 24)] * 3
    fq, hits, strand = arrays(reads, hl)
    dup, counts = check(fq, hits, strand, 0, K=4)
    assert dup.tolist() == [0, 0, 0, 1, 0, 1] and counts == [6, 2, 0, 0]


@pytest.mark.parametrize("paired,K", [(False, 1), (True, 1), (False, 4)])
def test_random_batches(paired, K):
    rng = random.Random(11 + K + paired)
    seen = {}
    for rnd in range(3):
        fq, hits, strand = random_batch(rng, 700, K=K, paired=paired, p_unmapped=(0.2, 0.5, 0.1)[rnd])
        check(fq, hits, strand, so.PAIRED if paired else 0, K)
        check(fq, hits, strand, so.PAIRED if paired else 0, K, min_qual=0)
        sso.markdup(CONTIGS, fq, hits, strand, so.PAIRED if paired else 0, K, PHRED, MIN_QUAL, events=seen)
    assert seen["group won on index"] >= 10 and seen["group won on score"] >= 20 and seen["unplaced"] >= 50, seen
    if paired:
        assert seen["pair group"] >= 20 and seen["fragment flagged by a pair"] >= 10 and seen["fragment group"] >= 5, seen
