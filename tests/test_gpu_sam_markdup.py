"""bg_sam_markdup[_dev] against the CPU statement of its rule (tests/sam_sort_oracle.py): the duplicate byte of every read and the
four counts, single-end and paired, host and device flavours.  The batches are synthetic hit records (tests/sam_sort_cases.py),
shaped so that runs of equal keys have the sizes at which a pass over runs can go wrong — 1, 2, and around the width of a
wavefront and of a block — that one run spans several blocks, that every score ties, that coordinates differ only above bit 32,
and that secondary slots sit on a winner's coordinate."""
import random

import numpy as np
import pytest
import torch

import sam_edge_cases as ec
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


# ---- the lanes of the score kernel, batch shapes, and the chain without pairs (tests/sam_edge_cases.py) ---------------------
@pytest.mark.parametrize("min_qual", ec.MIN_QUALS)
def test_quality_lengths_around_the_lanes_of_a_read(min_qual):
    fq, hits, strand = ec.qual_lengths()
    assert tuple(int(r["qual_len"]) for r in fq.recs[::3]) == ec.QUAL_LENGTHS
    dup, counts = check(fq, hits, strand, min_qual=min_qual)
    assert dup.tolist() == [0, 1, 1] + [1, 1, 0] * (len(ec.QUAL_LENGTHS) - 1)  # the last quality byte decides every group


@pytest.mark.parametrize("n", [15, 16, 17, 255, 256, 257])
def test_batch_sizes_around_a_block(n):
    fq, hits, strand = random_batch(random.Random(50 + n), n, n_coords=4)
    dup, counts = check(fq, hits, strand)
    assert n < 255 or counts[1] >= 50
    if n % 2 == 0:
        fq, hits, strand = random_batch(random.Random(60 + n), n, paired=True, n_coords=4)
        check(fq, hits, strand, so.PAIRED)


def test_nothing_is_placed():
    for paired in (False, True):
        fq, hits, strand = random_batch(random.Random(71), 300, paired=paired, p_unmapped=1.0)
        dup, counts = check(fq, hits, strand, so.PAIRED if paired else 0)
        assert counts == [0, 0, 0, 0] and not dup.any()


def test_fragments_only():
    fq, hits, strand = ec.fragments_only()
    dup, counts = check(fq, hits, strand, so.PAIRED)
    assert counts[0] == len(fq.recs) // 2 and counts[1] >= 20 and counts[2:] == [0, 0]


@pytest.mark.parametrize("K,flags", [(1, 0), (4, so.SECONDARY)])
def test_the_chain_without_pairs(K, flags):
    """markdup -> emit with dup -> keys -> sort on a synthetic unpaired batch: `sam.sorted_sam`, and the four device calls chained
    in HBM, against the composition of the four oracles under an SO:coordinate header"""
    from test_gpu_sam_emit_edges import index
    fm = index()
    n = 600
    fq, hits, strand = random_batch(random.Random(80 + K), n, K=K, p_unmapped=0.3)
    flags |= so.TAG_NM
    ops = np.zeros(0, dtype=np.uint8)
    dup, counts = sso.markdup(CONTIGS, fq, hits, strand, 0, K, PHRED, MIN_QUAL)
    plain = so.lines(CONTIGS, fq, hits, strand, ops, flags, K)
    flagged = sso.add_dup_flag(plain, dup, K)
    key = sso.sort_keys(CONTIGS, hits, strand, flags, K)
    perm, out_off, want = sso.sort(key, flagged)
    assert counts[1] >= 50 and sum(a != b for a, b in zip(plain, flagged)) >= counts[1] and (key == 2**64 - 1).sum() >= 100
    assert K == 1 or sum(not x for x in plain) >= 100 <= sum(bool(x) for s, x in enumerate(plain) if s % K)
    table = sam.Contigs(CONTIGS)
    header = so.header(CONTIGS).replace(b"SO:unsorted", b"SO:coordinate")
    mp = sam.MarkdupParams(0, K, PHRED, MIN_QUAL)
    assert sam.sorted_sam(fm, sam.SamParams(flags, K), table, fq, hits, strand, ops, markdup=mp, ctx=fm.ctx) == header + want
    # the device calls, chained in HBM
    stream = torch.cuda.current_stream().cuda_stream
    d_table, d_names, d_text, d_recs, d_seq, d_qual, d_hits, d_strand, d_ops = (dev(x) for x in (
        table.table, table.names, fq.text, fq.recs, fq.seq, fq.qual, hits, strand, np.zeros(16, np.uint8)))
    d_dup = torch.full((n,), 0x7e, dtype=torch.uint8, device=DEV)
    assert sam.markdup_dev(mp, n, d_table.data_ptr(), len(table), d_hits.data_ptr(), d_strand.data_ptr(), d_recs.data_ptr(), d_qual.data_ptr(),
                           d_dup.data_ptr(), stream=stream, ctx=fm.ctx) == counts
    d_off = torch.zeros(n * K + 1, dtype=torch.int64, device=DEV)
    emit = (fm, sam.SamParams(flags, K), n, d_table.data_ptr(), len(table), d_names.data_ptr(), d_text.data_ptr(), d_recs.data_ptr(),
            d_seq.data_ptr(), d_qual.data_ptr(), d_hits.data_ptr(), d_strand.data_ptr(), d_ops.data_ptr())
    total = sam.emit_dev(*emit, 0, 0, d_off.data_ptr(), d_dup=d_dup.data_ptr(), stream=stream)
    assert total == len(want)
    d_lines = torch.full((total,), 0x7e, dtype=torch.uint8, device=DEV)
    assert sam.emit_dev(*emit, d_lines.data_ptr(), total, d_off.data_ptr(), d_dup=d_dup.data_ptr(), stream=stream) == total
    d_key = torch.zeros(n * K, dtype=torch.int64, device=DEV)
    sam.sort_keys_dev(sam.SamParams(flags, K), n, d_table.data_ptr(), len(table), d_hits.data_ptr(), d_strand.data_ptr(), d_key.data_ptr(),
                      stream=stream, ctx=fm.ctx)
    d_sorted = torch.full((total + 64,), 0x7e, dtype=torch.uint8, device=DEV)
    d_sorted_off = torch.zeros(n * K + 1, dtype=torch.int64, device=DEV)
    d_perm = torch.zeros(n * K, dtype=torch.int64, device=DEV)
    sam.sort_dev(n * K, d_key.data_ptr(), d_lines.data_ptr(), d_off.data_ptr(), total, d_sorted.data_ptr(), total, d_sorted_off.data_ptr(),
                 d_perm.data_ptr(), stream=stream, ctx=fm.ctx)
    torch.cuda.synchronize()
    assert d_dup.cpu().numpy().tobytes() == dup.tobytes() and d_lines.cpu().numpy().tobytes() == b"".join(flagged)
    assert (d_key.cpu().numpy().astype(np.uint64) == key).all() and (d_perm.cpu().numpy().astype(np.uint64) == perm).all()
    assert (d_sorted_off.cpu().numpy().astype(np.uint64) == out_off).all()
    body = d_sorted.cpu().numpy()
    assert (body[total:] == 0x7e).all() and body[:total].tobytes() == want
    sso.check_sorted_text([c[0] for c in CONTIGS], b"".join(flagged), want)
