"""`bg_fastq_qual_cut[_dev]`, `bg_fastq_qual_select[_dev]` and `bg_fastq_qc_tables[_dev]` (csrc/fastq_qual.hip) byte for byte
against the three rules as a few lines of Python (tests/fastq_qual_oracle.py; include/biogpu.h defines them): the device flavour
with and without its host totals and the host flavour.  Batch sizes around the 16 reads of a block and beyond one round of the
grid; read lengths around the 16 symbols of a step and their multiples, and a read of thousands of symbols for the carried state;
shaped reads (all high, all low, the stop at the first symbol and at a step's edge, a maximum reached twice); bytes below the
phred offset; buffers at every alignment; max_cycles at 1, around the longest read, beyond the rows kept in LDS and at the cap;
the three record selections; records whose two lengths differ; the tables' invariants and their determinism."""
import random

import numpy as np
import pytest
import torch

import fastq_qual_oracle as qo
from fastq_qual_cases import CUTOFF, METHOD_PAIRS, PHRED, SELECT_FLAGS, cut_params, qual_string, random_records, select_params
from fastq_write_cases import Batch
from rust_bio_amd import fastq

pytestmark = pytest.mark.gpu
LDS_ROWS = 160  # rows of the tables a block keeps in LDS
HI, LO, AT = bytes([PHRED + 38]), bytes([PHRED + 3]), bytes([PHRED + CUTOFF])


def stream():
    return torch.cuda.current_stream().cuda_stream


def recs_of(quals, seqs=None):
    return [(b"r%d" % i, None, seqs[i] if seqs else b"A" * len(q), q) for i, q in enumerate(quals)]


def cut_checked(b, **cp):
    """both flavours against the rule; returns the rule's [(b, e)]"""
    n = len(b)
    want, want_tot, points = qo.cut(b.qual, b.qual_off, PHRED, **cp)
    d = b.to_dev()
    d_cut, tot = fastq.qual_cut_dev(n, d[4], d[5], stream=stream(), want_totals=True, phred_offset=PHRED, **cp)
    got = d_cut.cpu().numpy().tobytes()
    bad = [r for r in range(n) if got[64 * r:64 * r + 64] != want[r].tobytes()]
    assert not bad, (bad[:8], [points[r] for r in bad[:8]], cp)
    assert tot == want_tot
    d_again, none = fastq.qual_cut_dev(n, d[4], d[5], stream=stream(), phred_offset=PHRED, **cp)
    torch.cuda.synchronize()
    assert none is None and d_again.cpu().numpy().tobytes() == want.tobytes()
    h_cut, h_tot = fastq.qual_cut_arrays(b.qual, b.qual_off, want_totals=True, phred_offset=PHRED, **cp)
    assert h_cut.tobytes() == want.tobytes() and h_tot == want_tot
    return points


def select_checked(b, weight=None, **sp):
    """both flavours against the rule, with each output alone as well; returns the rule's (stats, bin, passed)"""
    n = len(b)
    want = qo.select(b.qual, b.qual_off, phred_offset=PHRED, weight=weight, **sp)
    d = b.to_dev()
    d_stats, d_bin, passed = fastq.qual_select_dev(n, d[4], d[5], weight=weight, stream=stream(), want_totals=True, phred_offset=PHRED, **sp)
    got = d_stats.cpu().numpy().view(qo.STATS_DTYPE)
    bad = [r for r in range(n) if got[r] != want[0][r]]
    assert not bad, (bad[:8], got[bad[:8]], want[0][bad[:8]])
    assert (d_bin.cpu().numpy().view(np.uint32) == want[1]).all() and passed == want[2]
    only_bin = fastq.qual_select_dev(n, d[4], d[5], weight=weight, stream=stream(), want_stats=False, phred_offset=PHRED, **sp)
    only_stats = fastq.qual_select_dev(n, d[4], d[5], weight=weight, stream=stream(), want_bin=False, phred_offset=PHRED, **sp)
    torch.cuda.synchronize()
    assert only_bin[0] is None and only_bin[2] is None and (only_bin[1].cpu().numpy().view(np.uint32) == want[1]).all()
    assert only_stats[1] is None and only_stats[0].cpu().numpy().tobytes() == want[0].tobytes()
    h_stats, h_bin, h_pass = fastq.qual_select_arrays(b.qual, b.qual_off, weight=weight, want_totals=True, phred_offset=PHRED, **sp)
    assert h_stats.tobytes() == want[0].tobytes() and (h_bin == want[1]).all() and h_pass == want[2]
    return want


def tables_checked(b, max_cycles, first=0, step=1):
    """both flavours against the rule, the device flavour twice; the invariants on the rule's own tables; returns them"""
    n = len(b)
    want, t = qo.tables(b.seq, b.seq_off, b.qual, b.qual_off, max_cycles, first, step, PHRED)
    d = b.to_dev()
    got = [fastq.qc_tables_dev(n, d[2], d[3], d[4], d[5], max_cycles, first, step, PHRED, stream=stream()) for _ in range(2)]
    torch.cuda.synchronize()
    bufs = [g.buf.cpu().numpy().view(np.uint64) for g in got]
    assert (bufs[0] == bufs[1]).all()
    for k in ("base", "qhist", "len_hist", "meanq_hist", "n_reads"):
        assert (getattr(got[0], k).cpu().numpy().view(np.uint64) == t[k]).all(), (k, max_cycles, first, step)
    assert (bufs[0] == want).all()
    h = fastq.qc_tables_arrays(b.seq, b.seq_off, b.qual, b.qual_off, max_cycles, first, step, PHRED)
    assert (h.buf == want).all() and (h.qhist == t["qhist"]).all()
    lens = [len(b.records[r][2]) for r in range(first, n, step)]
    assert int(t["n_reads"][0]) == len(lens) == int(t["len_hist"].sum())
    for c in range(max_cycles):
        assert int(t["base"][c].sum()) == sum(ln > c for ln in lens), c
    return t


def all_checked(b, rng, rnd=0, max_cycles=40):
    m5, m3 = METHOD_PAIRS[rnd % len(METHOD_PAIRS)]
    cut_checked(b, **cut_params(rng, m5, m3))
    flags = SELECT_FLAGS[rnd % 3] if len(b) % 2 == 0 else 0
    select_checked(b, weight=qo.ee_weights(PHRED) if rnd % 2 else None, max_weight=3 << 20, **select_params(rng, flags))
    tables_checked(b, max_cycles)


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 33])
def test_batch_sizes_around_a_block(n):
    rng = random.Random(100 + n)
    for rnd in range(3):
        all_checked(Batch(random_records(rng, n, hi=60), a_seq=rnd, a_qual=2 * rnd + 1), rng, rnd + n)


def test_more_reads_than_one_round_of_the_grid():
    # the tables take three blocks of 32 reads per compute unit a round (256 of them): the second round starts inside a pair
    rng = random.Random(7)
    pool = [qual_string(rng, ln, 0.5) for ln in (0, 1, 3, 5, 17) for _ in range(8)]
    n = 3 * 256 * 32 + 18
    quals = [pool[(r * 7 + r // 40) % 40] for r in range(n)]
    b = Batch(recs_of(quals, [bytes(b"ACGTN"[(r + i) % 5] for i in range(len(q))) for r, q in enumerate(quals)]))
    tables_checked(b, 4, 1, 2)
    tables_checked(b, 20)
    # the cut and the select take 8192 blocks a round.  The rules look at one read (one pair) at a time, so they are applied
    # to the 40 strings of the pool and the results laid out as the batch is
    n = 8192 * 16 + 18
    idx = np.array([(r * 7 + r // 40) % 40 for r in range(n)])
    p_off = np.cumsum([0] + [len(q) for q in pool])
    cp = dict(method_5p=qo.RUNSUM, method_3p=qo.RUNSUM, cutoff_5p=CUTOFF, cutoff_3p=CUTOFF)
    p_cut = qo.cut(b"".join(pool), p_off, PHRED, **cp)[0]
    sp = dict(min_mean_q=CUTOFF, low_q=CUTOFF, max_low_pct=50)
    p_stats, p_bin, _ = qo.select(b"".join(pool), p_off, phred_offset=PHRED, **sp)
    col = np.frombuffer(b"".join(pool[i] for i in idx) + b"#", dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum(np.array([len(q) for q in pool])[idx])]).astype(np.int64)
    d_qual, d_off = torch.from_numpy(col.copy()).to("cuda:0"), torch.from_numpy(off).to("cuda:0")
    d_cut, tot = fastq.qual_cut_dev(n, d_qual, d_off, stream=stream(), want_totals=True, phred_offset=PHRED, **cp)
    want = p_cut[idx]
    assert d_cut.cpu().numpy().tobytes() == want.tobytes()
    removed = np.where(want["score"] == qo.MIN_SCORE, 0, want["score"]).astype(np.int64)
    assert tot == (int((removed > 0).sum()), int(removed.sum())) and 0 < tot[0] < n
    d_stats, d_bin, passed = fastq.qual_select_dev(n, d_qual, d_off, stream=stream(), want_totals=True, flags=qo.PAIRED, phred_offset=PHRED, **sp)
    fail = p_bin[idx].reshape(-1, 2).max(axis=1).repeat(2)  # a pair passes if both mates do
    assert d_stats.cpu().numpy().tobytes() == p_stats[idx].tobytes()
    assert (d_bin.cpu().numpy().view(np.uint32) == fail).all() and passed == int((fail == 0).sum()) and 0 < passed < n
    assert (fail[-18:] == 0).any() and (fail[-18:] == 1).any() and (p_bin[idx] != fail).any()


@pytest.mark.parametrize("m5,m3", METHOD_PAIRS)
def test_read_lengths_around_a_step_and_a_long_read(m5, m3):
    rng = random.Random(11 + 3 * m5 + m3)
    lengths = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257]
    for window in (1, 2, 4, 5, 16, 17, 300):
        quals = [qual_string(rng, ln, p) for ln in lengths for p in (0.05, 0.5, 0.95)]
        quals.insert(5, qual_string(rng, 3000 + window, 0.9)[:2900] + qual_string(rng, 100 + window, 0.3))  # mostly low: a long carry
        quals.insert(9, qual_string(rng, 2500, 0.02))
        b = Batch(recs_of(quals), a_qual=window % 16)
        cut_checked(b, method_5p=m5, method_3p=m3, cutoff_5p=CUTOFF, cutoff_3p=CUTOFF, window=window)
        if m3 == qo.NONE:
            break  # the window is not looked at
    select_checked(b, weight=qo.ee_weights(PHRED), max_weight=1 << 21, low_q=CUTOFF, max_low_pct=30, min_mean_q=CUTOFF)


def test_shaped_reads():
    both = dict(method_5p=qo.RUNSUM, method_3p=qo.RUNSUM, cutoff_5p=CUTOFF, cutoff_3p=CUTOFF)
    below = bytes([PHRED - 1])
    quals = [HI * 40, LO * 40, AT * 40, below * 40, HI * 16, LO * 16, LO * 17, LO * 15,
             HI + LO * 39, LO * 39 + HI,                        # the stop fires at the first symbol of an end
             LO * 15 + HI * 20 + LO * 15, LO * 16 + HI * 20 + LO * 16, LO * 17 + HI * 20 + LO * 17,  # ... around a step's edge
             LO * 2 + bytes([PHRED + CUTOFF + 17]) * 2 + LO * 2 + HI * 30,  # the maximum of s twice: the first one wins
             HI * 30 + LO * 2 + bytes([PHRED + CUTOFF + 17]) * 2 + LO * 2,
             LO * 14 + bytes([PHRED + CUTOFF + 17]) * 2 + LO * 2 + HI * 30,  # ... the second one in the next step
             AT * 5 + LO + AT * 20 + LO + AT * 5,                # s stays where it is over symbols at the cutoff
             below * 3 + HI * 10 + below * 3, HI * 3 + below * 40 + HI * 3]
    for a_qual in range(16):
        b = Batch(recs_of(quals), a_qual=a_qual)
        points = cut_checked(b, **both)
        cut_checked(b, method_5p=qo.RUNSUM, method_3p=qo.WINDOW, cutoff_5p=CUTOFF, cutoff_3p=CUTOFF, window=4)
        if a_qual % 5 == 0:
            select_checked(b, min_mean_q=CUTOFF, low_q=CUTOFF, max_low_pct=25)
            tables_checked(b, 40)
    assert points[:4] == [(0, 40), (40, 40), (0, 40), (40, 40)] and points[8:10] == [(0, 1), (39, 40)]
    assert points[10:13] == [(15, 35), (16, 36), (17, 37)]
    assert points[13:16] == [(2, 36), (0, 34), (14, 48)] and points[16] == (27, 27)
    # cutoffs beyond every quality, and beyond what 32 bits hold of a sum
    for cutoff in (255, 256, 257, 0xFFFFFFFF):
        assert cut_checked(b, method_5p=qo.RUNSUM, method_3p=qo.NONE, cutoff_5p=cutoff)[0] == (40, 40)
        assert cut_checked(b, method_5p=qo.NONE, method_3p=qo.WINDOW, cutoff_3p=cutoff, window=0xFFFFFFFF)[0] == (0, 0)
    assert cut_checked(b, method_5p=qo.NONE, method_3p=qo.NONE) == [(0, len(q)) for q in quals]


def test_select_with_and_without_a_table():
    rng = random.Random(5)
    b = Batch(random_records(rng, 64, hi=120), a_qual=3)
    weight = qo.ee_weights(PHRED)
    sums = sorted(qo.stats_of(r[3], PHRED, 0, weight)["weight_sum"] for r in b.records)
    at = sums[20]
    for flags in SELECT_FLAGS:
        stats, bins, passed = select_checked(b, weight=weight, flags=flags, max_weight=at)
        if flags == 0:  # a read whose sum is the bound passes, the next larger one fails
            assert passed == sum(s <= at for s in sums) and (bins == (stats["weight_sum"] > at)).all()
        assert select_checked(b, flags=flags, max_weight=0)[2] == 64  # no table: the bound is not looked at
        select_checked(b, weight=weight, flags=flags, max_weight=at - 1)
        select_checked(b, weight=rng.sample(range(1 << 32), 256), max_weight=1 << 37, **select_params(rng, flags))
    # the device wrapper's max_ee is the same table and bound
    d = b.to_dev()
    got = fastq.qual_select_dev(64, d[4], d[5], max_ee=at / 2 ** 20, stream=stream(), want_totals=True)
    assert got[2] == sum(s <= at for s in sums)
    for low_q, pct in ((CUTOFF, 0), (CUTOFF, 100), (CUTOFF, 101), (0, 0), (300, 99)):
        select_checked(b, low_q=low_q, max_low_pct=pct)
    select_checked(b, min_mean_q=0xFFFFFFFF)


def test_tables_at_the_edges_of_max_cycles():
    rng = random.Random(13)
    records = random_records(rng, 90, hi=60, equal=0.6)
    longest = 200
    records[7] = (b"long", None, bytes(rng.choice(b"ACGTacgtNx") for _ in range(longest)), qual_string(rng, longest, 0.3))
    records[8] = (b"longq", None, b"ACGT", qual_string(rng, 190, 0.3))
    b = Batch(records, a_seq=5, a_qual=9)
    assert max(len(r[2]) for r in records) == longest and sum(len(r[2]) != len(r[3]) for r in records) > 20
    for mc in (1, longest - 1, longest, longest + 1, LDS_ROWS - 1, LDS_ROWS, LDS_ROWS + 1, 1024):
        for first, step in ((0, 1), (0, 2), (1, 2)):
            t = tables_checked(b, mc, first, step)
        if LDS_ROWS < mc < longest:  # rows in LDS, rows added to directly, and the collecting row all hold counts
            assert t["base"][LDS_ROWS - 1].sum() and t["base"][LDS_ROWS].sum() and t["base"][mc].sum() and t["qhist"][mc].sum()
    assert tables_checked(b, 30, 5, 1000)["n_reads"][0] == 1 and tables_checked(b, 30, 90, 1)["n_reads"][0] == 0
