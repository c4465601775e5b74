"""`bg_fastq_filter[_dev]` (csrc/fastq_emit.hip) column for column against the filter rule as a few lines of Python
(tests/fastq_write_oracle.py: filter_columns; include/biogpu.h defines the rule): the length bounds at their edges, the 'N'
count at the edges of the 16-lane groups, `check`, the two DISCARD flags on hand-made hit records, the pair rule, nothing and
everything kept, record counts around the scan's 2048-item block, the optional outputs and the host flavour."""
import random

import numpy as np
import pytest
import torch

import fastq_write_oracle as fw
from fastq_write_cases import Batch, random_records
from rust_bio_amd import _lib, fastq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def hit_records(trimmed, n_pat, rng=None):
    """bg_alignment_t[n * n_pat]: a record that is `trimmed` has a hit in one (random) pattern, the others have none"""
    rng = rng or random.Random(0)
    hits = np.zeros(len(trimmed) * n_pat, dtype=_lib.ALN_DTYPE)
    hits["score"] = fw.MIN_SCORE
    for r, t in enumerate(trimmed):
        if t:
            hits["score"][r * n_pat + rng.randrange(n_pat)] = rng.randint(0, 3)
    return hits


def same(got, want, n):
    recs, seq, so, qual, qo, keep = got
    w_recs, w_seq, w_so, w_qual, w_qo, w_keep = want
    k = len(w_recs)
    assert len(recs) == k
    assert recs.tobytes() == w_recs.tobytes()
    assert (np.asarray(so[:k + 1], dtype=np.uint64) == w_so).all() and (np.asarray(qo[:k + 1], dtype=np.uint64) == w_qo).all()
    assert bytes(seq[:len(w_seq)]) == w_seq and bytes(qual[:len(w_qual)]) == w_qual
    if keep is not None:
        assert bytes(keep[:n]) == w_keep.tobytes()


def filter_checked(batch, hits=None, n_pat=0, **flt):
    """the device flavour with totals and keep, without either, and the host flavour, all against the rule; returns the rule's columns"""
    n = len(batch)
    want = fw.filter_columns(*batch.columns(), hits=hits, n_pat=n_pat, **flt)
    _, d_recs, d_seq, d_so, d_qual, d_qo = batch.to_dev(DEV)
    d_hits = torch.from_numpy(hits.view(np.uint8).copy()).to(DEV) if hits is not None else None
    stream = torch.cuda.current_stream().cuda_stream
    o_recs, o_seq, o_so, o_qual, o_qo, d_keep, totals = fastq.filter_dev(n, d_recs, d_seq, d_so, d_qual, d_qo, d_hits=d_hits, n_pat=n_pat,
                                                                         stream=stream, want_keep=True, **flt)
    assert totals == (len(want[0]), len(want[1]), len(want[3]))
    same((o_recs.cpu().numpy().view(_lib.FQREC_DTYPE), o_seq.cpu().numpy(), o_so.cpu().numpy(), o_qual.cpu().numpy(), o_qo.cpu().numpy(),
          d_keep.cpu().numpy()), want, n)
    # no totals: the call does not wait; no keep
    a_recs, a_seq, a_so, a_qual, a_qo, a_keep, none = fastq.filter_dev(n, d_recs, d_seq, d_so, d_qual, d_qo, d_hits=d_hits, n_pat=n_pat,
                                                                       stream=stream, want_totals=False, **flt)
    torch.cuda.synchronize()
    assert none is None and a_keep is None
    k = totals[0]
    same((a_recs.cpu().numpy().view(_lib.FQREC_DTYPE)[:k], a_seq.cpu().numpy(), a_so.cpu().numpy(), a_qual.cpu().numpy(), a_qo.cpu().numpy(), None),
         want, n)
    same(fastq.filter_arrays(*batch.columns(), hits=hits, n_pat=n_pat, **flt), want, n)
    return want


def test_length_bounds_at_their_edges():
    lens = [19, 20, 21, 30, 31, 0, 1, 20, 30]
    b = Batch([(b"r%d" % i, None, b"A" * ln, b"I" * ln) for i, ln in enumerate(lens)])
    assert list(filter_checked(b, min_len=20, max_len=30)[5]) == [0, 1, 1, 1, 0, 0, 0, 1, 1]
    assert list(filter_checked(b, min_len=1)[5]) == [1, 1, 1, 1, 1, 0, 1, 1, 1]
    assert list(filter_checked(b, max_len=0)[5]) == [0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert list(filter_checked(b, min_len=20, max_len=20)[5]) == [0, 1, 0, 0, 0, 0, 0, 1, 0]


def test_n_count_at_the_group_edges():
    records = []
    for ln in (1, 16, 17, 150):
        for pos in sorted({0, ln - 1} | {p for p in (15, 16, 17) if p < ln}):
            for ch in b"Nn":
                s = bytearray(b"A" * ln)
                s[pos] = ch
                records.append((b"L%dp%d" % (ln, pos), None, bytes(s), b"I" * ln))
    for k in (2, 3):  # exactly max_n and max_n + 1 of them, spread over the lanes
        for ln in (17, 150):
            s = bytearray(b"C" * ln)
            for p in [0, ln - 1, 8][:k]:
                s[p] = ord("N") if p % 2 else ord("n")
            records.append((b"k%dL%d" % (k, ln), None, bytes(s), b"I" * ln))
    records.append((b"none", None, b"ACGT" * 20, b"I" * 80))
    records.append((b"empty", None, b"", b""))
    records.append((b"all", None, b"N" * 150, b"I" * 150))
    b = Batch(records)
    n_single = len(records) - 7
    keep0 = filter_checked(b, max_n=0)[5]
    assert not keep0[:n_single].any() and list(keep0[n_single:]) == [0, 0, 0, 0, 1, 1, 0]
    keep2 = filter_checked(b, max_n=2)[5]
    assert keep2[:n_single].all() and list(keep2[n_single:]) == [1, 1, 0, 0, 1, 1, 0]
    assert filter_checked(b, max_n=150)[5].all()
    assert filter_checked(b, max_n=149, min_len=1)[5].sum() == len(records) - 2


def test_check_ok_with_one_record_of_each_kind():
    b = Batch([(b"c%d" % c, None, b"ACGT", b"IIII") for c in range(6)], checks=list(range(6)))
    assert list(filter_checked(b, flags=fw.CHECK_OK)[5]) == [1, 0, 0, 0, 0, 0]
    assert filter_checked(b)[5].all()


@pytest.mark.parametrize("n_pat", [1, 3])
def test_discard_flags_on_hand_made_hits(n_pat):
    rng = random.Random(n_pat)
    b = Batch(random_records(rng, 40, 0, 40))
    trimmed = [rng.random() < 0.5 for _ in range(40)]
    trimmed[0], trimmed[-1] = True, False
    hits = hit_records(trimmed, n_pat, rng)
    assert list(filter_checked(b, hits, n_pat, flags=fw.DISCARD_UNTRIMMED)[5]) == [int(t) for t in trimmed]
    assert list(filter_checked(b, hits, n_pat, flags=fw.DISCARD_TRIMMED)[5]) == [int(not t) for t in trimmed]
    assert filter_checked(b, hits, n_pat)[5].all()  # without a flag the hits do not matter
    assert filter_checked(b, hits, n_pat, flags=fw.DISCARD_TRIMMED, min_len=5)[5].sum() < sum(not t for t in trimmed)


def test_pair_rule():
    lens = [30, 30, 30, 5, 5, 30, 5, 5] * 3  # pass/pass, pass/fail, fail/pass, fail/fail
    b = Batch([(b"p%d" % (i // 2), b"%d" % (i % 2 + 1), b"G" * ln, b"I" * ln) for i, ln in enumerate(lens)])
    assert list(filter_checked(b, min_len=20)[5]) == [1, 1, 1, 0, 0, 1, 0, 0] * 3
    assert list(filter_checked(b, flags=fw.PAIRED, min_len=20)[5]) == [1, 1, 0, 0, 0, 0, 0, 0] * 3
    assert list(filter_checked(b, flags=fw.PAIRED | fw.PAIR_BOTH, min_len=20)[5]) == [1, 1, 1, 1, 1, 1, 0, 0] * 3
    assert list(filter_checked(b, flags=fw.PAIRED, min_len=20, max_n=3)[5]) == [1, 1, 0, 0, 0, 0, 0, 0] * 3  # the 16-lane pass kernel
    assert list(filter_checked(b, flags=fw.PAIRED | fw.PAIR_BOTH, min_len=20, max_n=3)[5]) == [1, 1, 1, 1, 1, 1, 0, 0] * 3


def test_nothing_and_everything_kept():
    rng = random.Random(5)
    b = Batch(random_records(rng, 100, 0, 60))
    want = filter_checked(b, min_len=1000)
    assert len(want[0]) == 0 and list(want[2]) == [0] and list(want[4]) == [0]
    _, d_recs, d_seq, d_so, d_qual, d_qo = b.to_dev(DEV)
    res = fastq.filter_dev(100, d_recs, d_seq, d_so, d_qual, d_qo, min_len=1000)
    assert res[6] == (0, 0, 0) and res[2].cpu().tolist() == [0] and res[4].cpu().tolist() == [0]
    # nothing switched on: a copy, byte for byte
    o_recs, o_seq, o_so, o_qual, o_qo, _, totals = fastq.filter_dev(100, d_recs, d_seq, d_so, d_qual, d_qo)
    assert totals == (100, len(b.seq), len(b.qual))
    assert o_recs.cpu().numpy().tobytes() == b.recs.tobytes()
    assert torch.equal(o_so, d_so) and torch.equal(o_qo, d_qo)
    assert o_seq.cpu().numpy()[:len(b.seq)].tobytes() == b.seq and o_qual.cpu().numpy()[:len(b.qual)].tobytes() == b.qual
    filter_checked(b)
    # no record at all
    empty = fastq.filter_arrays(b.recs[:0], b"", [0], b"", [0], min_len=1)
    assert len(empty[0]) == 0 and list(empty[2]) == [0] and list(empty[4]) == [0]
    e = Batch([])
    _, d_recs, d_seq, d_so, d_qual, d_qo = e.to_dev(DEV)
    res = fastq.filter_dev(0, d_recs, d_seq, d_so, d_qual, d_qo, flags=fw.PAIRED)
    assert res[6] == (0, 0, 0) and res[2].cpu().tolist() == [0] and res[4].cpu().tolist() == [0]


@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_counts_around_the_scan_block(n):
    rng = random.Random(n)
    b = Batch(random_records(rng, n, 0, 8))
    want = filter_checked(b, min_len=3, max_n=1)
    assert 0 < len(want[0]) < n
    ids = [rec[0] for rec, k in zip(b.records, want[5]) if k]  # kept order is input order
    assert [b.text[int(c["id_off"]):int(c["id_off"] + c["id_len"])] for c in want[0]] == ids
    if n % 2 == 0:
        filter_checked(b, flags=fw.PAIRED, min_len=3)
