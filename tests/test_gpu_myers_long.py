"""The block-based Myers kernels (csrc/myers_long.hip) against the restatement of myers::long at w = 64
(tests/myers_long_oracle.py), records, counts and operations byte for byte through the host and the device flavour: the
reference's known answers through the mirror, every block count with its last block, one-block patterns against the u64
calls, patterns of several block counts in one call, and FASTQ text -> bg_fastq_parse_dev -> bg_myers_long_best_batch_dev
with a 66-symbol adapter -> bg_fastq_trim_dev."""
import random

import numpy as np
import pytest
import torch

import myers_cases as mc
import myers_long_oracle as ml
import myers_oracle as mo
from myers_cases import DEV, dna, mutated, same_best
from myers_long_cases import KATS, check_all, pair
from rust_bio_amd import _lib, fastq, myers

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", KATS, ids=lambda c: c["name"])
def test_known_answers_through_the_mirror(case):
    pattern, ambigs, wildcards = mc.pattern_args(case)
    my, want = pair(pattern, ambigs, wildcards)
    text, k = case["text"].encode(), min(case.get("k", 0xFFFFFFFF), 0xFFFFFFFF)
    ends = want.find_all_end(text, k)
    assert my.distance(b"") == (1 << 64) - 1 - 64 == want.distance(b"")
    if len(ends) > myers.MYERS_MAX_HITS:  # more hits than a job reports: the count and the first 64 of the batch call
        assert case["find_all_end"] == [list(h) for h in ends]
        for ends_only in (False, True):
            rec, count = myers.long_find_all_batch([my], _lib.as_u8(text), np.array([0, len(text)], dtype=np.uint64), k, 64, ends_only)
            wrec, wcount = ml.find_all_records([want], [text], k, 64, ends_only)
            assert int(count[0]) == len(ends) and rec.tobytes() == wrec.tobytes()
        assert my.distance(text) == min(d for _, d in ends) and my.find_best_end(text) == min(ends, key=lambda h: h[1])
        return
    full = my.find_all(text, k)
    best = my.best_alignment(text, k)
    wbest = ml.best_hit(want, text, k)
    got_best = None
    if best is not None:
        got_best = (best["ystart"], best["yend"], best["score"], [myers.OPS.index(o) for o in best["operations"]])
        assert got_best == wbest
    # the path of a hit that is not the text's best: the best call on the text cut at the hit's end, bounded by its distance
    paths = {}
    for hit in mc.named_hits(case):
        s, e, d, ops = want.find_all(text, k)[hit]
        if ml.best_hit(want, text[:e], d) == (s, e, d, ops):
            a = my.best_alignment(text[:e], d)
            paths[hit] = [myers.OPS.index(o) for o in a["operations"]]
            assert (a["ystart"], a["yend"], a["score"]) == (s, e, d)
    assert full == [h[:3] for h in want.find_all(text, k)]
    mc.check_case(case, my.distance(text), my.find_all_end(text, k), full, paths, got_best)
    if "best_end" in case:
        assert list(my.find_best_end(text)) == case["best_end"]


def planted(rng, pattern, n_before, n_behind, rate, alphabet=b"ACGT"):
    return dna(rng, n_before, alphabet) + mutated(rng, pattern, alphabet, rate) + dna(rng, n_behind, alphabet)


@pytest.mark.parametrize("m", [64, 65, 66, 127, 128, 129, 192, 193])
def test_block_counts_and_the_last_block(m):
    """m = 65, 129, 193: a last block of one symbol (long.rs:430-434); 64, 128, 192: a full one"""
    rng = random.Random(m)
    pattern = dna(rng, m)
    texts = [planted(rng, pattern, 7, 5, 0.0), planted(rng, pattern, 0, 9, 0.05), planted(rng, pattern, 30, 0, 0.12),
             pattern[3:-2], pattern[:m // 2], pattern[-1:] + b"T" * 9, b"", dna(rng, 40) + pattern[:-1]]
    for k in (0, 3, m // 10 + 2, m, 10 ** 6):
        best = check_all([pair(pattern)], texts, k)
    assert int(best["score"][0]) == 0 and int(best["n_ops"][0]) == m


@pytest.mark.parametrize("m", [1023, 1024])
def test_sixteen_blocks(m):
    """the largest pattern: texts of at most 300 bytes are shorter than it, so hits need a large max_dist"""
    rng = random.Random(m)
    pattern = dna(rng, m)
    texts = [mutated(rng, pattern[100:330], b"ACGT", 0.03)[:300], pattern[-120:], b"", pattern[:64] + pattern[960:]]
    want = ml.MyersLong(pattern)
    floor = min(d for t in texts if t for _, d in want.find_all_end(t, m))
    for k in (floor - 1, floor + 4, 10 ** 6):
        best = check_all([pair(pattern)], texts, k, max_hits=2)
    assert int(best["score"][1]) == m - 120 and int(best["ystart"][1]) == 0 and int(best["yend"][1]) == 120


@pytest.mark.parametrize("m", [64, 33])
def test_one_block_patterns_give_the_records_of_the_u64_calls(m):
    rng = random.Random(m)
    patterns = [dna(rng, m), dna(rng, m, b"AC"), b"T" * m]
    texts = [planted(rng, patterns[0], 5, 5, 0.1), planted(rng, patterns[1], 0, 30, 0.2, b"AC"), patterns[0][2:-1], b"", b"A" * 64,
             patterns[0] + patterns[1], dna(rng, 150)]
    buf, off = _lib.concat(texts)
    longs, shorts = [myers.MyersLong(p) for p in patterns], [myers.Myers(p) for p in patterns]
    for k in (0, 2, 20, m, 255):
        a, b = myers.long_best_batch(longs, buf, off, k, ops_stride=128), myers.best_batch(shorts, buf, off, k, ops_stride=128)
        assert a[0].tobytes() == b[0].tobytes()
        same_best(a, b, 128)
        for ends_only in (False, True):
            a = myers.long_find_all_batch(longs, buf, off, k, 4, ends_only)
            b = myers.find_all_batch(shorts, buf, off, k, 4, ends_only)
            assert a[0].tobytes() == b[0].tobytes() and (a[1] == b[1]).all()
    # ... and a Myers object is accepted as a one-block pattern
    assert myers.long_best_batch(shorts, buf, off, 5)[0].tobytes() == myers.best_batch(shorts, buf, off, 5)[0].tobytes()
    check_all([pair(p) for p in patterns], texts, 20)


def test_patterns_of_several_block_counts_in_one_call():
    rng = random.Random(4)
    patterns = [dna(rng, m) for m in (20, 70, 130, 300)]
    texts = [planted(rng, p, rng.randint(0, 30), rng.randint(0, 30), rate)[:300] for p in patterns for rate in (0.0, 0.04)]
    texts += [patterns[1] + patterns[0], b"", dna(rng, 200), patterns[3][:299]]
    for k in (3, 12, 10 ** 6):
        check_all([pair(p) for p in patterns], texts, k, max_hits=2)


# ---- the pipeline: parse, match a 66-symbol adapter, trim -------------------------------------------------------------
ADAPTER66 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC" + b"ATCACGAT" + b"ATCTCGTATGCCGTCTTCTGCTTG"  # stem, index, tail
K = 6


def test_parse_match_a_66_symbol_adapter_and_trim():
    from test_gpu_fastq_trim import expected, fastq_bytes, same_columns
    assert len(ADAPTER66) == 66
    rng = random.Random(66)
    records = []
    for r in range(120):
        insert = dna(rng, rng.randint(20, 150))
        kind = 0 if r in (0, 119) else rng.randint(0, 5)
        if kind <= 2:
            seq = insert + mutated(rng, ADAPTER66, b"ACGT", rng.choice([0, 0, 0.04]))
        elif kind == 3:
            seq = insert + ADAPTER66[:rng.choice([64, 40])]  # cut short at the read's end
        else:
            seq = insert
        records.append((seq, bytes(rng.randint(33, 73) for _ in range(len(seq)))))
    fq, n = fastq_bytes(records), len(records)
    stream = torch.cuda.current_stream().cuda_stream
    d_fq = torch.frombuffer(bytearray(fq), dtype=torch.uint8).to(DEV)
    got_n, status, _, d_recs, d_seq, d_so, d_qual, d_qo = fastq.parse_dev(d_fq)
    assert (got_n, status) == (n, "ok")
    pats = [myers.MyersLong(ADAPTER66)]
    d_hits, _ = myers.long_best_batch_dev(pats, d_seq, d_so, K, stream=stream)
    hits = myers.records(d_hits)
    want_hits, _ = ml.best_records([ml.MyersLong(ADAPTER66)], [s for s, _ in records], K)
    assert hits.tobytes() == want_hits.tobytes()
    assert 50 <= (hits["score"] != mo.MIN_SCORE).sum() < n and hits["score"][0] == 0 and hits["score"][-1] == 0
    parsed = fastq.parse_arrays(fq)
    want = expected(mo.TRIM_3P, hits, 1, parsed)
    o_recs, o_seq, o_so, o_qual, o_qo, totals = myers.trim_dev(mo.TRIM_3P, d_hits, 1, n, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream)
    torch.cuda.synchronize()
    same_columns((o_recs.cpu().numpy().view(_lib.FQREC_DTYPE), o_seq.cpu().numpy(), o_so.cpu().numpy().astype(np.uint64),
                  o_qual.cpu().numpy(), o_qo.cpu().numpy().astype(np.uint64)), want)
    assert totals == (len(want[1]), len(want[3])) and totals[0] < sum(len(s) for s, _ in records)
    # the u64 call still refuses the pattern
    raw = np.zeros(1, dtype=_lib.MYERS_PATTERN_DTYPE)
    raw["m"] = 66
    with pytest.raises(_lib.BiogpuError) as e:
        myers.best_batch(raw, parsed.seq, parsed.seq_off, K)
    assert e.value.status == -8
