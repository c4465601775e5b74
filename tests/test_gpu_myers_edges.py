"""The Myers kernels (csrc/myers.hip) at the smallest shapes where they can go wrong, every call of both flavours
byte for byte against the restatement (tests/myers_oracle.py): pattern lengths around the 32-bit halves of the bit
vectors, text lengths around the pattern's and the 8-byte words a lane loads, hits at the edges of the stored columns,
misaligned text pointers between guard bytes, wavefront and block boundaries in the number of texts, pattern groups,
sub-batches, ties, hit slots and operation slots that are too small."""
import random

import numpy as np
import pytest
import torch

import myers_cases as mc
import myers_oracle as mo
from myers_cases import DEV, both_best, both_find_all, dev, dna, same_best
from rust_bio_amd import _lib, myers

pytestmark = pytest.mark.gpu
MS = [1, 2, 31, 32, 33, 63, 64]
OPS_CAP = -9


def pair(pattern, ambigs=None, wildcards=None):
    """(mirror, restatement) of one pattern"""
    b = myers.MyersBuilder()
    for sym, eq in (ambigs or {}).items():
        b.ambig(sym, eq)
    for w in wildcards or ():
        b.text_wildcard(w)
    return b.build_64(pattern), mo.Myers(pattern, ambigs, wildcards)


def check_all(pairs, texts, k, max_hits=4, stride=128):
    """the best call and both find-all calls, host and device flavour, against the restatement"""
    pats, want = [p[0] for p in pairs], [p[1] for p in pairs]
    wbest = mo.best_records(want, texts, k, stride)
    for got in both_best(pats, texts, k, stride):
        same_best(got, wbest, stride)
    for ends_only in (False, True):
        wrec, wcount = mo.find_all_records(want, texts, k, max_hits, ends_only)
        for rec, count in both_find_all(pats, texts, k, max_hits, ends_only):
            assert (count == wcount).all()
            assert rec.tobytes() == wrec.tobytes()
    return wbest[0]


@pytest.mark.parametrize("m", MS)
def test_text_lengths_and_bounds(m):
    rng = random.Random(m)
    pattern = dna(rng, m)
    lengths = [0, 1, m - 1, m, m + 1, 15, 16, 17, 2 * m + 1, 2 * m + 2, 2 * m + 3, 4 * m + 5]
    texts = []
    for n in lengths:
        t = bytearray(dna(rng, n))
        if n >= m:  # a planted copy with an edit or two
            at = rng.randint(0, n - m)
            t[at:at + m] = pattern
            if m > 2:
                t[at + m // 2] = ord("T") if pattern[m // 2] != ord("T") else ord("A")
        texts.append(bytes(t))
    for k in sorted({0, 1, m - 1, m, 255}):
        check_all([pair(pattern)], texts, k)


@pytest.mark.parametrize("m", [32, 33, 64])
def test_carry_across_bit_31(m):
    """the add of xh must carry from bit 31 into bit 32: a run of matches over symbols 28 .. 36 between mismatches, a full
    self-match (the carry ripples through every bit) and the all-mismatch text of test_large_dist"""
    rng = random.Random(31)
    pattern = dna(rng, m, b"ACG")
    run = b"T" * 28 + pattern[28:min(37, m)] + b"T" * (m - min(37, m))
    texts = [b"TTT" + run + b"TT", run, pattern, b"TT" + pattern * 2, pattern[:31] + pattern[33:], b"A" * 64]
    mono = pair(b"T" * m)
    same = pair(b"A" * m)
    for k in (0, 3, m, 255):
        check_all([pair(pattern), mono, same], texts, k)
    best = check_all([mono], [b"A" * 64], 64)  # common_tests.rs:307-327: every column is a hit of distance m
    assert int(best["score"][0]) == m


@pytest.mark.parametrize("m", [2, 31, 33, 64])
def test_best_end_at_the_edges_of_the_stored_columns(m):
    rng = random.Random(100 + m)
    pattern = dna(rng, m, b"ACG")
    for k in (1, m, 255):
        ring = m + min(k, m) + 2
        texts = [pattern[-1:] + b"T" * 20,        # column 0: only the last symbol matches
                 b"T" * 37 + pattern]              # the last column
        for end in (ring - 4, ring - 3, ring - 2, 2 * m + 1, 2 * m + 2):  # the first stored column is the max state, the initial state,
            if end + 1 >= m:                                              # the text's first column ...
                texts.append(b"T" * (end + 1 - m) + pattern + b"T" * 9)
        best = check_all([pair(pattern)], texts, k)
        if k >= m - 1:
            assert (int(best["yend"][0]), int(best["score"][0])) == (1, m - 1)
        assert (int(best["yend"][1]), int(best["score"][1])) == (37 + m, 0)


@pytest.mark.parametrize("m", [5, 33, 64])
def test_texts_shorter_than_the_pattern(m):
    rng = random.Random(m)
    pattern = b"CATGC" if m == 5 else dna(rng, m)  # m = 5: test_shorter's pattern
    texts = [pattern[1:-1], pattern[2:-3], pattern[1:m // 2] + pattern[m // 2 + 1:-1], pattern[:1], b""]
    want = mo.Myers(pattern)
    paths = [h[3] for t in texts for h in [mo.best_hit(want, t, 6)] if h]
    assert any(o[0] == mo.INS and o[-1] == mo.INS for o in paths)  # as test_shorter: a path that begins and ends with Ins
    for k in (2, 6, m, 255):
        check_all([pair(pattern)], texts, k)


@pytest.mark.parametrize("delta", [1, 3, 7])
def test_misaligned_text_between_guard_bytes(delta):
    """the text starts `delta` bytes past an 8-byte boundary; copies of the pattern lie directly before and behind it, so
    that a kernel that reads a byte outside [off[0], off[n]) reports a hit the restatement does not have"""
    rng = random.Random(delta)
    pattern = b"ACGGTCA"
    (my, want), k = pair(pattern), 1
    texts = [dna(rng, n, b"TTAC") for n in (5, 9, 0, 16, 23, 8, 1, 40)]
    texts[0] = pattern[2:]          # continues a guard copy that ends where the text begins
    texts[-1] = texts[-1][:-4] + pattern[:4]  # ... and is continued by the guard behind
    body = b"".join(texts)
    lead = pattern * 3 + b"G" * ((delta - 3 * len(pattern) - 2) % 8) + pattern[:2]  # 8 q + delta bytes that texts[0] continues
    guard = pattern[4:] + pattern * 2
    assert len(lead) % 8 == delta
    d_buf = dev(np.frombuffer(lead + body + guard, np.uint8))
    assert d_buf.data_ptr() % 8 == 0
    off = np.zeros(len(texts) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t) for t in texts])
    wrec, wops = mo.best_records([want], texts, k, 16)
    wall = mo.find_all_records([want], texts, k, 4, False)
    wends = mo.find_all_records([want], texts, k, 4, True)
    stream = torch.cuda.current_stream().cuda_stream
    # (a) the pointer itself is misaligned, offsets from 0; (b) an aligned pointer and offsets that start at the lead's length
    for d_text, shift in ((d_buf[len(lead):], 0), (d_buf, len(lead))):
        assert (d_text.data_ptr() + shift) % 8 == delta
        d_off = dev(off + shift, np.int64)
        d_aln, d_ops = myers.best_batch_dev([my], d_text, d_off, k, ops_stride=16, stream=stream)
        same_best((myers.records(d_aln), d_ops.cpu().numpy()), (wrec, wops), 16)
        d_aln, d_count = myers.find_all_batch_dev([my], d_text, d_off, k, 4, stream=stream)
        assert myers.records(d_aln).tobytes() == wall[0].tobytes() and (d_count.cpu().numpy() == wall[1]).all()
        d_aln, d_count = myers.find_all_batch_dev([my], d_text, d_off, k, 4, True, stream=stream)
        assert myers.records(d_aln).tobytes() == wends[0].tobytes() and (d_count.cpu().numpy() == wends[1]).all()
    # the host flavour with offsets that do not start at 0
    host = np.frombuffer(lead + body + guard, np.uint8)
    rec, ops = myers.best_batch([my], host, (off + len(lead)).astype(np.uint64), k, ops_stride=16)
    same_best((rec, ops), (wrec, wops), 16)


@pytest.fixture()
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def with_ctx(ctx, pairs, texts, k, max_hits=4, stride=128):
    pats, want = [p[0] for p in pairs], [p[1] for p in pairs]
    buf, off = _lib.concat(texts)
    wrec, wops = mo.best_records(want, texts, k, stride)
    same_best(myers.best_batch(pats, buf, off, k, ops_stride=stride, ctx=ctx), (wrec, wops), stride)
    stream = torch.cuda.current_stream().cuda_stream
    d_text, d_off = dev(buf) if len(buf) else torch.zeros(1, dtype=torch.uint8, device=DEV), dev(off, np.int64)
    d_aln, d_ops = myers.best_batch_dev(pats, d_text, d_off, k, ops_stride=stride, ctx=ctx, stream=stream)
    torch.cuda.synchronize()
    same_best((myers.records(d_aln), d_ops.cpu().numpy()), (wrec, wops), stride)
    for ends_only in (False, True):
        w = mo.find_all_records(want, texts, k, max_hits, ends_only)
        rec, count = myers.find_all_batch(pats, buf, off, k, max_hits, ends_only, ctx=ctx)
        assert rec.tobytes() == w[0].tobytes() and (count == w[1]).all()
        d_aln, d_count = myers.find_all_batch_dev(pats, d_text, d_off, k, max_hits, ends_only, ctx=ctx, stream=stream)
        torch.cuda.synchronize()
        assert myers.records(d_aln).tobytes() == w[0].tobytes() and (d_count.cpu().numpy() == w[1]).all()


@pytest.mark.parametrize("n_texts", [1, 63, 64, 65, 257])
def test_text_counts_with_empty_texts_and_sub_batches(ctx, n_texts):
    """wavefront and block boundaries in the number of texts, empty texts in the middle, three patterns of different
    lengths; with 257 texts the launches are cut at 256 jobs (771 jobs: four launches of each pattern group)"""
    rng = random.Random(n_texts)
    pairs = [pair(b"ACGTA"), pair(b"GGATCCGGATCCGGATCCGGATCCGGATCCGGATC"), pair(b"T")]
    texts = []
    for _ in range(n_texts):
        t = dna(rng, rng.randint(0, 40))
        if rng.random() < 0.6:  # a mutated copy of one of the patterns
            at = rng.randint(0, len(t))
            t = t[:at] + mc.mutated(rng, rng.choice([b"ACGTA", b"GGATCCGGATCCGGATCCGGATCCGGATCCGGATC"]), b"ACGT", 0.06) + t[at:]
        texts.append(t)
    for i in range(n_texts // 2, n_texts, 7):
        texts[i] = b""
    texts[n_texts // 2] = b""
    if n_texts == 257:
        ctx.set_option("myers_chunk_jobs", 256)
    with_ctx(ctx, pairs, texts, 2)


@pytest.mark.parametrize("n_pat", [1, 3, 30])
def test_pattern_counts_and_lds_groups(ctx, n_pat):
    """30 patterns over 20 symbols (21 byte classes: 168 bytes of LDS each) with the table budget lowered to 4 KB: 22 fit,
    the call runs two groups"""
    rng = random.Random(n_pat)
    alphabet = bytes(range(65, 85))
    patterns = [dna(rng, rng.choice([3, 9, 33, 64]), alphabet) for _ in range(n_pat)]
    pairs = [pair(p) for p in patterns]
    texts = [dna(rng, rng.randint(0, 90), alphabet) for _ in range(20)]
    for i, p in enumerate(patterns[:20]):  # a text each with a copy of the pattern that lacks its middle symbol
        texts[i] = texts[i][:10] + p[:len(p) // 2] + p[len(p) // 2 + 1:] + texts[i][10:]
    if n_pat == 30:
        ctx.set_option("myers_lds_bytes", 4096)
    with_ctx(ctx, pairs, texts, 3)


def test_ambiguity_codes_and_a_text_wildcard():
    ambigs = {ord("R"): list(b"AG"), ord("Y"): list(b"CT"), ord("N"): list(b"ACGT")}
    pairs = [pair(b"ACRTYGNA", ambigs), pair(b"ACRTYGNA", ambigs, [ord("*"), ord("N")]), pair(b"ACRTYGNA")]
    texts = [b"TTACATCGTATT", b"ACGTTGCA", b"ACRTYGNA", b"AC*T*G*A", b"NNNNNNNN", b"ACTTCGAA", b"", b"GGACATCGA*ACATTGTAGG"]
    for k in (0, 1, 8):
        check_all(pairs, texts, k)


def test_equal_best_distances_take_the_first_end():
    pattern = b"ACGGTCAGT"
    texts = [b"TT" + pattern + b"TTT" + pattern + b"T" + pattern,                       # three exact copies
             b"TT" + pattern[:4] + pattern[5:] + b"TTT" + pattern[:4] + b"T" + pattern[5:],  # two at distance 1, one end each ... or more
             pattern[:-1] + b"TT" + pattern[:-1],
             b"ACACACACACAC"]
    best = check_all([pair(pattern), pair(b"AC")], texts, 2, max_hits=4)
    assert (int(best["yend"][0]), int(best["score"][0])) == (2 + len(pattern), 0)
    assert (int(best["yend"][7]), int(best["score"][7])) == (2, 0)  # "AC" in "ACAC...": six exact ends, the first wins


@pytest.mark.parametrize("max_hits", [1, 4])
def test_hit_slots(max_hits):
    """jobs with no hit, exactly max_hits hits and more: count is the total, the slots hold the first hits in text order"""
    pattern = b"ACGGT"
    texts = [b"TTTTTTTT", b"TT".join([pattern] * max_hits), b"T".join([pattern] * (max_hits + 2)), b"", pattern]
    want = mo.Myers(pattern)
    assert [len(want.find_all_end(t, 0)) for t in texts] == [0, max_hits, max_hits + 2, 0, 1]
    check_all([pair(pattern)], texts, 0, max_hits=max_hits)
    check_all([pair(pattern)], texts, 1, max_hits=max_hits)


def test_operation_slots_too_small():
    """ops_stride = m + 1: a path with two or more deleted text bytes does not fit (two jobs; one fits exactly).  BG_ERR_OPS_CAP from the call, and in
    the job's record with its exact n_ops; the other jobs are answered in full"""
    pattern = b"ACGGTCAGTTGCA"
    m, stride = len(pattern), len(pattern) + 1
    texts = [pattern, pattern[:5] + b"TT" + pattern[5:], pattern[:4] + b"C" + pattern[4:], pattern[:6] + b"TTT" + pattern[6:],
             b"TTTT", pattern[1:]]
    my, want = pair(pattern)
    wide, wops = mo.best_records([want], texts, 4, 128)
    assert [int(n) for n in wide["n_ops"]] == [m, m + 2, m + 1, m + 3, 0, m]
    buf, off = _lib.concat(texts)
    with pytest.raises(_lib.BiogpuError) as e:
        myers.best_batch([my], buf, off, 4, ops_stride=stride)
    assert e.value.status == OPS_CAP
    stream = torch.cuda.current_stream().cuda_stream
    d_aln, d_ops = myers.best_batch_dev([my], dev(buf), dev(off, np.int64), 4, ops_stride=stride, stream=stream, allow_ops_cap=True)
    torch.cuda.synchronize()
    for rec, ops in (myers.best_batch([my], buf, off, 4, ops_stride=stride, allow_ops_cap=True), (myers.records(d_aln), d_ops.cpu().numpy())):
        for j in range(len(texts)):
            w = wide[j].copy()
            n = int(w["n_ops"])
            if n > stride:
                w["status"], w["ops_off"] = OPS_CAP, j * stride
            elif n:
                w["ops_off"] = (j + 1) * stride - n
                assert ops[(j + 1) * stride - n:(j + 1) * stride].tobytes() == wops[(j + 1) * 128 - n:(j + 1) * 128].tobytes(), j
            assert rec[j].tobytes() == w.tobytes(), j
    # without an operations buffer nothing can overflow: same coordinates and counts, no error
    rec, _ = myers.best_batch([my], buf, off, 4)
    for f in ("score", "ystart", "yend", "n_ops"):
        assert (rec[f] == wide[f]).all()
    assert (rec["status"] == 0).all() and (rec["ops_off"] == 0).all()
