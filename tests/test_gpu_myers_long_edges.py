"""The block-based Myers kernels (csrc/myers_long.hip) at the smallest shapes where they can go wrong, every call of both
flavours byte for byte against the restatement at w = 64 (tests/myers_long_oracle.py): carries between blocks, the
reference's Ukkonen band (which the kernels do not keep) at its thresholds, every move of the traceback at a block boundary,
ties, hit slots, pattern groups, sub-batches, operation slots that are too small between guard bytes, misaligned text
between guard copies of the pattern, ambiguity codes and a text wildcard."""
import random

import numpy as np
import pytest
import torch

import myers_cases as mc
import myers_long_oracle as ml
from myers_cases import DEV, dev, dna, same_best
from myers_long_cases import check_all, pair
from rust_bio_amd import _lib, myers

pytestmark = pytest.mark.gpu
OPS_CAP = -9


def other(c):
    return ord("T") if c != ord("T") else ord("A")


def test_carries_between_blocks():
    """runs of matches over pattern symbols 60 .. 68 and 124 .. 132 between mismatches; an all-match block 0 whose add in xh
    overflows while -1 enters block 1 (a self-match, and a one-letter pattern in a one-letter text); +1 into every block in
    every column (no symbol of the pattern occurs)"""
    rng = random.Random(60)
    m = 140
    pattern = dna(rng, m, b"ACG")
    run1 = b"T" * 60 + pattern[60:69] + b"T" * (m - 69)
    run2 = b"T" * 124 + pattern[124:133] + b"T" * (m - 133)
    texts = [run1, b"TT" + run2 + b"T", pattern, b"GG" + pattern + pattern[:70], pattern[:63] + pattern[65:], b"T" * 100,
             b"A" * 200, pattern[64:] + pattern[:64]]
    pairs = [pair(pattern), pair(b"A" * 130), pair(b"T" * 129)]
    for k in (0, 5, 131, 10 ** 6):
        best = check_all(pairs, texts, k)
    assert int(best["score"][2 * 3]) == 0 and int(best["score"][5 * 3]) == m  # the self-match; nothing matches
    assert int(best["score"][6 * 3 + 1]) == 0 and int(best["yend"][6 * 3 + 1]) == 130


BAND_M = 200


@pytest.fixture(scope="module")
def band_case():
    rng = random.Random(200)
    pattern = dna(rng, BAND_M, b"ACG")
    shorter_p = b"CGGGGTGTGCACGCGTGGGTCCTGAGGGAGCTCGTCGGTGTGGGGTTCGGGGGGGTTTGT"  # common_tests.rs:270-278
    shorter_t = b"CCACGCGTGGGTCCTGAGGGAGCTCGTCGGTGTGGGGTTCGGGGGGGTTTGT"
    pad = dna(rng, 70)
    texts = [pattern[:150] + b"T" * 40 + pattern[150:],                 # 150 symbols match, 40 columns diverge, the rest matches
             pattern[:60] + b"T" * 20 + pattern[:150] + pattern[151:],   # a false start, then the pattern one symbol short
             dna(rng, 20) + pattern + dna(rng, 20),
             pattern[:64] + bytes([other(pattern[64])]) + pattern[65:130] + pattern[133:],
             pattern[5:120],                                             # shorter than the pattern
             b"", shorter_t + pad]
    return [pair(pattern), pair(shorter_p + pad)], texts


@pytest.mark.parametrize("k", [0, 1, 3, 63, 64, 65, 200, 10 ** 6])
def test_band_thresholds(band_case, k):
    """max_dist around the multiples of 64 at which the reference's band starts with one more block (long.rs:206) and drops
    blocks (long.rs:263); the kernels compute all four blocks and must report what the band reports"""
    pairs, texts = band_case
    best = check_all(pairs, texts, k, max_hits=3)
    if k >= 8:
        assert (int(best["ystart"][6 * 2 + 1]), int(best["yend"][6 * 2 + 1]), int(best["score"][6 * 2 + 1])) == (0, 52 + 70, 8)
    if k >= 4:
        assert int(best["score"][3 * 2]) == 4


@pytest.mark.parametrize("row", [63, 64, 65])
def test_traceback_moves_at_a_block_boundary(row):
    rng = random.Random(row)
    m = 100
    pattern = dna(rng, m, b"ACG")
    texts = [pattern[:row - 1] + pattern[row + 2:],                          # Ins: three pattern symbols around `row` are absent
             pattern[:row] + b"TTT" + pattern[row:],                         # Del: three extra text bytes before `row`
             pattern[:row] + bytes([other(pattern[row])]) + pattern[row + 1:],  # Subst at `row`
             pattern[:row] + pattern[row + 1:],                              # one Ins exactly at `row`
             pattern[:row] + b"T" + pattern[row:],                           # one Del
             pattern[40:] + b"TTTTT",                                        # the best end within the first m columns
             pattern[row:]]                                                  # ... with the path's Ins run ending at the boundary
    want = ml.MyersLong(pattern)
    paths = [ml.best_hit(want, t, 6) for t in texts[:5]]
    assert [sorted(set(p[3])) for p in paths] == [[ml.MATCH, ml.INS], [ml.MATCH, ml.DEL], [ml.MATCH, ml.SUBST], [ml.MATCH, ml.INS],
                                                  [ml.MATCH, ml.DEL]]
    assert paths[2][3][row] == ml.SUBST and paths[3][3][row] == ml.INS and paths[1][3][row:row + 3] == [ml.DEL] * 3
    for k in (6, 45, m):
        best = check_all([pair(pattern)], texts, k)
    assert (int(best["ystart"][5]), int(best["yend"][5]), int(best["score"][5])) == (0, 60, 40)


def test_equal_best_distances_take_the_first_end():
    rng = random.Random(9)
    pattern = dna(rng, 70, b"ACG")
    one_off = pattern[:30] + pattern[31:]
    texts = [b"TT" + pattern + b"TTT" + pattern + b"T" + pattern, b"TT" + one_off + b"TTT" + one_off, pattern[:-1] + b"TT" + pattern[:-1]]
    best = check_all([pair(pattern)], texts, 2, max_hits=4)
    assert (int(best["yend"][0]), int(best["score"][0])) == (72, 0)
    assert (int(best["yend"][1]), int(best["score"][1])) == (71, 1)


@pytest.mark.parametrize("max_hits", [1, 4])
def test_hit_slots(max_hits):
    """jobs with no hit, exactly max_hits hits and (at max_dist 2, where every copy has several ends) more: count is the
    total, the slots hold the first hits in text order"""
    rng = random.Random(max_hits)
    pattern = dna(rng, 66, b"ACG")
    texts = [b"T" * 80, b"TT".join([pattern] * max_hits), b"", pattern]
    want = ml.MyersLong(pattern)
    assert [len(want.find_all_end(t, 0)) for t in texts] == [0, max_hits, 0, 1]
    check_all([pair(pattern)], texts, 0, max_hits=max_hits)
    assert len(want.find_all_end(texts[1], 2)) > max_hits and len(want.find_all_end(texts[3], 2)) > 1
    check_all([pair(pattern)], texts, 2, max_hits=max_hits)


@pytest.fixture()
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n_pat", [1, 3, 30])
def test_pattern_counts_and_lds_groups(ctx, n_pat):
    """patterns over 20 symbols (21 byte classes: 168 bytes of LDS per block) of one to three blocks with the table budget
    lowered to 4 KB: 30 patterns have some 60 blocks, the call runs several groups, cut where the block count's
    instantiation changes as well"""
    rng = random.Random(n_pat)
    alphabet = bytes(range(65, 85))
    patterns = [dna(rng, [70, 130, 20, 129, 64, 65][i % 6], alphabet) for i in range(n_pat)]
    texts = [dna(rng, rng.randint(0, 60), alphabet) for _ in range(10)]
    for i, p in enumerate(patterns[:10]):  # a text each with a copy of the pattern that lacks its middle symbol
        texts[i] = texts[i][:10] + p[:len(p) // 2] + p[len(p) // 2 + 1:] + texts[i][10:]
    ctx.set_option("myers_lds_bytes", 4096)
    check_all([pair(p) for p in patterns], texts, 3, max_hits=2, ctx=ctx)


@pytest.mark.parametrize("n_texts", [1, 63, 64, 65, 257])
def test_text_counts_with_empty_texts_and_sub_batches(ctx, n_texts):
    """wavefront and block boundaries in the number of texts, empty texts in the middle; launches cut at 256 jobs"""
    rng = random.Random(n_texts)
    pattern = dna(rng, 70)
    texts = []
    for _ in range(n_texts):
        t = dna(rng, rng.randint(0, 30))
        if rng.random() < 0.6:
            at = rng.randint(0, len(t))
            t = t[:at] + mc.mutated(rng, pattern, b"ACGT", 0.05) + t[at:]
        texts.append(t)
    for i in range(n_texts // 2, n_texts, 7):
        texts[i] = b""
    ctx.set_option("myers_chunk_jobs", 256)
    check_all([pair(pattern)], texts, 4, max_hits=2, ctx=ctx)


def test_operation_slots_too_small_between_guard_bytes():
    """ops_stride = m + 1: a path with two or more deleted text bytes does not fit.  BG_ERR_OPS_CAP from the call and in the
    job's record with its exact n_ops, the other jobs answered in full, and no byte written outside the slots"""
    rng = random.Random(3)
    pattern = dna(rng, 70, b"ACG")
    m, stride, full = 70, 71, 140
    texts = [pattern, pattern[:64] + b"TT" + pattern[64:], pattern[:40] + b"T" + pattern[40:], pattern[:6] + b"TTT" + pattern[6:], b"TTTT",
             pattern[1:]]
    my, want = pair(pattern)
    wide, wops = ml.best_records([want], texts, 4, full)
    assert [int(n) for n in wide["n_ops"]] == [m, m + 2, m + 1, m + 3, 0, m]
    buf, off = _lib.concat(texts)
    with pytest.raises(_lib.BiogpuError) as e:
        myers.long_best_batch([my], buf, off, 4, ops_stride=stride)
    assert e.value.status == OPS_CAP
    guard = 64
    d_all = torch.full((2 * guard + len(texts) * stride,), 0xEE, dtype=torch.uint8, device=DEV)
    d_aln = torch.zeros(len(texts) * 64, dtype=torch.uint8, device=DEV)
    myers.long_best_batch_dev([my], dev(buf), dev(off, np.int64), 4, ops_stride=stride, stream=torch.cuda.current_stream().cuda_stream,
                              allow_ops_cap=True, out=(d_aln, d_all[guard:guard + len(texts) * stride]))
    torch.cuda.synchronize()
    everything = d_all.cpu().numpy()
    assert (everything[:guard] == 0xEE).all() and (everything[-guard:] == 0xEE).all()
    assert (everything[guard + 4 * stride:guard + 5 * stride] == 0xEE).all()  # the job without a hit wrote nothing
    for rec, ops in (myers.long_best_batch([my], buf, off, 4, ops_stride=stride, allow_ops_cap=True),
                     (myers.records(d_aln), everything[guard:-guard])):
        for j in range(len(texts)):
            w = wide[j].copy()
            n = int(w["n_ops"])
            if n > stride:
                w["status"], w["ops_off"] = OPS_CAP, j * stride
            elif n:
                w["ops_off"] = (j + 1) * stride - n
                assert ops[(j + 1) * stride - n:(j + 1) * stride].tobytes() == wops[(j + 1) * full - n:(j + 1) * full].tobytes(), j
            assert rec[j].tobytes() == w.tobytes(), j
    rec, _ = myers.long_best_batch([my], buf, off, 4)  # without an operations buffer nothing can overflow
    for f in ("score", "ystart", "yend", "n_ops"):
        assert (rec[f] == wide[f]).all()
    assert (rec["status"] == 0).all() and (rec["ops_off"] == 0).all()


@pytest.mark.parametrize("delta", [1, 3, 7])
def test_misaligned_text_between_guard_copies(delta):
    """the text starts `delta` bytes past an 8-byte boundary; copies of the pattern lie directly before and behind it, so
    that a kernel that reads a byte outside [off[0], off[n]) reports a hit the restatement does not have"""
    rng = random.Random(delta)
    pattern = dna(rng, 70, b"ACG")
    (my, want), k = pair(pattern), 2
    texts = [dna(rng, n, b"TTAC") for n in (75, 9, 0, 16, 23, 8, 1, 90)]
    texts[0] = pattern[3:] + b"TTTTT"             # continues a guard copy that ends where the text begins
    texts[-1] = texts[-1][:-40] + pattern[:40]    # ... and is continued by the guard behind
    texts[3] = pattern[:30] + pattern[31:]        # a real hit in between
    body = b"".join(texts)
    lead = pattern + b"G" * ((delta - len(pattern) - 3) % 8) + pattern[:3]
    guard = pattern[40:] + pattern
    assert len(lead) % 8 == delta
    d_buf = dev(np.frombuffer(lead + body + guard, np.uint8))
    assert d_buf.data_ptr() % 8 == 0
    off = np.zeros(len(texts) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t) for t in texts])
    wrec, wops = ml.best_records([want], texts, k, 140)
    assert (wrec["score"] != ml.MIN_SCORE).sum() == 1
    wall = ml.find_all_records([want], texts, k, 4, False)
    wends = ml.find_all_records([want], texts, k, 4, True)
    stream = torch.cuda.current_stream().cuda_stream
    for d_text, shift in ((d_buf[len(lead):], 0), (d_buf, len(lead))):
        assert (d_text.data_ptr() + shift) % 8 == delta
        d_off = dev(off + shift, np.int64)
        d_aln, d_ops = myers.long_best_batch_dev([my], d_text, d_off, k, ops_stride=140, stream=stream)
        same_best((myers.records(d_aln), d_ops.cpu().numpy()), (wrec, wops), 140)
        d_aln, d_count = myers.long_find_all_batch_dev([my], d_text, d_off, k, 4, stream=stream)
        assert myers.records(d_aln).tobytes() == wall[0].tobytes() and (d_count.cpu().numpy() == wall[1]).all()
        d_aln, d_count = myers.long_find_all_batch_dev([my], d_text, d_off, k, 4, True, stream=stream)
        assert myers.records(d_aln).tobytes() == wends[0].tobytes() and (d_count.cpu().numpy() == wends[1]).all()
    host = np.frombuffer(lead + body + guard, np.uint8)
    same_best(myers.long_best_batch([my], host, (off + len(lead)).astype(np.uint64), k, ops_stride=140), (wrec, wops), 140)


def test_ambiguity_codes_and_a_text_wildcard():
    """test_ambig (common_tests.rs:281-296) stretched to 70 symbols: R in the pattern takes A and G of the text, R in the text
    only R; N in the text is a wildcard for one of the patterns"""
    ambigs = {ord("R"): list(b"AG")}
    pattern, text = (b"TRRRCGTR" * 9)[:70], (b"TGATCRTR" * 9)[:70]
    pairs = [pair(pattern, ambigs), pair(pattern, ambigs, [ord("N")]), pair(pattern)]
    texts = [text, b"GG" + text + b"C", text[:64] + b"N" + text[65:], b"N" * 75, pattern, text[:33] + text[34:], b""]
    for k in (0, 18, 70):
        best = check_all(pairs, texts, k)
    assert int(best["score"][0]) == 2 * 8 + 2 and int(best["score"][3 * 3 + 1]) == 0  # two per period; all wildcards
