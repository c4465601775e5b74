"""myers::long on the CPU: the Python restatement (tests/myers_long_oracle.py) at w = 8 (what the reference's own tests
run) and w = 64 (what the device implements) against the reference's known answers (tests/golden/myers_long_kats.json) and
against a plain O(mn) DP with a path-consistency check — ends, distances and, under the band's barrier blocks, paths; the
restatement with its Ukkonen band against itself with every block in every column (the device computes all blocks); the
mirror's peq builder against long.rs:86-115; and the argument checks of the host entry points that return before a device is
touched.

The restatement is the definition: had it ever disagreed with the DP, the case would stand here as a known answer and the
device would follow the restatement.  It has not, in these cases or in 27 000 more drawn the same way."""
import random

import numpy as np
import pytest

import myers_cases as mc
import myers_long_oracle as ml
import myers_oracle as mo
from myers_long_cases import KATS
from rust_bio_amd import _lib, myers


@pytest.mark.parametrize("w", [8, 64])
@pytest.mark.parametrize("case", KATS, ids=lambda c: c["name"])
def test_restatement_gives_the_reference_answers(case, w):
    my, text = ml.MyersLong(*mc.pattern_args(case), w=w), case["text"].encode()
    k = case.get("k", ml.USIZE)
    full = my.find_all(text, k)
    mc.check_case(case, my.distance(text), my.find_all_end(text, k), [h[:3] for h in full], {i: h[3] for i, h in enumerate(full)},
                  ml.best_hit(my, text, k))
    if "best_end" in case:
        assert list(my.find_best_end(text)) == case["best_end"]


def test_overflow_case_is_two_full_blocks_and_has_every_column():
    case = next(c for c in KATS if c["name"] == "test_myers_long_overflow")
    assert len(case["pattern"]) == 128 and len(case["find_all_end"]) == len(case["text"])
    my = ml.MyersLong(case["pattern"].encode())
    assert len(my.peq) == 2 and my.peq[1].high_mask == 1 << 63
    assert [d for _, d in case["find_all_end"]] == mo.dp_columns(my.full_peq(), my.m, case["text"].encode())


@pytest.mark.parametrize("w", [8, 64])
def test_restatement_panics_where_the_reference_does(w):
    with pytest.raises(ValueError, match="empty"):
        ml.MyersLong(b"", w=w)
    with pytest.raises(ValueError):
        ml.MyersLong(b"ACGT", w=w).find_best_end(b"")
    assert ml.MyersLong(b"ACGT" * 20, w=w).distance(b"") == (1 << 64) - 1 - w  # myers_impl.rs:168-180 with long.rs:586


def _cases(w, base, n):
    """seeded (m, k, pattern, text): m around w, 2w, 3w, k from 0 to m + 5, texts shorter and longer than the pattern"""
    rng = random.Random(base)
    for i in range(n):
        m = [w, 2 * w, 3 * w][i % 3] + [-1, 0, 1][(i // 3) % 3]
        alpha = rng.choice([b"ACGT", b"ACGT", b"AC", bytes(range(65, 85))])
        pattern, text = mc.random_case(rng, m, alpha, max_text=rng.choice([m // 2 + 1, m + 10, 3 * m]))
        yield m, rng.randint(0, m + 5), pattern, text


@pytest.mark.parametrize("w, n", [(8, 360), (64, 72)])
def test_restatement_against_the_plain_dp_and_without_its_band(w, n):
    tracebacks = banded = 0
    for m, k, pattern, text in _cases(w, 2000 + w, n):
        my = ml.MyersLong(pattern, w=w)
        peq = my.full_peq()
        want = mo.dp_columns(peq, m, text)
        assert my.find_all_end(text, k) == [(i, d) for i, d in enumerate(want) if d <= k], (pattern, text, k)
        assert my.distance(text) == (min(want) if want else ml.USIZE - w)
        hits = my.find_all(text, k)
        assert [(e - 1, d) for _, e, d, _ in hits] == [(i, d) for i, d in enumerate(want) if d <= k]
        for start, end, dist, ops in hits:
            mo.check_path(peq, m, text, start, end, dist, ops)
            tracebacks += 1
        # every block in every column (band >= m: long.rs:206, 263) changes nothing
        assert my.find_all(text, k, band=m) == hits, (pattern, text, k)
        assert my.find_all_end(text, k, band=m) == my.find_all_end(text, k)
        banded += k < m - w and len(hits) > 0
    assert tracebacks > n and banded > n // 10  # hits traced while the band left blocks out


def test_one_block_patterns_are_the_u64_variant():
    rng = random.Random(5)
    for m in (1, 33, 63, 64):
        for _ in range(10):
            pattern, text = mc.random_case(rng, m)
            k = rng.choice([0, 2, m // 2, m, 255])
            assert ml.MyersLong(pattern).find_all(text, k) == mo.Myers(pattern).find_all(text, k)


def test_mirror_builds_peq_as_new_ambig_does():
    b = myers.MyersBuilder().ambig(b"R", b"A").ambig(b"R", b"G").text_wildcard(b"N")
    pattern = b"TRRA" * 17  # 68 symbols: one full block and a chunk of four
    my = b.build_long_64(pattern)
    want, m = ml.build_peq(pattern, {ord("R"): list(b"AG")}, [ord("N")], 64)
    assert my.m == m == 68 and my.peq.shape == (2, 256)
    assert [[int(v) for v in blk] for blk in my.peq] == [p.peq for p in want]
    assert int(my.peq[1][ord("T")]) == 0b0001 and int(my.peq[1][ord("A")]) == 0b1110
    assert int(my.peq[1][ord("N")]) == (1 << 64) - 1  # a wildcard is all ones, above the chunk too (long.rs:105-109)
    peq, blk_off, ms = myers.long_patterns_array([my, myers.Myers(b"ACGT"), myers.MyersLong(b"A" * 129)])
    assert list(blk_off) == [0, 2, 3, 6] and list(ms) == [68, 4, 129] and peq.shape == (6 * 256,)
    with pytest.raises(ValueError, match="empty"):
        myers.MyersLong(b"")
    with pytest.raises(ValueError, match="too long"):
        myers.MyersBuilder().build_long_64(b"A" * 1025)
    assert myers.MyersLong(b"A" * 1024).peq.shape == (16, 256)
    assert myers.MyersLong.NO_DISTANCE == (1 << 64) - 1 - 64


def _raw(ms, blk_off=None):
    ms = np.array(ms, dtype=np.uint32)
    if blk_off is None:
        blk_off = np.concatenate([[0], np.cumsum((ms.astype(np.int64) + 63) // 64)])
    blk_off = np.array(blk_off, dtype=np.uint64)
    peq = np.zeros((max(1, int(blk_off.max())) + 17) * 256, dtype=np.uint64)
    return peq, blk_off, ms


def test_host_entry_points_check_their_arguments_before_any_device():
    L = _lib.lib()
    text, off = np.frombuffer(b"ACGT", dtype=np.uint8), np.array([0, 4], dtype=np.uint64)
    aln, cnt = np.zeros(1100 * 4, dtype=_lib.ALN_DTYPE), np.zeros(1100, dtype=np.uint32)

    def best(raw, n_pat=None):
        peq, blk_off, ms = raw
        return L.bg_myers_long_best_batch(None, peq.ctypes.data, blk_off.ctypes.data, ms.ctypes.data, len(ms) if n_pat is None else n_pat, 1,
                                          1, text.ctypes.data, off.ctypes.data, aln.ctypes.data, None, 0)

    def best_dev(raw):
        peq, blk_off, ms = raw
        return L.bg_myers_long_best_batch_dev(None, peq.ctypes.data, blk_off.ctypes.data, ms.ctypes.data, len(ms), 1, 1, None, None, None,
                                              None, 0, None)

    def find_all(raw, max_hits, flags=0, n_pat=None, dev=False):
        peq, blk_off, ms = raw
        n_pat = len(ms) if n_pat is None else n_pat
        if dev:
            return L.bg_myers_long_find_all_batch_dev(None, peq.ctypes.data, blk_off.ctypes.data, ms.ctypes.data, n_pat, 1, max_hits, flags,
                                                      1, None, None, None, None, None)
        return L.bg_myers_long_find_all_batch(None, peq.ctypes.data, blk_off.ctypes.data, ms.ctypes.data, n_pat, 1, max_hits, flags, 1,
                                              text.ctypes.data, off.ctypes.data, aln.ctypes.data, cnt.ctypes.data)

    one = _raw([70])
    for raw, rc in [(_raw([0], [0, 0]), -1),            # "Pattern is empty"
                    (_raw([1025], [0, 17]), -8),        # more than BG_MYERS_LONG_MAX_M
                    (_raw([4, 1025, 0], [0, 1, 18, 18]), -8),  # the first offender decides
                    (_raw([70], [0, 1]), -1),           # two blocks, one declared
                    (_raw([70], [0, 3]), -1),
                    (_raw([70], [1, 3]), -1),           # blk_off[0] != 0
                    (_raw([64, 65], [0, 2, 3]), -1)]:   # the right total, the wrong split
        assert best(raw) == rc and best_dev(raw) == rc, (raw[2], raw[1])
        assert find_all(raw, 1) == rc and find_all(raw, 1, dev=True) == rc, (raw[2], raw[1])
    assert best(one, n_pat=0) == -1 and find_all(one, 1, n_pat=0) == -1
    many = _raw([70] * 1025)
    assert best(many) == -8 and find_all(many, 1) == -8 and best_dev(many) == -8
    for dev in (False, True):
        assert find_all(one, 0, dev=dev) == -1 and find_all(one, 65, dev=dev) == -1
        assert find_all(one, 1, flags=2, dev=dev) == -1  # an unknown flag
    # legal arguments get as far as the missing ctx
    assert best(one) == -1 and best(_raw([1024])) == -1 and best(_raw([1])) == -1 and best(_raw([70] * 1024)) == -1
    assert best(_raw([20, 70, 130, 300])) == -1 and find_all(one, 64) == -1
    assert L.bg_myers_long_best_batch(None, None, None, None, 1, 1, 1, None, None, None, None, 0) == -1
