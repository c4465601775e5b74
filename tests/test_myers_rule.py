"""Myers<u64> on the CPU: the Python restatement (tests/myers_oracle.py) against the reference's known answers and
against a plain O(mn) DP with a path-consistency check, the mirror's peq builder against simple.rs:55-74, the argument
checks of the host entry points that return before a device is touched, and the trim rule on hand cases."""
import random

import numpy as np
import pytest

import myers_cases as mc
import myers_oracle as mo
from rust_bio_amd import _lib, myers


@pytest.mark.parametrize("case", mc.KATS, ids=lambda c: c["name"])
def test_restatement_gives_the_reference_answers(case):
    my, text, k = mc.restatement(case), case["text"].encode(), mc.k_of(case)
    full = my.find_all(text, k)
    mc.check_case(case, my.distance(text), my.find_all_end(text, k), [h[:3] for h in full], {i: h[3] for i, h in enumerate(full)},
                  mo.best_hit(my, text, k))
    if "best_end" in case:
        assert list(my.find_best_end(text)) == case["best_end"]


def test_restatement_panics_where_the_reference_does():
    with pytest.raises(ValueError, match="empty"):
        mo.Myers(b"")
    with pytest.raises(ValueError, match="too long"):
        mo.Myers(b"A" * 65)
    with pytest.raises(ValueError):
        mo.Myers(b"ACGT").find_best_end(b"")
    assert mo.Myers(b"ACGT").distance(b"") == 255  # myers_impl.rs:168-180: the loop never runs


@pytest.mark.parametrize("m", [1, 2, 5, 13, 31, 32, 33, 63, 64])
def test_restatement_against_the_plain_dp(m):
    rng = random.Random(1000 + m)
    tracebacks = 0
    for _ in range(40):
        pattern, text = mc.random_case(rng, m)
        my = mo.Myers(pattern)
        k = rng.choice([0, 1, 2, m // 2, m, 255])
        want = mo.dp_columns(my.peq, m, text)
        assert [d for _, d in my.find_all_end(text, 255)] == want  # every column's distance
        hits = my.find_all(text, k)
        assert [(e - 1, d) for _, e, d, _ in hits] == [(i, d) for i, d in enumerate(want) if d <= min(k, 255)]
        for start, end, dist, ops in hits:
            mo.check_path(my.peq, m, text, start, end, dist, ops)
            tracebacks += 1
    assert tracebacks > 40


def test_mirror_builds_peq_as_new_ambig_does():
    b = myers.MyersBuilder().ambig(b"R", b"A").ambig(b"R", b"G").text_wildcard(b"N")  # a repeated ambig accumulates
    my = b.build_64(b"TRRA")
    peq = [int(v) for v in my.peq]
    assert my.m == 4
    assert peq[ord("T")] == 0b0001
    assert peq[ord("R")] == 0b0110  # the symbol's own bit ...
    assert peq[ord("G")] == 0b0110  # ... and its equivalents'
    assert peq[ord("A")] == 0b1110
    assert peq[ord("N")] == (1 << 64) - 1  # a wildcard is all ones (T::max_value(), above bit m too)
    assert peq[ord("C")] == 0
    want, _ = mo.build_peq(b"TRRA", {ord("R"): list(b"AG")}, [ord("N")])
    assert peq == want
    plain = myers.Myers(b"ACCA")
    assert [int(plain.peq[c]) for c in b"ACGT"] == [0b1001, 0b0110, 0, 0]
    with pytest.raises(ValueError, match="empty"):
        myers.Myers(b"")
    with pytest.raises(ValueError, match="too long"):
        myers.MyersBuilder().build_64(b"A" * 65)


def _raw_patterns(ms):
    a = np.zeros(len(ms), dtype=_lib.MYERS_PATTERN_DTYPE)
    a["m"] = ms
    a["peq"][:, ord("A")] = 1
    return a


def test_host_entry_points_check_their_arguments_before_any_device():
    L = _lib.lib()
    text, off = np.frombuffer(b"ACGT", dtype=np.uint8), np.array([0, 4], dtype=np.uint64)
    aln, cnt = np.zeros(1100 * 4, dtype=_lib.ALN_DTYPE), np.zeros(1100, dtype=np.uint32)

    def best(pats, n_pat):
        return L.bg_myers_best_batch(None, pats.ctypes.data, n_pat, 1, 1, text.ctypes.data, off.ctypes.data, aln.ctypes.data, None, 0)

    def find_all(pats, n_pat, max_hits, flags=0):
        return L.bg_myers_find_all_batch(None, pats.ctypes.data, n_pat, 1, max_hits, flags, 1, text.ctypes.data, off.ctypes.data,
                                         aln.ctypes.data, cnt.ctypes.data)

    one = _raw_patterns([4])
    assert best(_raw_patterns([0]), 1) == -1 and find_all(_raw_patterns([0]), 1, 1) == -1      # "Pattern is empty"
    assert best(_raw_patterns([65]), 1) == -8 and find_all(_raw_patterns([65]), 1, 1) == -8    # "Pattern too long"
    assert best(_raw_patterns([4, 65, 0]), 3) == -8                                            # the first offender decides
    assert best(one, 0) == -1 and find_all(one, 0, 1) == -1
    many = _raw_patterns([4] * 1025)
    assert best(many, 1025) == -8 and find_all(many, 1025, 1) == -8
    assert find_all(one, 1, 0) == -1 and find_all(one, 1, 65) == -1
    assert find_all(one, 1, 1, flags=2) == -1                                                     # an unknown flag
    # legal arguments get as far as the missing ctx
    assert best(one, 1) == -1 and best(_raw_patterns([64]), 1) == -1 and best(many, 1024) == -1
    assert find_all(one, 1, 64) == -1
    assert L.bg_fastq_trim(None, 0, 2, None, 1, *[None] * 11) == -1                            # an unknown trim mode
    assert L.bg_fastq_trim(None, 0, 0, None, 1025, *[None] * 11) == -8


def _trim(mode, hits, seq, qual):
    (lo, hi), (qlo, qhi) = mo.trim_range(mode, hits, len(seq), len(qual))
    return seq[lo:hi], qual[qlo:qhi]


def test_trim_rule_on_hand_cases():
    none = (mo.MIN_SCORE, 0, 0)
    seq, qual = b"ACGTACGTAC", b"IIIIIHHHHH"
    assert _trim(mo.TRIM_3P, [none, none], seq, qual) == (seq, qual)                        # no hit: the read stays whole
    assert _trim(mo.TRIM_5P, [none], seq, qual) == (seq, qual)
    assert _trim(mo.TRIM_3P, [(1, 6, 9), (0, 4, 7), none], seq, qual) == (b"ACGT", b"IIII")  # several patterns: the smallest start
    assert _trim(mo.TRIM_5P, [(1, 0, 3), (0, 1, 5), none], seq, qual) == (b"CGTAC", b"HHHHH")  # ... the largest end
    assert _trim(mo.TRIM_3P, [(0, 0, 4)], seq, qual) == (b"", b"")                           # a hit at column 0: an empty record
    assert _trim(mo.TRIM_5P, [(0, 6, 10)], seq, qual) == (b"", b"")
    assert _trim(mo.TRIM_3P, [(0, 8, 10)], seq, b"IIIII") == (b"ACGTACGT", b"IIIII")         # qualities shorter than the sequence
    assert _trim(mo.TRIM_3P, [(0, 3, 10)], seq, b"IIIII") == (b"ACG", b"III")
    assert _trim(mo.TRIM_5P, [(0, 0, 7)], seq, b"IIIII") == (b"TAC", b"")
    assert _trim(mo.TRIM_5P, [(0, 0, 2)], seq, b"IIIII") == (seq[2:], b"III")
    assert _trim(mo.TRIM_3P, [(0, 12, 14)], seq, qual) == (seq, qual)                        # clamped to the read
