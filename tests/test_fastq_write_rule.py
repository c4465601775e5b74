"""FASTQ out on the CPU: the Python restatement of `fastq::Writer::write` and of the filter rule (tests/fastq_write_oracle.py)
against the reference's known answers, write-then-parse through the FASTQ oracle, the reason the filter exists (the reader
rejects a record with an empty sequence), and the argument checks of bg_fastq_filter / bg_fastq_emit, which return before a
device is touched and say why (bg_last_error)."""
import ctypes as C
import random

import numpy as np
import pytest

import fastq_write_oracle as fw
import oracle_py as orc
from kat_util import load
from rust_bio_amd import _lib, fastq

KATS = load("fastq_write_kats.json")["writer"]


@pytest.mark.parametrize("case", KATS, ids=lambda c: c["name"].split(" (")[0])
def test_restatement_gives_the_reference_answers(case):
    desc = None if case["desc"] is None else case["desc"].encode()
    assert fw.write(case["id"].encode(), desc, case["seq"].encode(), case["qual"].encode()) == case["text"].encode()


def test_restatement_on_hand_cases():
    assert fw.write(b"id", b"", b"AC", b"II") == b"@id \nAC\n+\nII\n"       # Some(""): the space stays
    assert fw.write(b"", None, b"", b"") == b"@\n\n+\n\n"                    # nothing is checked
    assert fw.write(b"r", None, b"ACGT", b"I") == b"@r\nACGT\n+\nI\n"        # unequal lengths are written as they are


def _random_records(rng, n):
    out = []
    for r in range(n):
        desc = None if rng.random() < 0.4 else b" ".join(bytes(rng.randint(48, 122) for _ in range(rng.randint(1, 9))) for _ in range(rng.randint(1, 3)))
        ln = rng.randint(1, 60)
        out.append((b"r%d" % r, desc, bytes(rng.choice(b"ACGTN") for _ in range(ln)), bytes(rng.randint(33, 73) for _ in range(ln))))
    return out


def test_written_records_parse_back():
    rng = random.Random(7)
    records = _random_records(rng, 200)
    text = b"".join(fw.write(*r) for r in records)
    got, status, _ = orc.fastq_parse(text)
    assert status == "ok"
    assert [(g["id"], g["desc"], g["seq"], g["qual"]) for g in got] == records
    # wrapped multi-line input comes back on one line: parse, write, parse again
    wrapped = b"@id description\nACGT\nGGGG\nC\n+\n@@@@\n!!!!\n$\n@id2\nAC\nG\n+\nII\nI\n"
    first, status, _ = orc.fastq_parse(wrapped)
    assert status == "ok" and [r["seq"] for r in first] == [b"ACGTGGGGC", b"ACG"]
    again = b"".join(fw.write(r["id"], r["desc"], r["seq"], r["qual"]) for r in first)
    assert again == b"@id description\nACGTGGGGC\n+\n@@@@!!!!$\n@id2\nACG\n+\nIII\n"
    second, status, _ = orc.fastq_parse(again)
    assert status == "ok" and second == first


def test_the_reader_rejects_an_empty_record():
    """what bg_fastq_trim leaves of a read that is all adapter cannot be read again: the filter's min_len >= 1 is the remedy"""
    text = fw.write(b"id", None, b"", b"")
    assert text == b"@id\n\n+\n\n"
    recs, status, _ = orc.fastq_parse(text)
    assert (recs, status) == ([], "IncompleteRecord")
    recs, status, _ = orc.fastq_parse(fw.write(b"a", None, b"ACGT", b"IIII") + text)
    assert (len(recs), status) == (1, "IncompleteRecord")


def test_filter_rule_on_hand_cases():
    assert fw.passes(b"ACGT", 0, False) and fw.passes(b"", 5, True)
    assert not fw.passes(b"ACG", 0, False, min_len=4) and fw.passes(b"ACGT", 0, False, min_len=4, max_len=4)
    assert not fw.passes(b"ACGTA", 0, False, max_len=4)
    assert fw.passes(b"ANnA", 0, False, max_n=2) and not fw.passes(b"ANnN", 0, False, max_n=2) and not fw.passes(b"n", 0, False, max_n=0)
    assert not fw.passes(b"A", 5, False, flags=fw.CHECK_OK) and fw.passes(b"A", 0, False, flags=fw.CHECK_OK)
    assert fw.passes(b"A", 0, True, flags=fw.DISCARD_UNTRIMMED) and not fw.passes(b"A", 0, False, flags=fw.DISCARD_UNTRIMMED)
    assert fw.passes(b"A", 0, False, flags=fw.DISCARD_TRIMMED) and not fw.passes(b"A", 0, True, flags=fw.DISCARD_TRIMMED)
    four = [True, True, True, False, False, True, False, False]
    assert fw.keep_flags(four, 0) == four
    assert fw.keep_flags(four, fw.PAIRED) == [True, True, False, False, False, False, False, False]
    assert fw.keep_flags(four, fw.PAIRED | fw.PAIR_BOTH) == [True, True, True, True, True, True, False, False]


def test_entry_points_check_their_arguments_before_any_device():
    L = _lib.lib()
    rec = np.zeros(2, dtype=_lib.FQREC_DTYPE)
    buf, off, hit = np.zeros(8, dtype=np.uint8), np.zeros(3, dtype=np.uint64), np.zeros(2, dtype=_lib.ALN_DTYPE)
    p = lambda a: a.ctypes.data  # noqa: E731

    def flt(n=2, flags=0, min_len=0, max_len=fw.NO_BOUND, max_n=fw.NO_BOUND, hits=None, n_pat=0, null=None, dev=False, no_filter=False):
        f = fastq.filter_params(flags, min_len, max_len, max_n)
        cols = {"recs": p(rec), "seq": p(buf), "seq_off": p(off), "qual": p(buf), "qual_off": p(off), "recs_out": p(rec), "seq_out": p(buf),
                "seq_off_out": p(off), "qual_out": p(buf), "qual_off_out": p(off)}
        if null:
            cols[null] = None
        args = (None, n, None if no_filter else p(f), None if hits is None else p(hits), n_pat, *cols.values(), None, None)
        rc = L.bg_fastq_filter_dev(*args, None) if dev else L.bg_fastq_filter(*args)
        return rc, L.bg_last_error().decode()

    for dev in (False, True):
        assert flt(flags=32, dev=dev) == (-1, "bg_fastq_filter: unknown flag bits")
        assert flt(flags=fw.DISCARD_TRIMMED | fw.DISCARD_UNTRIMMED, hits=hit, n_pat=1, dev=dev) == (-1, "bg_fastq_filter: both DISCARD flags")
        for d in (fw.DISCARD_TRIMMED, fw.DISCARD_UNTRIMMED):
            assert flt(flags=d, hits=None, n_pat=1, dev=dev) == (-1, "bg_fastq_filter: a DISCARD flag without hits")
            assert flt(flags=d, hits=hit, n_pat=0, dev=dev) == (-1, "bg_fastq_filter: a DISCARD flag without hits")
        assert flt(flags=fw.PAIR_BOTH, dev=dev) == (-1, "bg_fastq_filter: PAIR_BOTH without PAIRED")
        assert flt(n=1, flags=fw.PAIRED, dev=dev) == (-1, "bg_fastq_filter: PAIRED with an odd record count")
        assert flt(min_len=5, max_len=4, dev=dev) == (-1, "bg_fastq_filter: min_len above max_len")
        assert flt(flags=fw.DISCARD_TRIMMED, hits=hit, n_pat=1025, dev=dev) == (-8, "bg_fastq_filter: n_pat above BG_MYERS_MAX_PATTERNS")
        assert flt(n_pat=1025, dev=dev)[0] == -8
        assert flt(no_filter=True, dev=dev) == (-1, "bg_fastq_filter: null filter")
        for col in ("recs", "seq", "seq_off", "qual", "qual_off", "recs_out", "seq_out", "qual_out"):
            assert flt(null=col, dev=dev) == (-1, "bg_fastq_filter: null column"), col
            assert flt(n=0, null=col, dev=dev) == (-1, "bg_fastq_filter: null ctx"), col  # no record: not looked at
        for col in ("seq_off_out", "qual_off_out"):
            assert flt(n=0, null=col, dev=dev) == (-1, "bg_fastq_filter: null output offsets"), col
        # legal arguments get as far as the missing ctx
        assert flt(dev=dev) == (-1, "bg_fastq_filter: null ctx")
        assert flt(flags=fw.PAIRED | fw.PAIR_BOTH | fw.CHECK_OK | fw.DISCARD_TRIMMED, min_len=4, max_len=4, max_n=0, hits=hit, n_pat=1024,
                   dev=dev) == (-1, "bg_fastq_filter: null ctx")

    total = C.c_uint64(7)

    def emit(n=2, first=0, step=1, null=None, out=None, cap=0, off_=off, tot=total, dev=False):
        cols = {"text": p(buf), "recs": p(rec), "seq": p(buf), "qual": p(buf)}
        if null:
            cols[null] = None
        args = (None, n, first, step, *cols.values(), out, cap, None if off_ is None else p(off_), None if tot is None else C.byref(tot))
        rc = L.bg_fastq_emit_dev(*args, None) if dev else L.bg_fastq_emit(*args)
        return rc, L.bg_last_error().decode()

    for dev in (False, True):
        assert emit(step=0, dev=dev) == (-1, "bg_fastq_emit: step 0")
        assert emit(off_=None, dev=dev) == (-1, "bg_fastq_emit: null out_off or out_bytes")
        assert emit(tot=None, dev=dev) == (-1, "bg_fastq_emit: null out_off or out_bytes")
        assert emit(cap=16, dev=dev) == (-1, "bg_fastq_emit: null out with a capacity")
        for col in ("text", "recs", "seq", "qual"):
            assert emit(null=col, dev=dev) == (-1, "bg_fastq_emit: null text, recs, seq or qual"), col
            assert emit(first=1, step=2, null=col, dev=dev) == (-1, "bg_fastq_emit: null text, recs, seq or qual"), col
            assert emit(first=2, null=col, dev=dev) == (-1, "bg_fastq_emit: null ctx"), col  # first >= n: no line, not looked at
            assert emit(n=0, null=col, dev=dev) == (-1, "bg_fastq_emit: null ctx"), col
        assert emit(dev=dev) == (-1, "bg_fastq_emit: null ctx") and total.value == 0
        assert emit(out=p(buf), cap=8, dev=dev) == (-1, "bg_fastq_emit: null ctx")


def test_binding_describes_the_filter_struct():
    f = fastq.filter_params(fastq.FQF_PAIRED | fastq.FQF_CHECK_OK, 20, 150, 3)
    assert f.tobytes() == np.array([17, 20, 150, 3], dtype="<u4").tobytes()
    assert fastq.filter_params().tobytes() == np.array([0, 0, 0xFFFFFFFF, 0xFFFFFFFF], dtype="<u4").tobytes()
    assert (fw.PAIRED, fw.PAIR_BOTH, fw.DISCARD_UNTRIMMED, fw.DISCARD_TRIMMED, fw.CHECK_OK) == (
        _lib.FQF_PAIRED, _lib.FQF_PAIR_BOTH, _lib.FQF_DISCARD_UNTRIMMED, _lib.FQF_DISCARD_TRIMMED, _lib.FQF_CHECK_OK)
    assert [fastq.n_lines(n, f, s) for n, f, s in [(0, 0, 1), (5, 0, 1), (5, 0, 2), (5, 1, 2), (4, 1, 2), (5, 5, 1), (5, 9, 2), (5, 4, 7)]] == [0, 5, 3, 2, 2, 0, 0, 1]
