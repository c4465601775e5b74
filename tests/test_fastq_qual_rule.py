"""The quality rules on the CPU: the Python restatement of include/biogpu.h's three rules (tests/fastq_qual_oracle.py) on hand
cases a reader can check by eye, the composition cut -> trim 3' -> trim 5' against direct slicing, the argument checks of the
six entry points, which return before a device is touched and say why (bg_last_error), the binding's view of the three structs
and bg_qc_tables_words."""
import os
import random
import re

import numpy as np

import fastq_qual_oracle as qo
from fastq_qual_cases import CUTOFF, PHRED, random_records
from rust_bio_amd import _lib, fastq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_runsum_hand_cases():
    both = dict(method_5p=qo.RUNSUM, method_3p=qo.RUNSUM, cutoff_5p=10, cutoff_3p=10)
    assert qo.cut_points([40, 40, 40, 2, 2, 40, 2, 2], **both) == (0, 6)
    assert qo.cut_points([2, 2, 40, 2, 2], **both) == (2, 3)
    assert qo.cut_points([2, 2, 2], **both) == (3, 3)
    rec = qo.cut_record(3, 3, 3)
    assert (int(rec["score"]), int(rec["ystart"]), int(rec["yend"]), int(rec["ylen"])) == (3, 3, 3, 3)
    for q in ([10, 10, 10], [40, 9, 11], []):
        b, e = qo.cut_points(q, **both)
        rec = qo.cut_record(len(q), b, e)
        assert (b, e) == (0, len(q)) and int(rec["score"]) == qo.MIN_SCORE and int(rec["ylen"]) == len(q)
        assert rec.tobytes()[4:24] == bytes(20) and rec.tobytes()[28:] == bytes(36)
    # the record of a cut: score is what is removed, ystart = e >= yend = b
    rec = qo.cut_record(8, 0, 6)
    assert (int(rec["score"]), int(rec["ystart"]), int(rec["yend"]), int(rec["ylen"]), int(rec["mode"])) == (2, 6, 0, 8, 0)
    # a maximum reached twice: the first one (the shorter cut) stays
    assert qo.cut_points([40, 40, 2, 18, 2], method_3p=qo.RUNSUM, cutoff_3p=10) == (0, 4)
    assert qo.cut_points([2, 18, 2, 40], method_5p=qo.RUNSUM, method_3p=qo.NONE, cutoff_5p=10) == (1, 4)
    # both methods NONE
    assert qo.cut_points([0, 0], method_5p=qo.NONE, method_3p=qo.NONE) == (0, 2)


def test_window_hand_cases():
    for q, window, e in [([30, 30, 30, 30, 5, 30, 5, 5], 4, 3), ([30, 5, 30], 4, 3), ([30, 30, 5, 5, 30, 30], 2, 1), ([5, 30, 30], 2, 0),
                         ([30, 30, 30, 5], 2, 2), ([30, 30, 30, 30, 5], 4, 5)]:
        assert qo.cut_points(q, method_3p=qo.WINDOW, cutoff_3p=20, window=window) == (0, e), (q, window)
    # e < b becomes e = b
    assert qo.cut_points([5, 5, 30, 30], method_5p=qo.RUNSUM, method_3p=qo.WINDOW, cutoff_5p=20, cutoff_3p=20, window=2) == (2, 2)


def test_select_and_tables_hand_cases():
    raw = bytes([PHRED + 30, PHRED + 10, PHRED - 3, PHRED + 20])
    s = qo.stats_of(raw, PHRED, low_q=20, weight=qo.ee_weights(PHRED))
    assert (s["sum_q"], s["len"], s["n_low"], s["min_q"]) == (60, 4, 2, 0)
    assert s["weight_sum"] == round(2 ** 20 / 1000) + round(2 ** 20 / 10) + 2 ** 20 + round(2 ** 20 / 100)
    assert qo.passes(s, min_mean_q=15) and not qo.passes(s, min_mean_q=16)
    assert qo.passes(s, max_low_pct=50) and not qo.passes(s, max_low_pct=49) and qo.passes(s, max_low_pct=100) and qo.passes(s, max_low_pct=101)
    assert qo.passes(s, max_weight=s["weight_sum"], has_weight=True) and not qo.passes(s, max_weight=s["weight_sum"] - 1, has_weight=True)
    empty = qo.stats_of(b"", PHRED, 20)
    assert empty["min_q"] == 0 and qo.passes(empty, min_mean_q=40, max_low_pct=0)
    # pairs: one verdict for both mates
    qual, off = bytes([PHRED + 30, PHRED + 5]), [0, 1, 2]
    assert list(qo.select(qual, off, min_mean_q=20)[1]) == [0, 1]
    assert list(qo.select(qual, off, flags=qo.PAIRED, min_mean_q=20)[1]) == [1, 1]
    assert list(qo.select(qual, off, flags=qo.PAIRED | qo.PAIR_BOTH, min_mean_q=20)[1]) == [0, 0]
    # tables: two reads, max_cycles 2, so row 2 collects positions 2 and 3
    _, t = qo.tables(b"ACgNT", [0, 4, 5], bytes([PHRED + 1, PHRED + 2, PHRED + 70, PHRED - 1, PHRED + 2]), [0, 4, 5], 2)
    assert t["base"].tolist() == [[1, 0, 0, 1, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 1]]
    assert [(r, v, int(c)) for r in range(3) for v, c in enumerate(t["qhist"][r]) if c] == [(0, 1, 1), (0, 2, 1), (1, 2, 1), (2, 0, 1), (2, 63, 1)]
    assert t["len_hist"].tolist() == [0, 1, 0, 1] and int(t["n_reads"][0]) == 2
    assert [(v, int(c)) for v, c in enumerate(t["meanq_hist"]) if c] == [(2, 1), (18, 1)]


def test_cut_then_trim_3p_then_trim_5p_is_the_slice():
    rng = random.Random(3)
    records = random_records(rng, 300, equal=1.0)
    quals = b"".join(r[3] for r in records)
    off = np.cumsum([0] + [len(r[3]) for r in records])
    seen = {}
    cut, _, points = qo.cut(quals, off, PHRED, events=seen, method_5p=qo.RUNSUM, method_3p=qo.RUNSUM, cutoff_5p=CUTOFF, cutoff_3p=CUTOFF)
    got = qo.trimmed(records, cut)
    assert got == [(i, d, s[b:e], q[b:e]) for (i, d, s, q), (b, e) in zip(records, points)]
    assert min(seen[k] for k in ("no-hit", "3p", "5p", "both", "nothing left")) >= 5, seen
    # unequal lengths: the trim's clamping — the sequence keeps [b, e) as far as it reaches, the qualities what lies inside that
    assert qo.trimmed([(b"x", None, b"ACGTAC", b"IIII")], [qo.cut_record(4, 1, 3)]) == [(b"x", None, b"CG", b"II")]
    assert qo.trimmed([(b"x", None, b"AC", b"IIIII")], [qo.cut_record(5, 1, 4)]) == [(b"x", None, b"C", b"I")]


def test_entry_points_check_their_arguments_before_any_device():
    L = _lib.lib()
    p = lambda a: a.ctypes.data  # noqa: E731
    buf, off, cut = np.zeros(8, dtype=np.uint8), np.zeros(3, dtype=np.uint64), np.zeros(2, dtype=_lib.ALN_DTYPE)
    stats, bins = np.zeros(2, dtype=_lib.QUAL_STATS_DTYPE), np.zeros(2, dtype=np.uint32)
    weight, tab = np.zeros(256, dtype=np.uint32), np.zeros(fastq.qc_tables_words(1024), dtype=np.uint64)

    what = "bg_fastq_qual_cut: "

    def do_cut(n=2, null=None, no_params=False, dev=False, **kw):
        prm = fastq.qual_cut_params(**kw)
        cols = {"qual": p(buf), "qual_off": p(off), "cut_out": p(cut)}
        if null:
            cols[null] = None
        args = (None, n, None if no_params else p(prm), *cols.values(), None)
        rc = L.bg_fastq_qual_cut_dev(*args, None) if dev else L.bg_fastq_qual_cut(*args)
        return rc, L.bg_last_error().decode()

    for dev in (False, True):
        assert do_cut(no_params=True, dev=dev) == (-1, what + "null params")
        assert do_cut(method_5p=3, dev=dev) == (-1, what + "unknown method")
        assert do_cut(method_3p=3, dev=dev) == (-1, what + "unknown method")
        assert do_cut(method_5p=qo.WINDOW, window=4, dev=dev) == (-1, what + "WINDOW as method_5p")
        assert do_cut(method_3p=qo.WINDOW, window=0, dev=dev) == (-1, what + "window 0 with WINDOW")
        assert do_cut(phred_offset=256, dev=dev) == (-1, what + "phred_offset above 255")
        assert do_cut(null="qual_off", dev=dev) == (-1, what + "null qual_off")
        assert do_cut(n=0, null="qual_off", dev=dev) == (-1, what + "null qual_off")
        for col in ("qual", "cut_out"):
            assert do_cut(null=col, dev=dev) == (-1, what + "null qual or cut_out"), col
            assert do_cut(n=0, null=col, dev=dev) == (-1, what + "null ctx"), col  # no record: not looked at
        # legal arguments get as far as the missing ctx
        assert do_cut(dev=dev) == (-1, what + "null ctx")
        assert do_cut(method_5p=qo.NONE, method_3p=qo.NONE, dev=dev) == (-1, what + "null ctx")
        assert do_cut(method_5p=qo.RUNSUM, method_3p=qo.WINDOW, window=1, phred_offset=255, cutoff_3p=0xFFFFFFFF, dev=dev) == (-1, what + "null ctx")
        assert do_cut(method_3p=qo.RUNSUM, window=0, dev=dev) == (-1, what + "null ctx")  # window is not looked at without WINDOW

    what = "bg_fastq_qual_select: "

    def do_select(n=2, null=(), no_params=False, reserved=0, table=False, dev=False, **kw):
        prm = fastq.qual_select_params(**kw)
        prm["_reserved"] = reserved
        cols = {"qual": p(buf), "qual_off": p(off), "stats_out": p(stats), "bin_out": p(bins)}
        for c in null:
            cols[c] = None
        args = (None, n, None if no_params else p(prm), p(weight) if table else None, *cols.values(), None)
        rc = L.bg_fastq_qual_select_dev(*args, None) if dev else L.bg_fastq_qual_select(*args)
        return rc, L.bg_last_error().decode()

    for dev in (False, True):
        assert do_select(no_params=True, dev=dev) == (-1, what + "null params")
        assert do_select(flags=4, dev=dev) == (-1, what + "unknown flag bits")
        assert do_select(flags=qo.PAIR_BOTH, dev=dev) == (-1, what + "PAIR_BOTH without PAIRED")
        assert do_select(n=1, flags=qo.PAIRED, dev=dev) == (-1, what + "PAIRED with an odd record count")
        assert do_select(phred_offset=256, dev=dev) == (-1, what + "phred_offset above 255")
        assert do_select(reserved=1, dev=dev) == (-1, what + "non-zero _reserved")
        assert do_select(null=["qual_off"], dev=dev) == (-1, what + "null qual_off")
        assert do_select(null=["qual"], dev=dev) == (-1, what + "null qual")
        assert do_select(null=["stats_out", "bin_out"], dev=dev) == (-1, what + "both outputs null")
        assert do_select(n=0, null=["qual", "stats_out", "bin_out"], dev=dev) == (-1, what + "null ctx")
        assert do_select(dev=dev) == (-1, what + "null ctx")
        assert do_select(null=["stats_out"], flags=qo.PAIRED | qo.PAIR_BOTH, table=True, max_weight=1 << 40, dev=dev) == (-1, what + "null ctx")
        assert do_select(null=["bin_out"], max_low_pct=250, dev=dev) == (-1, what + "null ctx")

    what = "bg_fastq_qc_tables: "

    def do_tables(n=2, first=0, step=1, phred=33, max_cycles=100, null=(), dev=False):
        cols = {"seq": p(buf), "seq_off": p(off), "qual": p(buf), "qual_off": p(off), "tables": p(tab)}
        for c in null:
            cols[c] = None
        args = (None, n, first, step, phred, max_cycles, *cols.values())
        rc = L.bg_fastq_qc_tables_dev(*args, None) if dev else L.bg_fastq_qc_tables(*args)
        return rc, L.bg_last_error().decode()

    for dev in (False, True):
        assert do_tables(step=0, dev=dev) == (-1, what + "step 0")
        for mc in (0, 1025):
            assert do_tables(max_cycles=mc, dev=dev) == (-1, what + "max_cycles outside 1 .. BG_QC_MAX_CYCLES")
        assert do_tables(phred=256, dev=dev) == (-1, what + "phred_offset above 255")
        assert do_tables(null=["tables"], dev=dev) == (-1, what + "null tables")
        for col in ("seq_off", "qual_off"):
            assert do_tables(n=0, null=[col], dev=dev) == (-1, what + "null offsets"), col
        for col in ("seq", "qual"):
            assert do_tables(null=[col], dev=dev) == (-1, what + "null seq or qual"), col
            assert do_tables(first=1, step=2, null=[col], dev=dev) == (-1, what + "null seq or qual"), col
            assert do_tables(first=2, null=[col], dev=dev) == (-1, what + "null ctx"), col  # no record selected: not looked at
        for mc in (1, 1024):
            assert do_tables(max_cycles=mc, dev=dev) == (-1, what + "null ctx")


def test_binding_describes_the_structs():
    hdr = open(os.path.join(ROOT, "include", "biogpu.h")).read()
    for name, dtype, size in (("bg_qual_cut_t", _lib.QUAL_CUT_DTYPE, 24), ("bg_qual_stats_t", _lib.QUAL_STATS_DTYPE, 32),
                              ("bg_qual_select_t", _lib.QUAL_SELECT_DTYPE, 32)):
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1))
        fields = [(w, f.strip()) for w, names in re.findall(r"uint(32|64)_t ([\w, ]+);", body) for f in names.split(",")]
        assert [f for _, f in fields] == list(dtype.names), name
        at = 0
        for width, f in fields:  # natural alignment, no padding: every byte of the struct is a field's
            assert dtype.fields[f][1] == at and dtype.fields[f][0].itemsize == int(width) // 8, (name, f)
            at += int(width) // 8
        assert at == dtype.itemsize == size, name
    assert qo.STATS_DTYPE == _lib.QUAL_STATS_DTYPE
    assert _lib.QUAL_STATS_DTYPE.fields["len"][1] == 16 and _lib.QUAL_SELECT_DTYPE.fields["max_weight"][1] == 24
    prm = fastq.qual_cut_params(method_5p=fastq.QCUT_RUNSUM, method_3p=fastq.QCUT_WINDOW, cutoff_5p=7, cutoff_3p=20, window=4)
    assert prm.tobytes() == np.array([33, 1, 2, 7, 20, 4], dtype="<u4").tobytes()
    sel = fastq.qual_select_params(flags=fastq.QSEL_PAIRED, min_mean_q=25, low_q=15, max_low_pct=40, max_weight=1 << 33)
    assert sel.tobytes() == np.array([1, 33, 25, 15, 40, 0], dtype="<u4").tobytes() + np.array([1 << 33], dtype="<u8").tobytes()
    assert (qo.NONE, qo.RUNSUM, qo.WINDOW, qo.PAIRED, qo.PAIR_BOTH) == (_lib.QCUT_NONE, _lib.QCUT_RUNSUM, _lib.QCUT_WINDOW, _lib.QSEL_PAIRED,
                                                                         _lib.QSEL_PAIR_BOTH)
    assert (fastq.ee_weights(33) == qo.ee_weights(33)).all() and int(fastq.ee_weights(33)[33 + 20]) == round(2 ** 20 / 100)
    assert int(fastq.ee_weights(64)[10]) == 1 << 20


def test_tables_words_and_views():
    assert _lib.QC_MAX_CYCLES == 1024
    for mc in (1, 2, 150, 1024):
        R = mc + 1
        assert fastq.qc_tables_words(mc) == qo.tables_words(mc) == 5 * R + 64 * R + (R + 1) + 64 + 1
        buf, t = qo.tables(b"", [0], b"", [0], mc)
        v = fastq.QcTables(np.arange(len(buf), dtype=np.uint64), mc)
        assert v.base.shape == (R, 5) and v.qhist.shape == (R, 64) and len(v.len_hist) == R + 1 and len(v.meanq_hist) == 64
        assert int(v.base[0, 0]) == 0 and int(v.qhist[0, 0]) == 5 * R and int(v.len_hist[0]) == 69 * R
        assert int(v.meanq_hist[0]) == 70 * R + 1 and int(v.n_reads[0]) == 70 * R + 65 == len(buf) - 1
        assert all(len(t[k].reshape(-1)) == len(getattr(v, k).reshape(-1)) for k in t)
