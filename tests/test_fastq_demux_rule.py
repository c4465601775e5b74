"""Demultiplexing on the CPU: the Python restatement of the two rules of include/biogpu.h (tests/fastq_demux_oracle.py) on
hand cases a reader can check by eye, the argument checks of bg_fastq_demux_assign / bg_fastq_demux_split, which return
before a device is touched and say why (bg_last_error), and the binding's view of bg_demux_params_t."""
import numpy as np

import fastq_demux_oracle as dm
from rust_bio_amd import _lib, fastq

X = None  # no hit


def records(rows, ylen=30):
    """bg_alignment_t[len(rows) * n_pat]: a row holds per pattern None or a score or (score, ystart, yend)"""
    n_pat = len(rows[0])
    hits = np.zeros(len(rows) * n_pat, dtype=_lib.ALN_DTYPE)
    hits["score"], hits["ylen"], hits["mode"] = dm.MIN_SCORE, ylen, 2
    for r, row in enumerate(rows):
        for p, h in enumerate(row):
            if h is not None:
                s, ys, ye = h if isinstance(h, tuple) else (h, 0, 8)
                c = hits[r * n_pat + p]
                c["score"], c["ystart"], c["yend"], c["xlen"], c["xend"] = s, ys, ye, 8, 8
    return hits


# patterns 0, 1 -> bin 0; 2 -> bin 1; 3 -> bin 2; 4 is ignored (an adapter).  (scores per pattern, min_margin) -> (bin, pat)
BINS = [0, 0, 1, 2, dm.IGNORE]
U, A = 3, 4  # unassigned, ambiguous
TABLE = [
    ([X, X, X, X, X], 1, (U, dm.IGNORE)),  # nothing
    ([X, X, X, X, 0], 1, (U, dm.IGNORE)),  # only the ignored pattern hits
    ([X, X, 1, X, X], 1, (1, 2)),          # one hit: second is infinite
    ([X, X, 1, X, 0], 1, (1, 2)),          # the ignored pattern's better hit does not matter
    ([0, X, 1, X, X], 1, (0, 0)),          # second - best = 1 = min_margin
    ([0, X, 1, X, X], 2, (A, dm.IGNORE)),  # ... one below min_margin
    ([0, X, 2, X, X], 2, (0, 0)),          # ... and at it again
    ([1, 1, X, X, X], 1, (0, 0)),          # a tie inside one bin: the lower pattern, nothing ambiguous
    ([1, 0, X, X, X], 5, (0, 1)),          # two patterns of one bin: the better one, no runner-up in another bin
    ([X, 1, 1, X, X], 0, (0, 1)),          # min_margin 0: a tie between bins goes to the lower pattern
    ([X, 1, 1, X, X], 1, (A, dm.IGNORE)),  # ... with a margin it is ambiguous
    ([X, X, 2, 1, X], 1, (2, 3)),          # the winner is not the first hit
    ([3, 0, 1, 2, X], 1, (0, 1)),          # second is the best of the OTHER bins (1), not pattern 0's 3
    ([3, 0, 2, 1, X], 2, (A, dm.IGNORE)),
    ([300, X, 301, X, X], 1, (0, 0)),      # scores of the long call's range
]


def test_assign_table():
    for row, margin, (want_bin, want_pat) in TABLE:
        hits = records([row])
        b, h, p = dm.assign(hits, 5, BINS, 3, min_margin=margin)
        assert (int(b[0]), int(p[0])) == (want_bin, want_pat), (row, margin)
        if want_pat != dm.IGNORE:
            assert h[0].tobytes() == hits[want_pat].tobytes()
        else:
            assert h[0].tobytes() == dm.no_hit(hits[0]).tobytes()
            assert (int(h[0]["score"]), int(h[0]["ylen"]), int(h[0]["mode"]), int(h[0]["xlen"])) == (dm.MIN_SCORE, 30, 2, 0)


def test_anchors_and_pairs():
    hits = records([[(0, 3, 11)], [(0, 4, 12)], [(0, 19, 27)], [(0, 18, 26)]])  # ylen 30: 3 and 4 behind the end
    assert list(dm.assign(hits, 1, [0], 1, flags=dm.ANCHOR_5P, max_offset=3)[0]) == [0, 1, 1, 1]
    assert list(dm.assign(hits, 1, [0], 1, flags=dm.ANCHOR_3P, max_offset=3)[0]) == [1, 1, 0, 1]
    assert list(dm.assign(hits, 1, [0], 1, max_offset=0)[0]) == [0, 0, 0, 0]  # no anchor: anywhere
    # pairs (bins: pattern p -> bin p): winner on mate 1, on mate 2, on both with equal (score, p), excluded by MATE flags
    hits = records([[0, X], [X, X],   [X, X], [X, 1],   [1, X], [1, X],   [X, X], [0, X],   [2, X], [X, 0]])
    b, h, p = dm.assign(hits, 2, [0, 1], 2, flags=dm.PAIRED)
    assert list(b) == [0, 0, 1, 1, 0, 0, 0, 0, 1, 1]
    assert list(p) == [0, dm.IGNORE, dm.IGNORE, 1, 0, dm.IGNORE, dm.IGNORE, 0, dm.IGNORE, 1]
    assert h[4].tobytes() == hits[8].tobytes() and int(h[5]["score"]) == dm.MIN_SCORE  # equal: mate 1 carries it
    b, h, p = dm.assign(hits, 2, [0, 1], 2, flags=dm.PAIRED | dm.MATE1)
    assert list(b) == [0, 0, 2, 2, 0, 0, 2, 2, 0, 0] and list(p[6:]) == [dm.IGNORE, dm.IGNORE, 0, dm.IGNORE]
    b, h, p = dm.assign(hits, 2, [0, 1], 2, flags=dm.PAIRED | dm.MATE2)
    assert list(b) == [2, 2, 1, 1, 0, 0, 0, 0, 1, 1] and list(p[:6]) == [dm.IGNORE, dm.IGNORE, dm.IGNORE, 1, dm.IGNORE, 0]
    assert dm.assign(hits, 2, [0, 1], 2, flags=dm.PAIRED | dm.MATE1 | dm.MATE2)[0].tolist() == dm.assign(hits, 2, [0, 1], 2, flags=dm.PAIRED)[0].tolist()
    # the pair's runner-up may sit on the other mate: 0 on mate 1 (bin 0), 1 on mate 2 (bin 1)
    hits = records([[0, X], [X, 1]])
    assert list(dm.assign(hits, 2, [0, 1], 2, flags=dm.PAIRED, min_margin=1)[0]) == [0, 0]
    assert list(dm.assign(hits, 2, [0, 1], 2, flags=dm.PAIRED, min_margin=2)[0]) == [3, 3]
    assert list(dm.assign(hits, 2, [0, 1], 2, min_margin=2)[0]) == [0, 1]


def test_split_on_a_hand_case():
    from fastq_write_cases import Batch
    b = Batch([(b"r%d" % i, None, b"ACGT"[:ln], b"IIII"[:ql]) for i, (ln, ql) in enumerate([(4, 4), (0, 0), (3, 2), (1, 1), (2, 2), (4, 3)])])
    bins = [2, 0, 7, 2, 0xFFFFFFFF, 3]  # n_bins 2: 7 and 0xFFFFFFFF are unassigned (group 2), 3 is ambiguous
    hit = records([[i] for i in range(6)])
    recs, seq, so, qual, qo, h, perm, bin_off = dm.split(bins, 2, *b.columns(), hit=hit)
    assert list(perm) == [1, 0, 2, 3, 4, 5] and list(bin_off) == [0, 1, 1, 5, 6]
    assert seq == b"" + b"ACGT" + b"ACG" + b"A" + b"AC" + b"ACGT" and qual == b"IIII" + b"II" + b"I" + b"II" + b"III"
    assert list(so) == [0, 0, 4, 7, 8, 10, 14] and list(recs["seq_off"]) == list(so[:6]) and list(recs["qual_off"]) == list(qo[:6])
    assert [int(x["score"]) for x in h] == [1, 0, 2, 3, 4, 5]
    assert [int(c["id_off"]) for c in recs] == [int(b.recs[r]["id_off"]) for r in perm]
    e = dm.split([], 3, b.recs[:0], b"", [0], b"", [0])
    assert list(e[7]) == [0] * 6 and list(e[2]) == [0]


def test_entry_points_check_their_arguments_before_any_device():
    L = _lib.lib()
    hit, out = np.zeros(4, dtype=_lib.ALN_DTYPE), np.zeros(2, dtype=_lib.ALN_DTYPE)
    bins = np.zeros(2, dtype=np.uint32)
    p = lambda a: a.ctypes.data  # noqa: E731
    what = "bg_fastq_demux_assign: "

    def assign(n=2, flags=0, n_bins=2, n_pat=2, pat_bin=(0, 1), null=None, no_params=False, dev=False):
        prm = fastq.demux_params(n_bins, flags, 1, 0)
        pb = np.array(pat_bin, dtype=np.uint32) if pat_bin is not None else None
        cols = {"hits": p(hit), "bin": p(bins), "hit_out": p(out)}
        if null:
            cols[null] = None
        args = (None, n, None if no_params else p(prm), cols["hits"], n_pat, None if pb is None else p(pb), cols["bin"], cols["hit_out"], None)
        rc = L.bg_fastq_demux_assign_dev(*args, None) if dev else L.bg_fastq_demux_assign(*args)
        return rc, L.bg_last_error().decode()

    for dev in (False, True):
        assert assign(no_params=True, dev=dev) == (-1, what + "null params")
        assert assign(flags=32, dev=dev) == (-1, what + "unknown flag bits")
        assert assign(flags=dm.ANCHOR_5P | dm.ANCHOR_3P, dev=dev) == (-1, what + "both ANCHOR flags")
        for m in (dm.MATE1, dm.MATE2, dm.MATE1 | dm.MATE2):
            assert assign(flags=m, dev=dev) == (-1, what + "a MATE flag without PAIRED")
        assert assign(n=1, flags=dm.PAIRED, dev=dev) == (-1, what + "PAIRED with an odd record count")
        assert assign(n_bins=0, dev=dev) == (-1, what + "n_bins 0")
        assert assign(n_bins=1025, dev=dev) == (-8, what + "n_bins above BG_DMX_MAX_BINS")
        assert assign(n_pat=0, dev=dev) == (-1, what + "n_pat 0")
        assert assign(n_pat=1025, dev=dev) == (-8, what + "n_pat above BG_MYERS_MAX_PATTERNS")
        assert assign(pat_bin=None, dev=dev) == (-1, what + "null pat_bin")
        assert assign(pat_bin=(0, 2), dev=dev) == (-1, what + "a pat_bin entry names no bin")
        assert assign(pat_bin=(0xFFFFFFFE, 0), dev=dev) == (-1, what + "a pat_bin entry names no bin")
        for col in ("hits", "bin", "hit_out"):
            assert assign(null=col, dev=dev) == (-1, what + "null hits, bin or hit_out"), col
            assert assign(n=0, null=col, dev=dev) == (-1, what + "null ctx"), col  # no record: not looked at
        # legal arguments get as far as the missing ctx
        assert assign(dev=dev) == (-1, what + "null ctx")
        assert assign(pat_bin=(dm.IGNORE, 1), dev=dev) == (-1, what + "null ctx")
        assert assign(flags=dm.ANCHOR_3P | dm.PAIRED | dm.MATE2, n_bins=1024, pat_bin=(1023, 0), dev=dev) == (-1, what + "null ctx")

    rec = np.zeros(2, dtype=_lib.FQREC_DTYPE)
    buf, off, boff = np.zeros(8, dtype=np.uint8), np.zeros(3, dtype=np.uint64), np.zeros(1027, dtype=np.uint64)
    what = "bg_fastq_demux_split: "

    def split(n=2, n_bins=2, null=None, hit_in=None, hit_o=None, dev=False):
        cols = {"bin": p(bins), "hit": hit_in, "recs": p(rec), "seq": p(buf), "seq_off": p(off), "qual": p(buf), "qual_off": p(off),
                "recs_out": p(rec), "seq_out": p(buf), "seq_off_out": p(off), "qual_out": p(buf), "qual_off_out": p(off), "hit_out": hit_o,
                "perm": None, "bin_off": p(boff)}
        if null:
            cols[null] = None
        args = (None, n, n_bins, *cols.values())
        rc = L.bg_fastq_demux_split_dev(*args, None, None) if dev else L.bg_fastq_demux_split(*args)
        return rc, L.bg_last_error().decode()

    for dev in (False, True):
        assert split(n_bins=0, dev=dev) == (-1, what + "n_bins 0")
        assert split(n_bins=1025, dev=dev) == (-8, what + "n_bins above BG_DMX_MAX_BINS")
        assert split(null="bin_off", dev=dev) == (-1, what + "null bin_off")
        for col in ("seq_off_out", "qual_off_out"):
            assert split(n=0, null=col, dev=dev) == (-1, what + "null output offsets"), col
        assert split(hit_o=p(out), dev=dev) == (-1, what + "hit_out without hit")
        for col in ("bin", "recs", "seq", "seq_off", "qual", "qual_off", "recs_out", "seq_out", "qual_out"):
            assert split(null=col, dev=dev) == (-1, what + "null bin or column"), col
            assert split(n=0, null=col, dev=dev) == (-1, what + "null ctx"), col
        assert split(dev=dev) == (-1, what + "null ctx")
        assert split(n_bins=1024, hit_in=p(hit), hit_o=p(out), dev=dev) == (-1, what + "null ctx")
        assert split(hit_in=p(hit), dev=dev) == (-1, what + "null ctx")  # hit without hit_out: nothing to carry, allowed


def test_binding_describes_the_params_struct():
    prm = fastq.demux_params(96, fastq.DMX_ANCHOR_5P | fastq.DMX_PAIRED | fastq.DMX_MATE1, 1, 2)
    assert prm.tobytes() == np.array([13, 96, 1, 2], dtype="<u4").tobytes() and _lib.DEMUX_PARAMS_DTYPE.itemsize == 16
    assert fastq.demux_params(3).tobytes() == np.array([0, 3, 0, 0], dtype="<u4").tobytes()
    assert (dm.ANCHOR_5P, dm.ANCHOR_3P, dm.PAIRED, dm.MATE1, dm.MATE2, dm.IGNORE) == (
        _lib.DMX_ANCHOR_5P, _lib.DMX_ANCHOR_3P, _lib.DMX_PAIRED, _lib.DMX_MATE1, _lib.DMX_MATE2, _lib.DMX_IGNORE)
    assert _lib.DMX_MAX_BINS == 1024 == _lib.MYERS_MAX_PATTERNS
    # the header's struct: four uint32 fields in this order
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "biogpu.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} bg_demux_params_t;", hdr).group(1)
    assert re.findall(r"uint32_t (\w+);", body) == list(_lib.DEMUX_PARAMS_DTYPE.names)
