"""Batches for the demultiplexing tests: hand-made and random hit records in the layout of `bg_myers_best_batch` (read r's
n_pat records at r * n_pat), pattern-to-sample tables, and every legal combination of the assign flags."""
import numpy as np

import fastq_demux_oracle as dm
from rust_bio_amd import _lib

LEGAL_FLAGS = [a | p for a in (0, dm.ANCHOR_5P, dm.ANCHOR_3P)
               for p in (0, dm.PAIRED, dm.PAIRED | dm.MATE1, dm.PAIRED | dm.MATE2, dm.PAIRED | dm.MATE1 | dm.MATE2)]


def blank_hits(n, n_pat, ylen=30, xlen=8):
    """no-hit records as the Myers calls leave them: score BG_MIN_SCORE, xlen, ylen, mode"""
    hits = np.zeros(n * n_pat, dtype=_lib.ALN_DTYPE)
    hits["score"], hits["xlen"], hits["ylen"], hits["mode"] = dm.MIN_SCORE, xlen, ylen, 2
    return hits


def set_hit(hits, n_pat, r, p, score, ystart=0, yend=None):
    c = hits[r * n_pat + p]
    c["score"], c["ystart"], c["yend"] = score, ystart, ystart + 8 if yend is None else yend
    c["xend"], c["n_ops"], c["ops_off"] = c["xlen"], 8, (r * n_pat + p) * 16  # bytes a verbatim copy must carry
    return hits


def random_hits(rng, n, n_pat, p_hit=0.3, max_score=3):
    """few distinct scores and offsets, so that ties, margins at their edge and anchors at theirs are common"""
    hits = blank_hits(n, n_pat)
    for r in range(n):
        ylen = rng.randint(8, 40)
        hits["ylen"][r * n_pat:(r + 1) * n_pat] = ylen
        for p in range(n_pat):
            if rng.random() < p_hit:
                ys = rng.choice([0, 1, 2, 3, ylen - 8, max(0, ylen - 10)])
                set_hit(hits, n_pat, r, p, rng.randint(0, max_score), ys, min(ylen, ys + 8))
    return hits


def random_pat_bin(rng, n_pat, n_bins, p_ignore=0.15):
    return np.array([dm.IGNORE if rng.random() < p_ignore else rng.randrange(n_bins) for _ in range(n_pat)], dtype=np.uint32)
