"""Seeded generators of synthetic hit records for the duplicate-marking, key and sort tests (no index is needed for any of
them): reads with made-up qualities, hits at coordinates drawn from a few values so that groups form, on either strand, some
clipped, some across a contig's end, some unmapped."""
import numpy as np

import sam_oracle as so
from rust_bio_amd import _lib

CONTIGS = [(b"chrA", 0, 1999), (b"chr_B.1", 2000, 1999), (b"c|3", 4000, 2000)]
# the index text goes beyond 2^32: two contigs whose starts differ only above bit 32, and one far above
BIG_CONTIGS = [(b"lo", 5, 3000), (b"hi", 2**32 + 5, 3000), (b"far", 2**40 + 77, 5000)]
PHRED, MIN_QUAL = 33, 15


def make_hit(score, strand, ref_start, ref_end, xstart, xend, xlen):
    """one entry of a hit list: None is an unmapped read"""
    return {"score": score, "strand": strand, "ref_start": ref_start, "ref_end": ref_end, "xstart": xstart, "xend": xend, "xlen": xlen}


def arrays(reads, hits):
    """reads: [(id, seq, qual)] bytes triples; hits: len(reads) * K entries of make_hit or None.
    Returns (fq: so.Fastq, hits: SEED_HIT_DTYPE[], strand: uint8[])."""
    fq = so.Fastq(reads, _lib.FQREC_DTYPE)
    h = np.zeros(len(hits), dtype=_lib.SEED_HIT_DTYPE)
    strand = np.full(len(hits), so.HIT_NONE, dtype=np.uint8)
    for s, e in enumerate(hits):
        if e is None:
            h[s]["aln"]["score"] = so.MIN_SCORE
            h[s]["window_start"] = h[s]["ref_start"] = h[s]["ref_end"] = 2**64 - 1
            continue
        a = h[s]["aln"]
        a["score"], a["xstart"], a["xend"], a["xlen"], a["mode"] = e["score"], e["xstart"], e["xend"], e["xlen"], 2
        h[s]["ref_start"], h[s]["ref_end"], strand[s] = e["ref_start"], e["ref_end"], e["strand"]
    return fq, h, strand


def read_of(r, length, q, paired=False):
    """a read of `length` bases whose qualities are all q"""
    name = b"r%d/%d" % (r // 2, r % 2 + 1) if paired else b"r%d" % r
    return name, b"ACGT" * (length // 4) + b"ACGT"[:length % 4], bytes([PHRED + q]) * length


def random_batch(rng, n, K=1, paired=False, contigs=CONTIGS, n_coords=24, p_unmapped=0.12, p_clip=0.2, p_cross=0.05, p_copy=0.3):
    """n reads with K slots each; `rng` is a random.Random.  Coordinates come from n_coords values per contig and alignment
    lengths from three values, qualities from three levels (one below MIN_QUAL) and two read lengths: groups form, scores tie.
    With `paired`, a pair takes the placements of an earlier pair with probability p_copy, half of the time with the mates
    swapped (the same two ends, but lo is the other mate)."""
    reads, places = [], []  # a placement: None or (strand, start, rlen, clip at the read's start, clip at its end, score)
    for r in range(n):
        length = rng.choice((20, 31))
        q = rng.choice((10, 20, 20, 30))
        name, seq, qual = read_of(r, length, q, paired)
        if rng.random() < 0.2:  # a mixed read: the floor decides part of its score
            qual = bytes(rng.choice((PHRED + 5, PHRED + 14, PHRED + 15, PHRED + 40)) for _ in range(length))
        reads.append((name, seq, qual))
        for k in range(K):
            if rng.random() < (p_unmapped if k == 0 else 0.4):
                places.append(None)
                continue
            _, c_start, c_len = contigs[rng.randrange(len(contigs))]
            clip = [rng.randrange(1, 4) if rng.random() < p_clip else 0 for _ in range(2)]
            rlen = rng.choice((18, 20, 23))
            start = c_start + 40 + 9 * rng.randrange(n_coords)
            if rng.random() < 0.02:
                start = c_start + rng.randrange(0, 3)  # at the contig's first bases: the forward clip saturates
            if rng.random() < p_cross:
                start = c_start + c_len - rng.randrange(1, rlen)  # runs over the contig's end
            places.append((rng.randrange(2), start, rlen, clip[0], clip[1], rng.randrange(10, 60)))
        if paired and r % 2 == 1 and r >= 3 and rng.random() < p_copy:
            p = rng.randrange(r // 2)
            places[r - 1], places[r] = (places[2 * p], places[2 * p + 1])[::rng.choice((1, -1))]
    hits = []
    for s, pl in enumerate(places):
        length = len(reads[s // K][1])
        hits.append(None if pl is None else make_hit(pl[5], pl[0], pl[1], pl[1] + pl[2], pl[3], length - pl[4], length))
    return arrays(reads, hits)


def runs_batch(sizes, paired=False, contigs=CONTIGS, equal_scores=False, seed=1):
    """groups of exactly the given sizes, their members interleaved over the batch: group g sits at its own coordinate; with
    `paired` the members are pairs (mate 1 forward at the coordinate, mate 2 reverse 150 behind it)"""
    import random
    rng = random.Random(seed)
    members = [g for g, size in enumerate(sizes) for _ in range(size)]
    rng.shuffle(members)
    reads, hits = [], []
    for i, g in enumerate(members):
        _, c_start, _ = contigs[g % len(contigs)]
        at = c_start + 10 + 3 * g
        for mate in range(2 if paired else 1):
            r = len(reads)
            q = 20 if equal_scores else rng.choice((16, 20, 30, 40))
            reads.append(read_of(r, 24, q, paired))
            if mate == 0:
                hits.append(make_hit(40, 0, at, at + 24, 0, 24, 24))
            else:
                hits.append(make_hit(40, 1, at + 150, at + 174, 0, 24, 24))
    return arrays(reads, hits)


LINE_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257)


def synthetic_lines(rng, n, lengths=LINE_LENGTHS, long_at=None, long_len=140_000):
    """n records of the given lengths in random order (every byte value but chosen so that a misplaced byte shows), one of
    long_len bytes at index long_at, or several: long_at = {index: length}; returns (records: list of bytes, text: bytes,
    off: uint64[n + 1])"""
    recs = []
    longs = long_at if isinstance(long_at, dict) else {long_at: long_len}
    for i in range(n):
        ln = longs[i] if i in longs else rng.choice(lengths)
        j = np.arange(ln, dtype=np.uint64)
        recs.append(((i * 7 + j * 13 + (j >> 8) * 5 + (j >> 12)) & 0xFF).astype(np.uint8).tobytes())
    return recs, b"".join(recs), so.offsets(recs)
