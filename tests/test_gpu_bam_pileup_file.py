"""The pileup of a file the library wrote, on the paired batch of tests/test_gpu_bam_read_roundtrip.py: `bam.sorted_bam(...,
compress=True)` -> `bam.pileup_bam` over every contig equals tests/bam_pileup_oracle.py on the file's records, and equals a
second derivation that never sees a BAM byte: the lines of `sam.sorted_sam` for the same hits, parsed in plain Python for FLAG,
RNAME, POS, MAPQ, CIGAR, SEQ and QUAL.  With 0x400 taken out of `exclude` the rows grow by exactly the duplicates' bases."""
import re

import numpy as np
import pytest

import bam_pileup_oracle as po
from rust_bio_amd import bam, sam
from rust_bio_amd.pipeline import PairParams, seed_extend_pairs_mapq_arrays
from test_gpu_bam_read_roundtrip import entries_of
from test_gpu_sam_sorted_text import FLAGS, MIN_QUAL, PHRED, SC, case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mapped():
    B = case()
    p = B.parsed
    params, md = sam.SamParams(FLAGS, 1), sam.MarkdupParams(sam.SAM_PAIRED, 1, PHRED, MIN_QUAL)
    hits, strand, pairs, multi, ops = seed_extend_pairs_mapq_arrays(B.fm, SC, p.seq, p.seq_off, pair_params=PairParams(0, 1000, 17))
    chain = dict(multi=multi, pairs=pairs, markdup=md, ctx=B.fm.ctx)
    file = bam.sorted_bam(B.fm, params, B.contigs, p, hits, strand, ops, compress=True, **chain)
    text = sam.sorted_sam(B.fm, params, B.contigs, p, hits, strand, ops, **chain)
    _, contigs, stream, off = bam.read_bam(file, ctx=B.fm.ctx)
    entries = entries_of(contigs)
    slots = [stream[int(a):int(b)] for a, b in zip(off, off[1:])]
    regions = [(c, 0, ln) for c, (_, _, ln) in enumerate(entries)]
    return dict(B=B, file=file, text=text, entries=entries, slots=slots, regions=regions)


def text_pileup(text, entries, regions, exclude=0x704, min_baseq=0, strands=False):
    """rows from SAM lines alone: one dictionary entry a counted base"""
    names = [e[0] for e in entries]
    w = 16 if strands else 8
    counts = {}

    def add(ref, p, col):
        counts.setdefault((ref, p), [0] * w)[col] += 1
    for line in text.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        flag, rname, pos, cigar, seq, qual = int(f[1]), f[2], int(f[3]) - 1, f[5], f[9].upper(), f[10]  # (BAM's codes know no case)
        if rname == b"*" or pos < 0 or flag & 4 or flag & exclude:
            continue
        ref, base = names.index(rname), 8 if strands and flag & 0x10 else 0
        r, q = pos, 0
        for n, op in re.findall(rb"(\d+)([MIDNSHP=X])", cigar):
            n = int(n)
            if op in b"M=X":
                for k in range(n):
                    if seq == b"*":
                        add(ref, r + k, base + po.OTHER)
                    elif qual == b"*" or qual[q + k] - 33 >= min_baseq:
                        add(ref, r + k, base + (b"ACGT".index(seq[q + k:q + k + 1]) if seq[q + k:q + k + 1] in b"ACGT" else po.OTHER))
                r, q = r + n, q + n
            elif op == b"I":
                if r > pos:
                    add(ref, r - 1, base + po.INS)
                q += n
            elif op in b"DN":
                for k in range(n):
                    add(ref, r + k, base + (po.DEL if op == b"D" else po.SKIP))
                r += n
            elif op == b"S":
                q += n
    zero = [0] * w
    return np.array([counts.get((ref, p), zero) for ref, beg, end in regions for p in range(beg, end)], dtype=np.uint32).reshape(-1, w)


def test_the_files_pileup_is_the_oracles_and_the_sam_texts(mapped):
    entries, regions = mapped["entries"], mapped["regions"]
    named = [(entries[c][0].decode() if c % 2 else c, beg, end) for c, beg, end in regions]  # by name and by index
    for kw in (dict(), dict(min_baseq=20), dict(flags=bam.PILEUP_STRANDS, exclude=0x300)):
        rows, row_off = bam.pileup_bam(mapped["file"], named, ctx=mapped["B"].fm.ctx, **kw)
        want, want_off = po.pileup(mapped["slots"], entries, regions, **dict(dict(flags=0, require=0, exclude=0x704, min_mapq=0, min_baseq=0), **kw))
        assert row_off.tolist() == want_off and (rows == np.array(want, dtype=np.uint32)).all(), kw
        from_text = text_pileup(mapped["text"], entries, regions, exclude=kw.get("exclude", 0x704), min_baseq=kw.get("min_baseq", 0),
                                strands=bool(kw.get("flags", 0)))
        assert rows.shape == from_text.shape and (rows == from_text).all(), kw
        bases = int(from_text[:, :5].sum()) + (int(from_text[:, 8:13].sum()) if from_text.shape[1] == 16 else 0)
        assert int(bam.depth(rows).sum()) == bases > 0 and int(bam.depth(rows, deletions=True).sum()) >= bases


def test_duplicates_are_exactly_what_0x400_excludes(mapped):
    entries, regions, ctx = mapped["entries"], mapped["regions"], mapped["B"].fm.ctx
    without, _ = bam.pileup_bam(mapped["file"], regions, ctx=ctx)
    with_dups, _ = bam.pileup_bam(mapped["file"], regions, exclude=0x304, ctx=ctx)
    dups, _ = po.pileup(mapped["slots"], entries, regions, require=0x400, exclude=0x304)
    dups = np.array(dups, dtype=np.uint32)
    assert int(dups.sum()) > 0 and (with_dups - without == dups).all()
    assert (with_dups == text_pileup(mapped["text"], entries, regions, exclude=0x304)).all()
