"""The `__host__ __device__` bodies behind bg_sam_markdup, bg_sam_sort_keys and bg_sam_sort (csrc/sam_rule.h: placement, the
unclipped 5' end and the key, the score as the lanes of a group sum it, the entries and their total order, the pass over runs
that picks a group's winner, and the per-line copy plan — head, destination-aligned 16-byte body put together from a misaligned
source, tail) run on the CPU by a stand-alone program (tests/sam_sort_host_bodies.cpp) built with AddressSanitizer and UBSan, on
seeded random batches against the restatement (tests/sam_sort_oracle.py), byte for byte.  Every buffer has exactly its size and
the lines follow a poisoned prefix of 0 .. 15 bytes: a byte loaded or stored outside one stops the program.  Single-end with K = 1
and K = 3, paired with a quarter to two thirds of the reads unmapped (many pairs, many fragments); lines of every length around the 16-byte granule, and one beyond the long-line threshold per round; then the
batches of tests/sam_edge_cases.py at the edges of the copy's two paths and of the score's lane loop.  Nothing is loaded into Python."""
import os
import random
import subprocess

import numpy as np

import sam_edge_cases as ec
import sam_oracle as so
import sam_sort_oracle as sso
from rust_bio_amd import _lib
from sam_sort_cases import CONTIGS, LINE_LENGTHS, MIN_QUAL, PHRED, random_batch, synthetic_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVENTS = ("group of one", "group won on score", "group won on index", "pair group", "fragment flagged by a pair", "fragment group",
          "unplaced", "reverse", "clip term non-zero", "key UINT64_MAX")


def test_sam_sort_bodies_on_the_host_under_sanitizers(tmp_path):
    exe, inp, outp = str(tmp_path / "bodies"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + _lib.CSRC, "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "sam_sort_host_bodies.cpp"), "-o", exe])
    rng = random.Random(41)
    table = np.zeros(len(CONTIGS), dtype=_lib.SAM_CONTIG_DTYPE)
    for c, (name, start, ln) in enumerate(CONTIGS):
        table[c] = (start, ln, 0, len(name), 0)
    seen = {}
    rounds = [(True, 1, so.PAIRED), (False, 1, 0), (False, 3, so.SECONDARY), (True, 1, so.PAIRED), (False, 3, 0), (True, 1, so.PAIRED)] * 3

    def run(rnd, fq, hits, strand, K, key_flags, md_flags, recs, prefix, min_qual=MIN_QUAL):
        n, text, off = len(fq.recs), b"".join(recs), so.offsets(recs)
        with open(inp, "wb") as f:
            f.write(np.array([n, K, key_flags, md_flags, PHRED, min_qual, len(CONTIGS), len(fq.qual), prefix, len(text)], dtype=np.uint64).tobytes())
            f.write(table.tobytes() + hits.tobytes() + strand.tobytes() + fq.recs.tobytes() + bytes(fq.qual))
            f.write(bytes(prefix) + text + off.tobytes())
        subprocess.check_call([exe, inp, outp])
        raw = open(outp, "rb").read()
        w_dup, w_counts = sso.markdup(CONTIGS, fq, hits, strand, md_flags, K, PHRED, min_qual, events=seen)
        w_key = sso.sort_keys(CONTIGS, hits, strand, key_flags, K, events=seen)
        w_perm, w_off, w_text = sso.sort(w_key, recs)
        want = [w_dup.tobytes(), np.array(w_counts, dtype=np.uint64).tobytes(), w_key.tobytes(), w_perm.tobytes(), w_off.tobytes(), w_text]
        assert len(raw) == sum(len(w) for w in want), rnd
        at = 0
        for what, w in zip(("dup", "counts", "key", "perm", "out_off", "text"), want):
            assert raw[at:at + len(w)] == w, (rnd, what)
            at += len(w)
        return w_key

    for rnd, (paired, K, key_flags) in enumerate(rounds):
        n = 2 * rng.randint(150, 220)
        fq, hits, strand = random_batch(rng, n, K=K, paired=paired, p_unmapped=(0.3, 0.55, 0.7)[rnd // 3 % 3] if paired else 0.12)
        prefix = (rnd * 7 + 3) % 16
        recs, text, off = synthetic_lines(rng, n * K, lengths=LINE_LENGTHS + (40, 77, 100), long_at=rng.randrange(n * K),
                                          long_len=sso_long_len(rnd))
        run(rnd, fq, hits, strand, K, key_flags, so.PAIRED if paired else 0, recs, prefix)
    # the copy at the edges of its two paths (tests/sam_edge_cases.py): lengths around the switch to chunks, around a chunk and
    # the 32-column wrap, 256 long lines; the keys go in as hit records
    for i, b in enumerate((ec.sort_switch(), ec.sort_chunk(), ec.sort_rows(256))):
        fq, hits, strand = b.hits()
        assert (run(b.name, fq, hits, strand, 1, 0, 0, b.recs, (5 * i + 9) % 16) == b.key).all()
    # the score at the edges of the lane loop: quality strings of 0 ... 65 535 bytes whose last byte decides
    fq, hits, strand = ec.qual_lengths()
    for min_qual in ec.MIN_QUALS:
        recs, _, _ = synthetic_lines(rng, len(fq.recs))
        run("qualities %d" % min_qual, fq, hits, strand, 1, 0, 0, recs, 1, min_qual)
    assert not {k: seen.get(k, 0) for k in EVENTS if seen.get(k, 0) < 50}, seen


def sso_long_len(rnd):
    """a line beyond the long-line threshold (16 384 bytes), its length walking through the residues of 16"""
    return 16385 + 4096 * (rnd % 3) + rnd
