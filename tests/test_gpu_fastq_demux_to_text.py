"""Demultiplexing end to end, nothing but the split's group offsets and the writers' totals crossing to the host in between:
interleaved paired FASTQ text with inline 5' barcodes on mate 1 -> bg_fastq_parse_dev -> bg_myers_best_batch_dev (12 barcodes,
k = 1) -> bg_fastq_demux_assign_dev (anchored at the 5' end, the pair by mate 1, margin 1) -> bg_fastq_trim_dev on assign's one
record per read -> bg_fastq_demux_split_dev -> bg_fastq_emit_dev twice (R1 and R2), ONE call each for all samples.  Every
sample's slice of the two texts is compared with what the Python restatements write for that sample: the assign and split rules
(tests/fastq_demux_oracle.py), the trim rule (tests/myers_oracle.py) and `Writer::write` (tests/fastq_write_oracle.py).  The
Myers records the chain starts from are the device's, downloaded after the last call (that call has its own tests); every eighth
pair's are compared with the Myers restatement here as well."""
import random

import numpy as np
import pytest
import torch

import fastq_demux_oracle as dm
import fastq_write_oracle as fw
import myers_oracle as mo
from fastq_write_cases import Batch
from myers_cases import dna
from rust_bio_amd import _lib, fastq, myers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, N_BC, K = 4000, 12, 1


def barcodes(rng):
    """12 barcodes of 8 nt, any two at least 3 substitutions apart, except that 1 is 0 with two of them"""
    out = [dna(rng, 8)]
    twin = bytearray(out[0])
    for pos in (2, 5):
        twin[pos] = rng.choice([c for c in b"ACGT" if c != twin[pos]])
    out.append(bytes(twin))
    while len(out) < N_BC:
        c = dna(rng, 8)
        if all(sum(x != y for x, y in zip(c, o)) >= 3 for o in out):
            out.append(c)
    return out


def make_reads(bcs, seed=33):
    """N interleaved mates; mate 1 is barcode + 12 .. 142 bases, mate 2 20 .. 150 bases.  Of the barcodes a fifth carry one
    substitution, every 25th pair's is one substitution from both sample 0 and sample 1, every 20th pair has none, every 50th
    pair's mate 1 is only the barcode"""
    rng = random.Random(seed)
    reads, kinds = [], []
    for q in range(N // 2):
        bc = bytearray(bcs[rng.randrange(N_BC)])
        kind = "exact"
        if q % 25 == 7:
            bc = bytearray(bcs[0])
            bc[2] = bcs[1][2]  # one substitution from barcode 0 and from barcode 1
            kind = "between"
        elif q % 20 == 3:
            bc, kind = bytearray(), "none"
        elif rng.random() < 0.2:
            pos = rng.randrange(8)
            bc[pos] = rng.choice([c for c in b"ACGT" if c != bc[pos]])
            kind = "substituted"
        insert = b"" if q % 50 == 11 and bc else dna(rng, rng.randint(20 if not bc else 12, 142))
        m1, m2 = bytes(bc) + insert, dna(rng, rng.randint(20, 150))
        for mate, s in enumerate((m1, m2)):
            reads.append((b"pair%d" % q, b"%d:N:0" % (mate + 1), s, bytes(rng.randint(33, 73) for _ in range(len(s)))))
        kinds.append(kind if insert or not bc else "only")
    return reads, kinds


def restated(reads, kinds, hits, pat_bin, flags):
    """assign, trim and split on the restatements, and what the case holds: (bin, hit_out, trimmed records, their Batch, split)"""
    w_bin, w_hit, _ = dm.assign(hits, N_BC, pat_bin, N_BC, flags=flags, min_margin=1, max_offset=1)
    trimmed = []
    for r, (id_, desc, s, q) in enumerate(reads):
        (lo, hi), (qlo, qhi) = mo.trim_range(mo.TRIM_5P, [(int(w_hit[r]["score"]), int(w_hit[r]["ystart"]), int(w_hit[r]["yend"]))], len(s), len(q))
        trimmed.append((id_, desc, s[lo:hi], q[qlo:qhi]))
    tb = Batch(trimmed)
    split = dm.split(w_bin, N_BC, *tb.columns())
    w_boff = split[7]
    pair_bin = w_bin[0::2]
    by_kind = {k: [int(b) for b, kk in zip(pair_bin, kinds) if kk == k] for k in set(kinds)}
    assert set(by_kind) == {"exact", "substituted", "between", "none", "only"}
    # a chance hit of another barcode next to the read's own, or at the start of an insert, is possible: nearly all, not all
    for k in ("exact", "substituted", "only"):
        assert sum(b < N_BC for b in by_kind[k]) >= 0.9 * len(by_kind[k]), k
    assert len(by_kind["substituted"]) > 250 and len(by_kind["only"]) >= 30
    assert all(b == N_BC + 1 for b in by_kind["between"]) and len(by_kind["between"]) == 80
    assert sum(b == N_BC for b in by_kind["none"]) >= 0.8 * len(by_kind["none"]) and len(by_kind["none"]) >= 90
    assert (w_bin[0::2] == w_bin[1::2]).all() and all(w_boff[g + 1] > w_boff[g] for g in range(N_BC + 2))
    assert all(int(x) % 2 == 0 for x in w_boff)
    cut = [len(t[2]) < len(r[2]) for t, r in zip(trimmed, reads)]
    assert not any(cut[1::2]) and sum(cut[0::2]) == int((pair_bin < N_BC).sum())
    assert sum(len(t[2]) == 0 for t in trimmed) >= 0.95 * len(by_kind["only"])
    return w_bin, w_hit, trimmed, tb, split


def test_demultiplex_trim_and_write_paired_reads():
    bcs = barcodes(random.Random(5))
    reads, kinds = make_reads(bcs)
    fq = b"".join(fw.write(*r) for r in reads)
    pat_bin = np.arange(N_BC, dtype=np.uint32)
    flags = fastq.DMX_ANCHOR_5P | fastq.DMX_PAIRED | fastq.DMX_MATE1
    stream = torch.cuda.current_stream().cuda_stream
    d_fq = torch.frombuffer(bytearray(fq), dtype=torch.uint8).to(DEV)
    n, status, _, d_recs, d_seq, d_so, d_qual, d_qo = fastq.parse_dev(d_fq, stream=stream)
    assert (n, status) == (N, "ok")
    d_hits, _ = myers.best_batch_dev([myers.Myers(b) for b in bcs], d_seq, d_so, K, stream=stream)
    d_bin, d_hit, _ = fastq.demux_assign_dev(n, d_hits, N_BC, pat_bin, N_BC, flags=flags, min_margin=1, max_offset=1, stream=stream)
    t_recs, t_seq, t_so, t_qual, t_qo, _ = myers.trim_dev(myers.TRIM_5P, d_hit, 1, n, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream,
                                                          want_totals=False)
    s_recs, s_seq, s_so, s_qual, s_qo, _, _, _, bin_off = fastq.demux_split_dev(n, d_bin, N_BC, t_recs, t_seq, t_so, t_qual, t_qo, stream=stream)
    texts = []
    for first in (0, 1):
        d_out, d_off, _ = fastq.emit_dev(n, d_fq, s_recs, s_seq, s_qual, first, 2, stream=stream)
        texts.append([t.cpu().numpy().tobytes() for t in fastq.demux_texts(d_out, d_off, bin_off, N_BC, first, 2)])
    torch.cuda.synchronize()

    # the same on the restatements, from the device's Myers records
    hits = myers.records(d_hits)
    sample = [r for q in range(0, N // 2, 8) for r in (2 * q, 2 * q + 1)]
    want_hits, _ = mo.best_records([mo.Myers(b) for b in bcs], [reads[r][2] for r in sample], K)
    assert hits.reshape(N, N_BC)[sample].tobytes() == want_hits.tobytes()
    w_bin, w_hit, trimmed, tb, (w_recs, w_seq, _, w_qual, _, _, w_perm, w_boff) = restated(reads, kinds, hits, pat_bin, flags)
    assert (d_bin.cpu().numpy().view(np.uint32) == w_bin).all() and d_hit.cpu().numpy().tobytes() == w_hit.tobytes()
    assert (bin_off == w_boff).all()

    parsed_back = 0
    for g in range(N_BC + 2):
        lo, hi = int(w_boff[g]), int(w_boff[g + 1])
        for first in (0, 1):
            want_text, _ = fw.emit(tb.text, w_recs[lo:hi], w_seq, w_qual, first, 2)
            assert texts[first][g] == want_text, (g, first)
            want = [trimmed[int(r)] for r in w_perm[lo + first:hi:2]]
            assert want_text == b"".join(fw.write(*w) for w in want)
            if want and all(len(w[2]) >= 1 for w in want):  # the reader rejects an empty record
                p = fastq.parse_arrays(texts[first][g])
                assert p.status == "ok" and len(p) == len(want)
                got = [p.record(k) for k in range(len(p))]
                assert [(x._id, x._desc, x._seq, x._qual) for x in got] == want
                parsed_back += 1
    assert parsed_back >= N_BC
    # the two texts of a sample hold the same pairs in the same order
    for g in range(N_BC + 2):
        ids = [[ln.split(b" ")[0] for ln in texts[first][g].split(b"\n")[0::4] if ln] for first in (0, 1)]
        assert ids[0] == ids[1]
