"""`bg_fastq_trim[_dev]` (csrc/fastq_trim.hip): FASTQ text -> bg_fastq_parse_dev -> bg_myers_best_batch_dev with two
adapters -> bg_fastq_trim_dev, both modes, field by field against the trim rule as a few lines of Python
(tests/myers_oracle.py: trim_range); and one end-to-end case in which trimming is what lets reads with a 3' adapter map
at their origin (bg_seed_extend_strands_batch_dev, bg_sam_emit_batch_dev)."""
import random

import numpy as np
import pytest
import torch

import myers_oracle as mo
from myers_cases import dna, mutated
from rust_bio_amd import _lib, fastq, myers, sam, synth
from rust_bio_amd.bwt import Occ, bwt, less
from rust_bio_amd.fmindex import FMIndex
from rust_bio_amd.pairwise import Scoring
from rust_bio_amd.pipeline import SeedParams, attach_text, seed_extend_strands_dev
from rust_bio_amd.suffix_array import SampledSuffixArray, suffix_array

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ADAPTER3 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"  # 33 symbols
ADAPTER5 = b"GTTCAGAGTTCTACAGTCCGACGATC"
K = 3


def make_records(n=203, seed=5):
    """(sequence, qualities) per record: inserts of 0 .. 80 bases, most with a 3' adapter (whole, cut short, with edits), some
    with the second adapter, some with none; the first and the last record carry an adapter; a few are adapter only (trimmed
    to nothing) and a few have fewer or more quality bytes than bases"""
    rng = random.Random(seed)
    out = []
    for r in range(n):
        insert = dna(rng, rng.randint(20, 80))
        kind = 0 if r in (0, n - 1) else rng.randint(0, 9)
        if r in (0, n - 1):
            seq = insert + ADAPTER3
        elif kind <= 4:
            seq = insert + mutated(rng, ADAPTER3, b"ACGT", rng.choice([0, 0, 0.04]))[:rng.choice([33, 33, 33, 20, 12])]
        elif kind == 5:
            seq = ADAPTER5 + insert
        elif kind == 6:
            seq = ADAPTER5 + insert + ADAPTER3
        elif kind == 7:
            seq = ADAPTER3 + dna(rng, rng.randint(0, 5))  # 3' trim leaves nothing
        else:
            seq = insert
        qual = bytes(rng.randint(33, 73) for _ in range(len(seq)))
        if r % 17 == 3:
            qual = qual[:len(qual) // 2]  # Record::check: UnequalLength; the reader takes it
        if r % 29 == 5:
            qual = qual + b"II"
        out.append((seq, qual))
    return out


def fastq_bytes(records):
    return b"".join(b"@r%d some text\n%s\n+\n%s\n" % (r, s, q) for r, (s, q) in enumerate(records))


def expected(mode, hits, n_pat, parsed):
    """the rule in Python on host columns: (recs, seq, seq_off, qual, qual_off)"""
    recs = parsed.recs.copy()
    seq, qual, so, qo = [], [], [0], [0]
    for r in range(len(recs)):
        s = parsed.seq[int(parsed.seq_off[r]):int(parsed.seq_off[r + 1])].tobytes()
        q = parsed.qual[int(parsed.qual_off[r]):int(parsed.qual_off[r + 1])].tobytes()
        h = [(int(x["score"]), int(x["ystart"]), int(x["yend"])) for x in hits[r * n_pat:(r + 1) * n_pat]]
        (lo, hi), (qlo, qhi) = mo.trim_range(mode, h, len(s), len(q))
        recs[r]["seq_off"], recs[r]["qual_off"], recs[r]["seq_len"], recs[r]["qual_len"] = so[-1], qo[-1], hi - lo, qhi - qlo
        seq.append(s[lo:hi])
        qual.append(q[qlo:qhi])
        so.append(so[-1] + hi - lo)
        qo.append(qo[-1] + qhi - qlo)
    return recs, b"".join(seq), np.array(so, np.uint64), b"".join(qual), np.array(qo, np.uint64)


def same_columns(got, want):
    recs, seq, so, qual, qo = got
    wrecs, wseq, wso, wqual, wqo = want
    for f in _lib.FQREC_DTYPE.names:
        assert (recs[f] == wrecs[f]).all(), f
    assert int(so[0]) == 0 and int(qo[0]) == 0
    assert (np.diff(so.astype(np.int64)) >= 0).all() and (np.diff(qo.astype(np.int64)) >= 0).all()
    assert (so == wso).all() and (qo == wqo).all()
    assert bytes(seq[:int(so[-1])]) == wseq and bytes(qual[:int(qo[-1])]) == wqual


@pytest.mark.parametrize("mode", [mo.TRIM_3P, mo.TRIM_5P], ids=["3p", "5p"])
def test_trim_after_parse_and_match(mode):
    records = make_records()
    fq = fastq_bytes(records)
    n = len(records)
    pats = [myers.Myers(ADAPTER3), myers.Myers(ADAPTER5)]
    stream = torch.cuda.current_stream().cuda_stream
    d_fq = torch.frombuffer(bytearray(fq), dtype=torch.uint8).to(DEV)
    k, status, _, d_recs, d_seq, d_so, d_qual, d_qo = fastq.parse_dev(d_fq)
    assert (k, status) == (n, "ok")
    d_hits, _ = myers.best_batch_dev(pats, d_seq, d_so, K, stream=stream)
    hits = myers.records(d_hits)
    want_hits, _ = mo.best_records([mo.Myers(ADAPTER3), mo.Myers(ADAPTER5)], [s for s, _ in records], K)
    assert hits.tobytes() == want_hits.tobytes()
    parsed = fastq.parse_arrays(fq)
    want = expected(mode, hits, 2, parsed)
    # what the case holds: records without a hit, trimmed to nothing, with unequal lengths; the first and last are trimmed
    lens, src = want[0]["seq_len"].astype(np.int64), parsed.recs["seq_len"].astype(np.int64)
    assert (lens == src).sum() >= 15 and (lens < src).sum() >= 100 and lens[0] < src[0] and lens[-1] < src[-1]
    if mode == mo.TRIM_3P:
        assert (lens == 0).sum() >= 5
    assert (parsed.recs["qual_len"] != parsed.recs["seq_len"]).sum() >= 10
    # the device flavour on what the parse and the match left in HBM
    o_recs, o_seq, o_so, o_qual, o_qo, totals = myers.trim_dev(mode, d_hits, 2, n, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream)
    torch.cuda.synchronize()
    got = (o_recs.cpu().numpy().view(_lib.FQREC_DTYPE), o_seq.cpu().numpy(), o_so.cpu().numpy().astype(np.uint64), o_qual.cpu().numpy(),
           o_qo.cpu().numpy().astype(np.uint64))
    same_columns(got, want)
    assert totals == (len(want[1]), len(want[3]))
    # ... without totals the call does not wait; same outputs
    again = myers.trim_dev(mode, d_hits, 2, n, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream, want_totals=False)
    torch.cuda.synchronize()
    assert again[5] is None and torch.equal(again[2], o_so) and torch.equal(again[0], o_recs)
    # the host flavour
    same_columns(myers.trim(mode, hits, 2, parsed.recs, parsed.seq, parsed.seq_off, parsed.qual, parsed.qual_off), want)
    # one pattern, one read, no read
    one = hits.reshape(n, 2)[:, 0].copy()
    same_columns(myers.trim(mode, one, 1, parsed.recs, parsed.seq, parsed.seq_off, parsed.qual, parsed.qual_off), expected(mode, one, 1, parsed))
    empty = myers.trim(mode, hits[:0], 2, parsed.recs[:0], parsed.seq[:0], parsed.seq_off[:1], parsed.qual[:0], parsed.qual_off[:1])
    assert len(empty[0]) == 0 and list(empty[2]) == [0] and list(empty[4]) == [0]


def test_trimmed_reads_map_where_untrimmed_ones_do_not():
    """reads cut from a 30 kbp reference with a 3' adapter appended: after trimming, every read whose adapter went maps at its
    origin with a CIGAR of its trimmed length; the same reads untrimmed do not all do so"""
    rng = random.Random(11)
    g = synth.random_dna(30_000, seed=41)
    text = np.append(g, np.uint8(ord("$")))
    sa = suffix_array(text)
    b = bwt(text, sa)
    fm = FMIndex(b, less(b, b"ACGTNacgtn$"), Occ(b, 64, b"ACGTNacgtn$"))
    SampledSuffixArray(sa, text, b, 16, fmindex=fm)
    attach_text(fm, text=text)
    n, L = 60, 100
    starts = [rng.randint(0, len(g) - L) for _ in range(n)]
    reads = [g[s:s + L].tobytes() + ADAPTER3 for s in starts]
    fq = fastq_bytes([(s, b"I" * len(s)) for s in reads])
    contigs = sam.Contigs([(b"chr1", 0, len(g))])
    d_contigs = torch.from_numpy(contigs.table.view(np.uint8).copy()).to(DEV)
    d_names = torch.from_numpy(contigs.names).to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    d_fq = torch.frombuffer(bytearray(fq), dtype=torch.uint8).to(DEV)
    k, status, _, d_recs, d_seq, d_so, d_qual, d_qo = fastq.parse_dev(d_fq, ctx=fm.ctx)
    assert (k, status) == (n, "ok")
    d_hits, _ = myers.best_batch_dev([myers.Myers(ADAPTER3)], d_seq, d_so, K, ctx=fm.ctx, stream=stream)
    t_recs, t_seq, t_so, t_qual, t_qo, totals = myers.trim_dev(mo.TRIM_3P, d_hits, 1, n, d_recs, d_seq, d_so, d_qual, d_qo, ctx=fm.ctx,
                                                               stream=stream)
    assert totals == (n * L, n * L)  # every adapter went, nothing else

    def map_and_emit(recs, seq, seq_off, qual, max_len):
        prm = SeedParams(20, 10, 16, 25)
        stride = 2 * max_len + 2 * prm.pad + 4
        d_h = torch.zeros(n * 96, dtype=torch.uint8, device=DEV)
        d_strand = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
        d_ops = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
        seed_extend_strands_dev(fm, Scoring.from_scores(-5, -1, 1, -1), n, seq.data_ptr(), seq_off.data_ptr(), max_len, d_h.data_ptr(),
                                d_strand.data_ptr(), d_ops.data_ptr(), stride, prm, stream=stream)
        torch.cuda.synchronize()
        d_off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
        args = (fm, sam.SamParams(0, 1), n, d_contigs.data_ptr(), 1, d_names.data_ptr(), d_fq.data_ptr(), recs.data_ptr(), seq.data_ptr(),
                qual.data_ptr(), d_h.data_ptr(), d_strand.data_ptr(), d_ops.data_ptr())
        total = sam.emit_dev(*args, 0, 0, d_off.data_ptr(), stream=stream)
        d_out = torch.zeros(total, dtype=torch.uint8, device=DEV)
        assert sam.emit_dev(*args, d_out.data_ptr(), total, d_off.data_ptr(), stream=stream) == total
        torch.cuda.synchronize()
        lines = [ln.split(b"\t") for ln in d_out.cpu().numpy().tobytes().splitlines()]
        assert len(lines) == n
        return lines

    def at_origin(lines):
        return [int(ln[1]) & 4 == 0 and int(ln[3]) == starts[r] + 1 and ln[5] == b"%d=" % L for r, ln in enumerate(lines)]

    trimmed = map_and_emit(t_recs, t_seq, t_so, t_qual, L)
    assert all(at_origin(trimmed))
    assert all(ln[9] == reads[r][:L] and len(ln[10]) == L for r, ln in enumerate(trimmed))  # SEQ and QUAL are the trimmed ones
    untrimmed = map_and_emit(d_recs, d_seq, d_so, d_qual, L + len(ADAPTER3))
    assert not all(at_origin(untrimmed))
    fm.close()
