"""A genome file's bytes to SAM without a host parser: FASTA and FASTQ text in HBM -> bg_fasta_parse_dev ->
bg_fasta_reference_dev (FMD | UPPER) -> bg_suffix_array_dev, bg_bwt_dev, bg_sa_sample_dev, bg_fm_build_dev ->
bg_seed_extend_smem_batch_dev -> bg_sam_emit_batch_dev, with the builder's text, contig table and names taken as they are.
Header and body must equal, byte for byte, what the same calls produce from a host-concatenated T$R$ and a hand-made
sam.Contigs.  One small case: three soft-masked contigs of 2 - 4 kbp wrapped at 60 columns, 40 reads on both strands."""
import numpy as np
import pytest
import torch

import fmd_cases as fc
from rust_bio_amd import fasta, fastq, sam, synth
from rust_bio_amd.fmindex import FMIndex
from rust_bio_amd.pairwise import Scoring
from rust_bio_amd.pipeline import SmemSeedParams, attach_text, seed_extend_smem_dev
from rust_bio_amd.suffix_array import bwt_dev, sample_dev, suffix_array_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SC = Scoring.from_scores(-5, -1, 1, -1)
PRM = SmemSeedParams(19, 16, 16, 25)
NAMES = (b"chr1", b"chr2", b"chrM")
N_READS, READ_LEN = 40, 100


def contigs_and_files():
    """(upper-case contigs, FASTA bytes with lower-case stretches, FASTQ bytes of reads from them)"""
    rng = np.random.default_rng(17)
    seqs = [fc.random_dna(n, 50 + k) for k, n in enumerate((2000, 4000, 3001))]
    fa = b""
    for name, s in zip(NAMES, seqs):
        m = bytearray(s)
        for _ in range(4):  # soft-masked repeats
            a = int(rng.integers(0, len(s) - 300))
            m[a:a + 250] = bytes(m[a:a + 250]).lower()
        fa += b">" + name + b" a contig of %d bases\n" % len(s) + b"".join(bytes(m[a:a + 60]) + b"\n" for a in range(0, len(m), 60))
    # the first 40 reads of synth.fm_patterns (exact substrings, a fifth with 1 - 3 substitutions), drawn contig by contig so
    # that none runs over a '$'; every odd one reverse complemented
    reads = []
    for k, s in enumerate(seqs):
        pat, off = synth.fm_patterns(np.frombuffer(s + b"$", np.uint8), 14, READ_LEN, seed=70 + k)
        reads += [pat[int(off[j]):int(off[j + 1])].tobytes() for j in range(14)]
    fq = b""
    for r, read in enumerate(reads[:N_READS]):
        if r % 2:
            read = fc.revcomp(read)
        fq += b"@read%d\n" % r + read + b"\n+\n" + bytes(rng.integers(33, 74, size=READ_LEN).astype(np.uint8)) + b"\n"
    return seqs, fa, fq


def map_and_emit(d_text, d_contigs, d_names, contigs, d_fq):
    """index of d_text (T$R$) built on the device, the reads mapped with SMEM seeds, SAM written: (header, body)"""
    stream = torch.cuda.current_stream().cuda_stream
    d_sa = suffix_array_dev(d_text)
    d_b = bwt_dev(d_text, d_sa)
    fm = FMIndex.from_device(d_b, 3, fc.ALPHA)
    sample_dev(d_sa, d_b, ord("$"), 8).attach(fm)
    attach_text(fm, d_text=d_text)
    n, status, _, d_recs, d_seq, d_seq_off, d_qual, _ = fastq.parse_dev(d_fq)
    assert (n, status) == (N_READS, "ok")
    stride = 2 * READ_LEN + 2 * PRM.pad + 4
    d_hits = torch.zeros(n * 96, dtype=torch.uint8, device=DEV)
    d_strand = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
    d_ops = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
    seed_extend_smem_dev(fm, SC, n, d_seq.data_ptr(), d_seq_off.data_ptr(), READ_LEN, d_hits.data_ptr(), d_strand.data_ptr(), d_ops.data_ptr(),
                         stride, PRM, stream=stream)
    torch.cuda.synchronize()
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    args = (fm, sam.SamParams(sam.SAM_TAG_NM | sam.SAM_TAG_MD, 1), n, d_contigs.data_ptr(), len(contigs), d_names.data_ptr(), d_fq.data_ptr(),
            d_recs.data_ptr(), d_seq.data_ptr(), d_qual.data_ptr(), d_hits.data_ptr(), d_strand.data_ptr(), d_ops.data_ptr())
    total = sam.emit_dev(*args, 0, 0, d_off.data_ptr(), stream=stream)
    d_out = torch.zeros(total, dtype=torch.uint8, device=DEV)
    assert sam.emit_dev(*args, d_out.data_ptr(), total, d_off.data_ptr(), stream=stream) == total
    torch.cuda.synchronize()
    body = d_out.cpu().numpy().tobytes()
    fm.close()
    return sam.header(contigs), body


def test_fasta_bytes_to_sam_equal_the_hand_made_reference():
    seqs, fa, fq = contigs_and_files()
    d_fq = torch.frombuffer(bytearray(fq), dtype=torch.uint8).to(DEV)
    # the path under test: nothing of the reference is built on the host
    d_fa = torch.frombuffer(bytearray(fa), dtype=torch.uint8).to(DEV)
    n, status, _, d_recs, d_seq, _ = fasta.parse_dev(d_fa)
    assert (n, status) == (3, "ok")
    d_text, d_contigs, d_names, contigs = fasta.reference_dev(n, d_recs, d_fa, d_seq, fasta.REF_FMD | fasta.REF_UPPER)
    got = map_and_emit(d_text, d_contigs, d_names, contigs, d_fq)
    # the existing path: T$R$ concatenated on the host, the contig table written by hand
    text = np.frombuffer(fc.full_text(b"$".join(seqs)), np.uint8)
    starts = np.cumsum([0] + [len(s) + 1 for s in seqs])
    hand = sam.Contigs([(name, int(starts[k]), len(s)) for k, (name, s) in enumerate(zip(NAMES, seqs))])
    assert d_text.cpu().numpy().tobytes() == text.tobytes()
    want = map_and_emit(torch.from_numpy(text.copy()).to(DEV), torch.from_numpy(hand.table.view(np.uint8).copy()).to(DEV),
                        torch.from_numpy(hand.names).to(DEV), hand, d_fq)
    assert got[0] == want[0] and got[0].count(b"@SQ") == 3
    assert got[1] == want[1]
    # the case is not vacuous: the reads are placed, on both strands and on every contig
    lines = [ln.split(b"\t") for ln in got[1].splitlines()]
    assert len(lines) == N_READS
    placed = [ln for ln in lines if not int(ln[1]) & 4]
    assert len(placed) >= 36 and {int(ln[1]) & 16 for ln in placed} == {0, 16} and {ln[2] for ln in placed} == set(NAMES)
