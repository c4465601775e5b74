"""The front of the pipeline end to end, nothing crossing to the host in between: interleaved paired FASTQ text ->
bg_fastq_parse_dev -> bg_myers_best_batch_dev (a 3' adapter) -> bg_fastq_trim_dev -> bg_fastq_filter_dev (pairs, at least 20
bases) -> bg_fastq_emit_dev twice (R1 and R2 texts).  Compared with the same steps on the oracle's records: the reader of the
CPU oracle, the Myers restatement, the trim rule, the filter rule and `Writer::write` in Python."""
import random

import numpy as np
import pytest
import torch

import fastq_write_oracle as fw
import myers_oracle as mo
import oracle_py as orc
from myers_cases import dna
from rust_bio_amd import _lib, fastq, myers, sam, synth
from rust_bio_amd.bwt import Occ, bwt, less
from rust_bio_amd.fmindex import FMIndex
from rust_bio_amd.suffix_array import suffix_array

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ADAPTER3 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"  # 33 symbols
K, MIN_LEN, N = 3, 20, 2000


def make_reads(seed=21):
    """N interleaved mates of 20 .. 150 bases; a third carry the adapter at a random position (the rest of the read follows it
    as far as the read goes), every 40th of those at position 0"""
    rng = random.Random(seed)
    reads = []
    for r in range(N):
        ln = rng.randint(20, 150)
        s = dna(rng, ln)
        if rng.random() < 1 / 3 or r == 6:
            pos = 0 if rng.random() < 1 / 40 or r == 6 else rng.randint(0, ln - 1)
            s = (s[:pos] + ADAPTER3 + dna(rng, ln))[:max(ln, pos + len(ADAPTER3))][:150]
        reads.append((b"pair%d" % (r // 2), b"%d:N:0" % (r % 2 + 1), s, bytes(rng.randint(33, 73) for _ in range(len(s)))))
    return reads


def test_trim_filter_and_write_paired_reads():
    reads = make_reads()
    fq = b"".join(fw.write(*r) for r in reads)
    stream = torch.cuda.current_stream().cuda_stream
    d_fq = torch.frombuffer(bytearray(fq), dtype=torch.uint8).to(DEV)
    n, status, _, d_recs, d_seq, d_so, d_qual, d_qo = fastq.parse_dev(d_fq, stream=stream)
    assert (n, status) == (N, "ok")
    d_hits, _ = myers.best_batch_dev([myers.Myers(ADAPTER3)], d_seq, d_so, K, stream=stream)
    t_recs, t_seq, t_so, t_qual, t_qo, _ = myers.trim_dev(myers.TRIM_3P, d_hits, 1, n, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream,
                                                          want_totals=False)
    f_recs, f_seq, f_so, f_qual, f_qo, d_keep, totals = fastq.filter_dev(n, t_recs, t_seq, t_so, t_qual, t_qo, flags=fastq.FQF_PAIRED,
                                                                         min_len=MIN_LEN, stream=stream, want_keep=True)
    kept = totals[0]
    r1, r1_off, _ = fastq.emit_dev(kept, d_fq, f_recs, f_seq, f_qual, 0, 2, stream=stream)
    r2, r2_off, _ = fastq.emit_dev(kept, d_fq, f_recs, f_seq, f_qual, 1, 2, stream=stream)
    torch.cuda.synchronize()

    # the same on the oracle's records
    want_recs, wst, _ = orc.fastq_parse(fq)
    assert wst == "ok" and [(w["id"], w["desc"], w["seq"], w["qual"]) for w in want_recs] == reads
    hits, _ = mo.best_records([mo.Myers(ADAPTER3)], [r[2] for r in reads], K)
    assert myers.records(d_hits).tobytes() == hits.tobytes()
    trimmed = []
    for r, (id_, desc, s, q) in enumerate(reads):
        (lo, hi), (qlo, qhi) = mo.trim_range(mo.TRIM_3P, [(int(hits[r]["score"]), int(hits[r]["ystart"]), int(hits[r]["yend"]))], len(s), len(q))
        trimmed.append((id_, desc, s[lo:hi], q[qlo:qhi]))
    passed = [fw.passes(t[2], 0, False, min_len=MIN_LEN) for t in trimmed]
    keep = fw.keep_flags(passed, fw.PAIRED)
    # what the case holds: reads cut, reads cut to nothing, pairs that go because of one mate, pairs that stay
    cut = [len(t[2]) < len(r[2]) for t, r in zip(trimmed, reads)]
    assert sum(cut) > 400 and sum(len(t[2]) == 0 for t in trimmed) >= 5 and len(trimmed[6][2]) == 0
    assert sum(p and not k for p, k in zip(passed, keep)) >= 20 and 600 < sum(keep) < N and sum(keep) % 2 == 0
    assert bytes(d_keep.cpu().numpy()[:n]) == bytes(keep) and kept == sum(keep)
    want_r1 = b"".join(fw.write(*trimmed[r]) for r in range(0, N, 2) if keep[r])
    want_r2 = b"".join(fw.write(*trimmed[r]) for r in range(1, N, 2) if keep[r])
    got_r1, got_r2 = r1.cpu().numpy().tobytes(), r2.cpu().numpy().tobytes()
    assert got_r1 == want_r1 and got_r2 == want_r2
    assert int(r1_off[-1]) == len(want_r1) and r1_off.numel() == r2_off.numel() == kept // 2 + 1

    # each text parses again on the device: the kept mates, ids pairwise equal, nothing shorter than 20
    cols = []
    for d_text, mate in ((r1, 0), (r2, 1)):
        k, status, _, p_recs, p_seq, p_so, p_qual, p_qo = fastq.parse_dev(d_text, stream=stream)
        torch.cuda.synchronize()
        assert (k, status) == (kept // 2, "ok")
        recs = p_recs.cpu().numpy().view(_lib.FQREC_DTYPE)
        assert (recs["check"] == 0).all() and recs["seq_len"].min() >= MIN_LEN and (recs["seq_len"] == recs["qual_len"]).all()
        text = d_text.cpu().numpy().tobytes()
        seq = p_seq.cpu().numpy().tobytes()
        ids = [text[int(c["id_off"]):int(c["id_off"] + c["id_len"])] for c in recs]
        seqs = [seq[int(c["seq_off"]):int(c["seq_off"] + c["seq_len"])] for c in recs]
        want = [trimmed[r] for r in range(mate, N, 2) if keep[r]]
        assert ids == [w[0] for w in want] and seqs == [w[2] for w in want]
        cols.append(ids)
    assert cols[0] == cols[1]

    # the filtered records are still what the SAM writer takes: ids resolve into the original text
    g = synth.random_dna(2_000, seed=3)
    ref = np.append(g, np.uint8(ord("$")))
    sa = suffix_array(ref)
    b = bwt(ref, sa)
    fm = FMIndex(b, less(b, b"ACGTNacgtn$"), Occ(b, 64, b"ACGTNacgtn$"))
    contigs = sam.Contigs([(b"chr1", 0, len(g))])
    d_contigs = torch.from_numpy(contigs.table.view(np.uint8).copy()).to(DEV)
    d_names = torch.from_numpy(contigs.names).to(DEV)
    unplaced = np.zeros(kept, dtype=_lib.SEED_HIT_DTYPE)
    unplaced["aln"]["score"] = _lib.MIN_SCORE
    d_h = torch.from_numpy(unplaced.view(np.uint8).copy()).to(DEV)
    d_strand = torch.full((kept,), _lib.HIT_NONE, dtype=torch.uint8, device=DEV)
    d_ops = torch.zeros(16, dtype=torch.uint8, device=DEV)
    d_off = torch.zeros(kept + 1, dtype=torch.int64, device=DEV)
    args = (fm, sam.SamParams(0, 1), kept, d_contigs.data_ptr(), 1, d_names.data_ptr(), d_fq.data_ptr(), f_recs.data_ptr(), f_seq.data_ptr(),
            f_qual.data_ptr(), d_h.data_ptr(), d_strand.data_ptr(), d_ops.data_ptr())
    total = sam.emit_dev(*args, 0, 0, d_off.data_ptr(), stream=stream)
    d_out = torch.zeros(total, dtype=torch.uint8, device=DEV)
    assert sam.emit_dev(*args, d_out.data_ptr(), total, d_off.data_ptr(), stream=stream) == total
    torch.cuda.synchronize()
    lines = [ln.split(b"\t") for ln in d_out.cpu().numpy().tobytes().splitlines()]
    want = [trimmed[r] for r in range(N) if keep[r]]
    assert [(ln[0], ln[9], ln[10]) for ln in lines] == [(w[0], w[2], w[3]) for w in want]
    fm.close()
