"""What the project writes, it reads back on the device.  bg_bgzf_deflate_dev -> bg_bgzf_blocks_dev -> bg_bgzf_inflate_dev gives
the input back with a block table equal to the deflater's; the compressed sorted BAM file of tests/test_gpu_bam_file_deflate.py
read by `bam.read_bgzf` is the stored file's payload, header plus records; a bgzipped FASTQ of 3 000 reads through
`fastq.parse_bgzf_dev` gives the records, `seq` and `qual` of `parse_dev` on the plain text, and no record for the file of an empty FASTQ."""
import gzip
import random

import numpy as np
import pytest
import torch

import bgzf_deflate_cases as dc
import fastq_write_cases as fw
from dev_shift import guards_intact, shifted, shifted_from
from rust_bio_amd import bam, fastq, sam

pytestmark = pytest.mark.gpu
P = dc.P


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("flags", [0, bam.BGZF_EOF])
def test_deflate_blocks_inflate(flags):
    rng = np.random.default_rng(77)
    for data in (dc.bam_like(), dc.text_of(rng, 2 * P + 77), dc.rand(rng, P + 1), bytes(3 * P), b"a"):
        n_payloads = (len(data) + P - 1) // P
        d_in = shifted_from(data, 5)
        cap = bam.framed_bytes(len(data), flags)
        d_file = shifted(cap, 9)
        d_off = torch.full((n_payloads + 1,), -1, dtype=torch.int64, device="cuda")
        size = bam.bgzf_deflate_dev(d_in.data_ptr(), len(data), d_file.data_ptr(), cap, flags, stream(), d_block_off=d_off.data_ptr())
        n, total = bam.bgzf_blocks_dev(d_file.data_ptr(), size, stream=stream())
        assert (n, total) == (n_payloads + (1 if flags else 0), len(data))
        d_b, d_o = (torch.full((n + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
        assert bam.bgzf_blocks_dev(d_file.data_ptr(), size, d_b.data_ptr(), d_o.data_ptr(), n, stream=stream()) == (n, total)
        assert d_b[:n_payloads + 1].tolist() == d_off.tolist()  # the deflater's table; the end-of-file block follows it
        assert int(d_b[n]) == size and d_o.tolist() == [min(b * P, len(data)) for b in range(n + 1)]
        d_out = shifted(total, 3)
        bam.bgzf_inflate_dev(d_file.data_ptr(), size, n, d_b.data_ptr(), d_o.data_ptr(), d_out.data_ptr(), total, stream=stream())
        assert d_out.cpu().numpy().tobytes() == data and guards_intact(d_out) and guards_intact(d_file)


def test_sorted_bam_read_back():
    from rust_bio_amd.pipeline import PairParams, seed_extend_pairs_mapq_arrays
    from test_gpu_sam_sorted_text import FLAGS, MIN_QUAL, PHRED, SC, case
    B = case()
    p = B.parsed
    params, md = sam.SamParams(FLAGS, 1), sam.MarkdupParams(sam.SAM_PAIRED, 1, PHRED, MIN_QUAL)
    hits, strand, pairs, multi, ops = seed_extend_pairs_mapq_arrays(B.fm, SC, p.seq, p.seq_off, pair_params=PairParams(0, 1000, 17))
    chain = dict(multi=multi, pairs=pairs, markdup=md, ctx=B.fm.ctx)
    stored = bam.sorted_bam(B.fm, params, B.contigs, p, hits, strand, ops, **chain)
    file = bam.sorted_bam(B.fm, params, B.contigs, p, hits, strand, ops, compress=True, **chain)
    plain = bam.read_bgzf(file, ctx=B.fm.ctx)
    assert plain == gzip.decompress(stored) == bam.read_bgzf(stored, ctx=B.fm.ctx)
    assert plain.startswith(bam.header(B.contigs, sam.SAM_SO_COORDINATE)) and len(plain) > len(bam.header(B.contigs, sam.SAM_SO_COORDINATE))


def test_bgzipped_fastq_parses_like_the_plain_text():
    b = fw.Batch(fw.random_records(random.Random(3), 3000, lo=30, hi=151, equal=1.0))
    text, _ = fastq.emit_arrays(b.host())
    file, _ = bam.bgzf_deflate_arrays(text, bam.BGZF_EOF)
    assert len(file) < 0.7 * len(text) and len(text) > 2 * P
    d_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    d_file = torch.from_numpy(np.frombuffer(file, np.uint8).copy()).cuda()
    want = fastq.parse_dev(d_text, stream=stream())
    d_got_text, got = fastq.parse_bgzf_dev(d_file, stream=stream())
    assert d_got_text.cpu().numpy().tobytes() == text
    assert got[:3] == want[:3] == (3000, "ok", want[2])
    n_seq, n_qual = int(want[5][-1]), int(want[7][-1])  # (seq and qual are buffers of the text's size: compare what the offsets cover)
    assert torch.equal(got[3], want[3]) and torch.equal(got[5], want[5]) and torch.equal(got[7], want[7])
    assert torch.equal(got[4][:n_seq], want[4][:n_seq]) and torch.equal(got[6][:n_qual], want[6][:n_qual])


def test_a_bgzipped_fastq_without_reads():
    # what bgzip writes for an empty FASTQ: the end-of-file block alone; and a file of several empty members
    for file in (bam.bgzf_deflate_arrays(b"", bam.BGZF_EOF)[0], bam.bgzf_deflate_arrays(b"", bam.BGZF_EOF)[0] * 3):
        assert len(file) % 28 == 0 and bam.read_bgzf(file) == b""
        d_file = torch.from_numpy(np.frombuffer(file, np.uint8).copy()).cuda()
        d_text, got = fastq.parse_bgzf_dev(d_file, stream=stream())
        assert d_text.numel() == 0 and got[:2] == (0, "ok")
