"""A compressed coordinate-sorted BAM file on the batch of tests/test_gpu_bam_file.py: `bam.sorted_bam(..., compress=True)` holds
the same payloads as the stored file (gzip.decompress of both is equal), ends in the end-of-file block and is smaller; and
`bam.virtual_offsets` through the block table of bg_bgzf_deflate leads to three records: the one block at v >> 16 is
decompressed and the record found at v & 0xFFFF."""
import gzip
import struct

import pytest

import bam_oracle as bo
from rust_bio_amd import bam, sam
from rust_bio_amd.pipeline import PairParams, seed_extend_pairs_mapq_arrays
from test_gpu_sam_sorted_text import FLAGS, MIN_QUAL, PHRED, SC, case

pytestmark = pytest.mark.gpu


def test_sorted_bam_compressed():
    B = case()
    p = B.parsed
    params, md = sam.SamParams(FLAGS, 1), sam.MarkdupParams(sam.SAM_PAIRED, 1, PHRED, MIN_QUAL)
    hits, strand, pairs, multi, ops = seed_extend_pairs_mapq_arrays(B.fm, SC, p.seq, p.seq_off, pair_params=PairParams(0, 1000, 17))
    chain = dict(multi=multi, pairs=pairs, markdup=md, ctx=B.fm.ctx)
    stored = bam.sorted_bam(B.fm, params, B.contigs, p, hits, strand, ops, **chain)
    assert stored == bam.sorted_bam(B.fm, params, B.contigs, p, hits, strand, ops, compress=False, **chain)
    file = bam.sorted_bam(B.fm, params, B.contigs, p, hits, strand, ops, compress=True, **chain)
    plain = gzip.decompress(file)
    assert plain == gzip.decompress(stored)
    assert file.endswith(bo.EOF_BLOCK) and len(file) < len(stored)
    # virtual offsets through the block table: the header's blocks, then the records'
    head = bam.header(B.contigs, sam.SAM_SO_COORDINATE)
    body = plain[len(head):]
    framed_head, head_off = bam.bgzf_deflate_arrays(head, 0, ctx=B.fm.ctx)
    framed_body, body_off = bam.bgzf_deflate_arrays(body, bam.BGZF_EOF, ctx=B.fm.ctx)
    assert file == framed_head + framed_body and int(head_off[-1]) == len(framed_head) and int(body_off[-1]) == len(framed_body) - 28
    recs = bo.split_records(body)
    off = bo.offsets(recs)
    picks = (0, len(recs) // 2, len(recs) - 1)
    for i, v in zip(picks, bam.virtual_offsets([int(off[i]) for i in picks], body_off, base=len(framed_head)).tolist()):
        at, within = v >> 16, v & 0xFFFF
        bsize, = struct.unpack_from("<H", file, at + 16)
        payload = gzip.decompress(file[at:at + bsize + 1])
        assert within < len(payload) and payload[within:within + len(recs[i])] == recs[i][:len(payload) - within], i  # (a record may end in the next block)
