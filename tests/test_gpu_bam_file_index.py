"""A coordinate-sorted BAM file with its BAI index, end to end, on the batch of tests/test_gpu_bam_file_deflate.py:
`bam.sorted_bam(..., index=True)`, stored and compressed.  The file is today's file byte for byte; the index is read by
tests/bai_oracle.py's reader, and for every contig and a handful of regions the chunks `query` lists are followed through the
file as a reader would — seek to v >> 16, inflate that block and its successors, start at v & 0xFFFF, stop at the chunk's end —:
what lies there splits into whole records, and they include every record that overlaps the region according to
bam_oracle.decode.  The pseudo-bins' counts and n_no_coor are the counts of the decoded file."""
import gzip
import struct

import pytest

import bai_oracle as ba
import bam_oracle as bo
from rust_bio_amd import bam, sam
from rust_bio_amd.pipeline import PairParams, seed_extend_pairs_mapq_arrays
from test_gpu_sam_sorted_text import FLAGS, MIN_QUAL, PHRED, SC, case

pytestmark = pytest.mark.gpu


def read_chunk(file, beg, end):
    """the bytes between two virtual offsets"""
    at, within, out = beg >> 16, beg & 0xFFFF, b""
    while True:
        bsize, = struct.unpack_from("<H", file, at + 16)
        payload = gzip.decompress(file[at:at + bsize + 1])
        if at == end >> 16:
            assert within <= (end & 0xFFFF) <= len(payload)
            return out + payload[within:end & 0xFFFF]
        assert at < end >> 16
        out += payload[within:]
        at, within = at + bsize + 1, 0


def test_sorted_bam_with_its_index():
    B = case()
    p = B.parsed
    params, md = sam.SamParams(FLAGS, 1), sam.MarkdupParams(sam.SAM_PAIRED, 1, PHRED, MIN_QUAL)
    hits, strand, pairs, multi, ops = seed_extend_pairs_mapq_arrays(B.fm, SC, p.seq, p.seq_off, pair_params=PairParams(0, 1000, 17))
    chain = dict(multi=multi, pairs=pairs, markdup=md, ctx=B.fm.ctx)
    head = bam.header(B.contigs, sam.SAM_SO_COORDINATE)
    for compress in (False, True):
        today = bam.sorted_bam(B.fm, params, B.contigs, p, hits, strand, ops, compress=compress, **chain)
        file, bai = bam.sorted_bam(B.fm, params, B.contigs, p, hits, strand, ops, compress=compress, index=True, **chain)
        assert file == today and isinstance(today, bytes)
        recs = bo.split_records(gzip.decompress(file)[len(head):])
        where = []  # (refID, pos, end, unmapped) from the decoder's fields
        for r in recs:
            f = bo.decode(r, B.entries)
            ref = -1 if f[2] == b"*" else [e[0] for e in B.entries].index(f[2])
            pos = int(f[3]) - 1
            where.append((ref, pos, pos + (bo.ref_length(bo.cigar_words(f[5])) or 1), bool(int(f[1]) & 4)))
        parsed = ba.parse(bai)
        refs, n_no_coor = parsed
        assert len(refs) == len(B.entries) and n_no_coor == sum(1 for w in where if w[0] < 0) > 0
        for c, (_, _, ln) in enumerate(B.entries):
            mine = [w for w in where if w[0] == c]
            assert mine and refs[c]["meta"][2:] == (sum(1 for w in mine if not w[3]), sum(1 for w in mine if w[3])), (compress, c)
            first = min(w[1] for w in mine)
            regions = [(0, ln), (0, 1), (first, first + 1), (ln // 2, ln // 2 + 150), (ln - 1, ln), (16383, 16385), (16384, 2 * 16384), (700, 700)]
            for beg, end in regions:
                found = []
                for vb, ve in ba.query(parsed, c, beg, end):
                    found += bo.split_records(read_chunk(file, vb, ve))  # (asserts that the chunk is whole records)
                for r, w in zip(recs, where):
                    if w[0] == c and beg < end and w[1] < end and w[2] > beg:
                        assert r in found, (compress, c, beg, end, w)
            assert ba.query(parsed, c, 700, 700) == []
            # the pseudo-bin's first chunk spans the contig's records
            vb, ve = refs[c]["meta"][:2]
            assert bo.split_records(read_chunk(file, vb, ve)) == [r for r, w in zip(recs, where) if w[0] == c]
