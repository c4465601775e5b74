"""Reading back what the library writes, and what it did not write, on the batch of tests/test_gpu_bam_file_index.py:
`bam.sorted_bam(..., index=True)` -> `bam.read_bam` gives the header, the contigs and the record table; `bam.index_bam` of the
file's bytes alone is the .bai written with it, stored and compressed; the keys of the records are the keys of the hits; the reads
come back as they were sequenced; an unmapped-only BAM of a parsed FASTQ gives its FASTQ text back.  The same records in a
foreign framing (members of 1, 7, 4 096 and 65 536 payload bytes in rotation, empty members between, zlib level 6) are indexed as
tests/bai_oracle.py indexes them with the virtual offsets of tests/bam_read_oracle.py, and a reader finds its records."""
import gzip
import struct

import numpy as np
import pytest
import torch

import bai_oracle as ba
import bam_oracle as bo
import bam_read_oracle as ro
import bgzf_inflate_cases as ic
from rust_bio_amd import bam, fastq, sam
from rust_bio_amd.pipeline import PairParams, seed_extend_pairs_mapq_arrays
from test_gpu_bam_file_index import read_chunk
from test_gpu_sam_sorted_text import FLAGS, MIN_QUAL, PHRED, SC, case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mapped():
    B = case()
    p = B.parsed
    params, md = sam.SamParams(FLAGS, 1), sam.MarkdupParams(sam.SAM_PAIRED, 1, PHRED, MIN_QUAL)
    hits, strand, pairs, multi, ops = seed_extend_pairs_mapq_arrays(B.fm, SC, p.seq, p.seq_off, pair_params=PairParams(0, 1000, 17))
    chain = dict(multi=multi, pairs=pairs, markdup=md, ctx=B.fm.ctx)
    files = {c: bam.sorted_bam(B.fm, params, B.contigs, p, hits, strand, ops, compress=c, index=True, **chain) for c in (False, True)}
    return dict(B=B, p=p, params=params, hits=hits, strand=strand, pairs=pairs, multi=multi, ops=ops, files=files)


def entries_of(contigs):
    return [(contigs.name(c), int(contigs.table["start"][c]), int(contigs.table["len"][c])) for c in range(len(contigs))]


def test_read_bam_gives_the_header_and_the_record_table(mapped):
    B = mapped["B"]
    head = bam.header(B.contigs, sam.SAM_SO_COORDINATE)
    for compress, (file, _) in mapped["files"].items():
        text, contigs, stream, off = bam.read_bam(file, ctx=B.fm.ctx)
        assert stream == gzip.decompress(file) and stream[:len(head)] == head
        assert text == sam.header(B.contigs, sam.SAM_SO_COORDINATE)
        assert entries_of(contigs) == [tuple(e) for e in B.entries] == entries_of(B.contigs)
        recs = bo.split_records(stream[len(head):])
        assert off.tolist() == (bo.offsets(recs) + np.uint64(len(head))).tolist() and len(recs) > 100


def test_index_bam_is_the_bai_written_with_the_file(mapped):
    for compress, (file, bai) in mapped["files"].items():
        assert bam.index_bam(file, ctx=mapped["B"].fm.ctx) == bai, compress


def test_keys_of_the_records_are_the_keys_of_the_hits(mapped):
    B, p = mapped["B"], mapped["p"]
    recs, off = bam.emit_arrays(B.fm, mapped["params"], B.contigs, p, mapped["hits"], mapped["strand"], mapped["ops"], multi=mapped["multi"], pairs=mapped["pairs"])
    want = sam.sort_keys_arrays(mapped["params"], B.contigs, len(p.recs), mapped["hits"], mapped["strand"], ctx=B.fm.ctx)
    _, contigs, _ = bam.read_header(bam.header(B.contigs))
    got = bam.sort_keys_records_arrays(recs, off, contigs, ctx=B.fm.ctx)
    wrote = np.diff(off.astype(np.int64)) > 0
    assert wrote.sum() > 100 and (got[wrote] == want[wrote]).all() and (got[~wrote] == np.uint64(2**64 - 1)).all()
    assert (got != np.uint64(2**64 - 1)).sum() > 50


def test_the_reads_come_back_as_they_were_sequenced(mapped):
    B, p = mapped["B"], mapped["p"]
    recs, off = bam.emit_arrays(B.fm, mapped["params"], B.contigs, p, mapped["hits"], mapped["strand"], mapped["ops"], multi=mapped["multi"], pairs=mapped["pairs"])
    key = sam.sort_keys_arrays(mapped["params"], B.contigs, len(p.recs), mapped["hits"], mapped["strand"], ctx=B.fm.ctx)
    body, body_off, perm = sam.sort_arrays(key, recs, off, ctx=B.fm.ctx)
    slots = [int(s) for s in perm if off[int(s) + 1] > off[int(s)]]  # the slot of the i-th record of the sorted stream
    table = ro.walk(body, 0, len(B.contigs))
    assert len(table) - 1 == len(slots)
    r, seq, seq_off, qual, qual_off, src = bam.reads_arrays(body, table, len(B.contigs), flags=bam.BAM_READS_ORIGINAL, exclude=0x900, ctx=B.fm.ctx)
    assert len(r) == len(p.recs)  # (K = 1: one primary record a read)
    n_rev = 0
    for j in range(len(r)):
        read = slots[int(src[j])]
        assert seq[int(seq_off[j]):int(seq_off[j + 1])].tobytes() == p.seq[int(p.seq_off[read]):int(p.seq_off[read + 1])].tobytes().upper(), j
        assert qual[int(qual_off[j]):int(qual_off[j + 1])].tobytes() == p.qual[int(p.qual_off[read]):int(p.qual_off[read + 1])].tobytes(), j
        n_rev += (struct.unpack_from("<H", body, table[int(src[j])] + 18)[0] >> 4) & 1
    assert n_rev > 20


def test_an_unmapped_bam_of_a_fastq_gives_the_fastq_back():
    rng = np.random.default_rng(11)
    text = b""
    for i in range(300):
        n = int(rng.integers(1, 200))
        text += b"@read%d\n%s\n+\n%s\n" % (i, bytes(rng.choice(list(b"ACGTN"), n).astype(np.uint8)), bytes(rng.integers(33, 74, n).astype(np.uint8)))
    p = fastq.parse_arrays(text)
    lines = [b"%s\t%d\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\n" % (x._id, 77 if k % 2 == 0 else 141, x._seq, x._qual) for k, x in enumerate(p.record(k) for k in range(len(p)))]
    stream = bo.header(b"@HD\tVN:1.6\tSO:unsorted\n", []) + b"".join(bo.records(lines, []))
    file = ic.bgzf(stream)
    d_file = torch.from_numpy(np.frombuffer(file, np.uint8).copy()).cuda()
    d_stream, (k, d_recs, d_seq, d_so, d_qual, d_qo, d_src) = fastq.parse_bam_dev(d_file)
    assert k == 300 and d_src.cpu().tolist() == list(range(300)) and d_stream.cpu().numpy().tobytes() == stream
    d_text, _, _ = fastq.emit_dev(k, d_stream, d_recs, d_seq, d_qual)
    assert d_text.cpu().numpy().tobytes() == text


def foreign(stream):
    """`stream` framed by another writer: payloads of 1, 7, 4 096 and 65 536 bytes in rotation at zlib level 6, an empty member
    after every fourth and in front, the end-of-file block"""
    out, at, k = [ic.member(b"")], 0, 0
    sizes = (1, 7, 4096, 65536)
    while at < len(stream):
        n = sizes[k % 4]
        out.append(ic.member(stream[at:at + n], 6))
        if k % 4 == 3:
            out.append(ic.member(b""))
        at += n
        k += 1
    return b"".join(out) + ic.EOF_BLOCK


def test_a_foreign_framing(mapped):
    B = mapped["B"]
    file, _ = mapped["files"][True]
    stream = gzip.decompress(file)
    other = foreign(stream)
    assert gzip.decompress(other) == stream
    head = bam.header(B.contigs, sam.SAM_SO_COORDINATE)
    recs = bo.split_records(stream[len(head):])
    rcode, block_off, out_off, _ = ic.walk(other)
    assert rcode == 0 and len(block_off) > 6 and 0 in np.diff(out_off)
    voff = ro.blocks_voff(block_off, out_off)
    entries = [tuple(e) for e in B.entries]
    want = ba.build(recs, entries, lambda o: voff(o + len(head)))
    bai = bam.index_bam(other, ctx=B.fm.ctx)
    assert bai == want
    parsed = ba.parse(bai)
    for c, (_, _, ln) in enumerate(entries):
        mine = [r for r in recs if struct.unpack_from("<i", r, 4)[0] == c]
        vb, ve = parsed[0][c]["meta"][:2]
        assert bo.split_records(read_chunk(other, vb, ve)) == mine and mine
        for beg, end in ((0, ln), (ln // 2, ln // 2 + 150), (16383, 16385)):
            found = []
            for b, e in ba.query(parsed, c, beg, end):
                found += bo.split_records(read_chunk(other, b, e))
            for r in mine:
                f = ba.fields(r, entries)
                if f[1] < end and f[2] > beg:
                    assert r in found, (c, beg, end)
