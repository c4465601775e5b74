"""A coordinate-sorted BAM file with duplicate flags, end to end, on the batch of tests/test_gpu_sam_sorted_text.py:
`bam.sorted_bam` (markdup -> BAM records -> keys -> bg_sam_sort -> two bg_bgzf_frame calls) -> gzip.decompress -> the oracle's
decoder.  The decoded records must be the fields of `sam.sorted_sam`'s lines in the same order, (refID, pos) ascending with the
unmapped records last, under the BAM header of the same contigs; `bam.virtual_offset` of three records must lead to them; and
the device entry points chained by hand give the same bytes."""
import gzip
import struct

import numpy as np
import pytest
import torch

import bam_oracle as bo
import sam_edge_cases as ec
import sam_oracle as so
from rust_bio_amd import bam, sam
from rust_bio_amd.pipeline import PairParams, seed_extend_pairs_mapq_arrays
from test_gpu_sam_emit import DEV
from test_gpu_sam_sorted_text import FLAGS, MIN_QUAL, PHRED, SC, case

pytestmark = pytest.mark.gpu


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(DEV)


def test_sorted_bam():
    B = case()
    p = B.parsed
    params, md = sam.SamParams(FLAGS, 1), sam.MarkdupParams(sam.SAM_PAIRED, 1, PHRED, MIN_QUAL)
    hits, strand, pairs, multi, ops = seed_extend_pairs_mapq_arrays(B.fm, SC, p.seq, p.seq_off, pair_params=PairParams(0, 1000, 17))
    chain = dict(multi=multi, pairs=pairs, markdup=md, ctx=B.fm.ctx)
    text = sam.sorted_sam(B.fm, params, B.contigs, p, hits, strand, ops, **chain)
    file = bam.sorted_bam(B.fm, params, B.contigs, p, hits, strand, ops, **chain)
    head_text = sam.header(B.contigs, sam.SAM_SO_COORDINATE)
    lines = [ln + b"\n" for ln in text[len(head_text):].split(b"\n")[:-1]]
    assert len(lines) == B.n and sum(int(ec.fields(ln)[1]) & 0x400 > 0 for ln in lines) >= 8
    # the container: a valid gzip stream that ends in the end-of-file block
    assert file.endswith(bo.EOF_BLOCK)
    plain = gzip.decompress(file)
    want_head = bo.header(head_text, B.entries)
    assert bam.header(B.contigs, sam.SAM_SO_COORDINATE) == want_head and plain.startswith(want_head)
    body = plain[len(want_head):]
    assert file == bo.frame(want_head) + bo.frame(body, True)
    # the records: the lines' fields, in the lines' order, sorted
    recs = bo.split_records(body)
    assert recs == bo.records(lines, B.entries)
    assert [bo.decode(r, B.entries) for r in recs] == [ec.fields(ln) for ln in lines]
    where = [struct.unpack_from("<ii", r, 4) for r in recs]
    order = [(c if c >= 0 else len(B.entries), pos) for c, pos in where]
    assert order == sorted(order) and order[0][0] == 0 and order[-1][0] == len(B.entries)
    # virtual offsets: the block at the file offset, then the byte inside its payload
    base = bam.framed_bytes(len(want_head))
    off = bo.offsets(recs)
    for i in (0, len(recs) // 2, len(recs) - 1):
        v = bam.virtual_offset(int(off[i]), base)
        at, within = v >> 16, v & 0xFFFF
        bsize, = struct.unpack_from("<H", file, at + 16)
        payload = gzip.decompress(file[at:at + bsize + 1])
        assert payload[within:within + len(recs[i])] == recs[i], i
    assert bam.virtual_offset(65280 + 5, 100) == ((100 + 65311) << 16) | 5
    # the device entry points chained by hand: records, keys, the permuted copy, the framing, nothing on the host in between
    stream = torch.cuda.current_stream().cuda_stream
    n, n_contigs = B.n, len(B.contigs)
    dup, _ = sam.markdup_arrays(md, B.contigs, p, hits, strand, ctx=B.fm.ctx)
    d_hits, d_strand, d_ops, d_multi, d_pairs, d_dup = (dev(x) for x in (hits, strand, ops, multi, pairs, dup))
    emit = (B.fm, params, n, B.d_contigs.data_ptr(), n_contigs, B.d_names.data_ptr(), B.d_fq.data_ptr(), B.d_recs.data_ptr(), B.d_seq.data_ptr(),
            B.d_qual.data_ptr(), d_hits.data_ptr(), d_strand.data_ptr(), d_ops.data_ptr())
    kw = dict(d_multi=d_multi.data_ptr(), d_pairs=d_pairs.data_ptr(), d_dup=d_dup.data_ptr(), stream=stream)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    total = bam.emit_dev(*emit, 0, 0, d_off.data_ptr(), **kw)
    assert total == len(body)
    d_recs = torch.full((total,), 0x7e, dtype=torch.uint8, device=DEV)
    assert bam.emit_dev(*emit, d_recs.data_ptr(), total, d_off.data_ptr(), **kw) == total
    d_key = torch.zeros(n, dtype=torch.int64, device=DEV)
    sam.sort_keys_dev(params, n, B.d_contigs.data_ptr(), n_contigs, d_hits.data_ptr(), d_strand.data_ptr(), d_key.data_ptr(), stream=stream, ctx=B.fm.ctx)
    d_sorted = torch.full((total,), 0x7e, dtype=torch.uint8, device=DEV)
    d_sorted_off, d_perm = torch.zeros(n + 1, dtype=torch.int64, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV)
    sam.sort_dev(n, d_key.data_ptr(), d_recs.data_ptr(), d_off.data_ptr(), total, d_sorted.data_ptr(), total, d_sorted_off.data_ptr(),
                 d_perm.data_ptr(), stream=stream, ctx=B.fm.ctx)
    need = bam.framed_bytes(total, bam.BGZF_EOF)
    d_file = torch.full((need,), 0x7e, dtype=torch.uint8, device=DEV)
    assert bam.bgzf_frame_dev(d_sorted.data_ptr(), total, d_file.data_ptr(), need, bam.BGZF_EOF, stream, ctx=B.fm.ctx) == need
    torch.cuda.synchronize()
    assert d_file.cpu().numpy().tobytes() == file[base:]
    assert (d_sorted_off.cpu().numpy().astype(np.uint64) == off).all() and so.offsets(recs).tolist() == off.tolist()
