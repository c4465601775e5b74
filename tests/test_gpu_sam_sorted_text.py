"""Coordinate-sorted SAM with duplicate flags, end to end on the device: FASTQ text -> bg_fastq_parse_dev -> paired seed-and-extend
with MAPQ -> bg_sam_markdup_dev -> bg_sam_emit_dup_batch_dev -> bg_sam_sort_keys_dev -> bg_sam_sort_dev, on a genome of 6 kbp cut
into three contigs the way tests/test_gpu_sam_emit.py cuts its genomes.  The reads hold planted duplicate pairs (one fragment
sequenced several times), a planted fragment (mate 1 of a duplicated fragment with an unmappable mate 2) and unmappable pairs.
The sorted body must pass the check that reads only SAM text, equal the record oracle's lines (tests/sam_oracle.py) with 0x400
added by the duplicate oracle and permuted by the sort oracle, and sit under a header that says SO:coordinate; without `dup`
the writer's bytes are bg_sam_emit_batch_dev's."""
import functools

import numpy as np
import pytest
import torch

import sam_oracle as so
import sam_sort_oracle as sso
from rust_bio_amd import fastq, sam, synth
from rust_bio_amd.pairwise import Scoring
from rust_bio_amd.pipeline import PairParams, attach_text, seed_extend_pairs_mapq_arrays, seed_extend_pairs_mapq_dev
from test_gpu_pipeline import build
from test_gpu_sam_emit import ALL_TAGS, DEV, Batch, cut, fastq_text
from test_gpu_seed_extend_pairs import mates_at

pytestmark = pytest.mark.gpu
SC = Scoring.from_scores(-5, -1, 1, -1)
L, FRAG = 80, 240
FLAGS = sam.SAM_PAIRED | ALL_TAGS
PHRED, MIN_QUAL = 33, 15


@functools.lru_cache(maxsize=None)
def case():
    g = synth.random_dna(6_000, seed=77).copy()
    text, entries = cut(g, (1_999, 3_999))
    rng = np.random.default_rng(5)
    starts = np.concatenate([rng.integers(20, 1_700, size=14), rng.integers(2_020, 3_700, size=14), rng.integers(4_020, 5_700, size=14)])
    planted = np.array([300] * 5 + [2_500] * 4 + [4_400] * 6)  # duplicate pairs: the same fragment again (a third with swapped mates)
    s = np.concatenate([starts, planted, [300, 2_500]])                             # ... and two fragments of planted pairs
    swap = np.zeros(len(s), bool)
    swap[1::3] = True
    reads, _, _ = mates_at(g, s, np.full(len(s), FRAG), L, 41, swap, sub=0.01)
    n_frag = len(s) - 2
    reads[2 * n_frag + 1] = synth.random_dna(L, seed=9)   # the fragments' other mates are unmappable
    reads[2 * n_frag + 3] = synth.random_dna(L, seed=10)
    junk = synth.random_dna(6 * L, seed=11).reshape(6, L)  # three unmappable pairs
    seqs = [x.tobytes() for x in reads] + [x.tobytes() for x in junk]
    ids = [b"f%d/%d" % (r // 2, r % 2 + 1) for r in range(len(seqs))]
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    return Batch(fm, entries, text, fastq_text(seqs, ids, seed=4), len(seqs))


def test_the_chain_on_the_device():
    B = case()
    p, pp = B.parsed, PairParams(0, 1000, 17)
    stream = torch.cuda.current_stream().cuda_stream
    n, n_contigs = B.n, len(B.contigs)
    # what the lines must be: the host calls' hits through the three oracles
    hits, strand, pairs, multi, ops = seed_extend_pairs_mapq_arrays(B.fm, SC, p.seq, p.seq_off, pair_params=pp)
    dup, counts = sso.markdup(B.entries, p, hits, strand, so.PAIRED, 1, PHRED, MIN_QUAL)
    print("sorted text case: reads with an end, reads flagged, pairs flagged, fragments flagged by a pair:", counts)
    assert counts[2] >= 4 and counts[3] >= 1 and n - counts[0] >= 8, counts
    plain = B.oracle(FLAGS, 1, hits, strand, ops, multi, pairs)
    flagged = sso.add_dup_flag(plain, dup)
    assert sum(a != b for a, b in zip(plain, flagged)) == counts[1]
    key = sso.sort_keys(B.entries, hits, strand, FLAGS, 1)
    perm, out_off, want = sso.sort(key, flagged)
    # the chain
    d_hits, d_strand, d_ops, stride = B.device_slots(1)
    d_pairs = torch.zeros(n // 2 * 16, dtype=torch.uint8, device=DEV)
    d_multi = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    seed_extend_pairs_mapq_dev(B.fm, SC, n // 2, B.d_seq.data_ptr(), B.d_seq_off.data_ptr(), B.max_len, d_hits.data_ptr(), d_pairs.data_ptr(),
                               d_multi.data_ptr(), d_strand.data_ptr(), d_ops.data_ptr(), stride, pair_params=pp, stream=stream)
    d_dup = torch.full((n,), 0x7e, dtype=torch.uint8, device=DEV)
    got_counts = sam.markdup_dev(sam.MarkdupParams(sam.SAM_PAIRED, 1, PHRED, MIN_QUAL), n, B.d_contigs.data_ptr(), n_contigs, d_hits.data_ptr(),
                                 d_strand.data_ptr(), B.d_recs.data_ptr(), B.d_qual.data_ptr(), d_dup.data_ptr(), stream=stream, ctx=B.fm.ctx)
    assert got_counts == counts and d_dup.cpu().numpy().tobytes() == dup.tobytes()
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    emit = (B.fm, sam.SamParams(FLAGS, 1), n, B.d_contigs.data_ptr(), n_contigs, B.d_names.data_ptr(), B.d_fq.data_ptr(), B.d_recs.data_ptr(),
            B.d_seq.data_ptr(), B.d_qual.data_ptr(), d_hits.data_ptr(), d_strand.data_ptr(), d_ops.data_ptr())
    kw = dict(d_multi=d_multi.data_ptr(), d_pairs=d_pairs.data_ptr(), stream=stream)
    total = sam.emit_dev(*emit, 0, 0, d_off.data_ptr(), d_dup=d_dup.data_ptr(), **kw)
    assert total == len(want)
    d_text = torch.full((total,), 0x7e, dtype=torch.uint8, device=DEV)
    assert sam.emit_dev(*emit, d_text.data_ptr(), total, d_off.data_ptr(), d_dup=d_dup.data_ptr(), **kw) == total
    unsorted = d_text.cpu().numpy().tobytes()
    assert unsorted == b"".join(flagged) and (d_off.cpu().numpy().astype(np.uint64) == so.offsets(flagged)).all()
    d_key = torch.zeros(n, dtype=torch.int64, device=DEV)
    sam.sort_keys_dev(sam.SamParams(FLAGS, 1), n, B.d_contigs.data_ptr(), n_contigs, d_hits.data_ptr(), d_strand.data_ptr(), d_key.data_ptr(),
                      stream=stream, ctx=B.fm.ctx)
    assert (d_key.cpu().numpy().astype(np.uint64) == key).all()
    d_sorted = torch.full((total + 32,), 0x7e, dtype=torch.uint8, device=DEV)
    d_sorted_off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    d_perm = torch.zeros(n, dtype=torch.int64, device=DEV)
    sam.sort_dev(n, d_key.data_ptr(), d_text.data_ptr(), d_off.data_ptr(), total, d_sorted.data_ptr(), total, d_sorted_off.data_ptr(),
                 d_perm.data_ptr(), stream=stream, ctx=B.fm.ctx)
    torch.cuda.synchronize()
    body = d_sorted.cpu().numpy()
    assert (body[total:] == 0x7e).all()
    body = body[:total].tobytes()
    assert (d_perm.cpu().numpy().astype(np.uint64) == perm).all() and (d_sorted_off.cpu().numpy().astype(np.uint64) == out_off).all()
    assert body == want
    # the check that reads only text; unmapped lines last; flagged lines present
    places = sso.check_sorted_text([e[0] for e in B.entries], unsorted, body)
    assert places[0][0] == 0 and places[-1][0] == len(B.entries) and {pl[0] for pl in places} == {0, 1, 2, 3}
    assert sum(int(line.split(b"\t")[1]) & 0x400 > 0 for line in body.splitlines()) == counts[1]
    header = sam.header(B.contigs, sam.SAM_SO_COORDINATE)
    assert header.startswith(b"@HD\tVN:1.6\tSO:coordinate\n") and header == so.header(B.entries).replace(b"SO:unsorted", b"SO:coordinate")
    # the host chain gives the same file
    assert sam.sorted_sam(B.fm, sam.SamParams(FLAGS, 1), B.contigs, p, hits, strand, ops, multi=multi, pairs=pairs,
                          markdup=sam.MarkdupParams(sam.SAM_PAIRED, 1, PHRED, MIN_QUAL), ctx=B.fm.ctx) == header + want
    # without dup the writer writes what bg_sam_emit_batch_dev writes: the flavour with a null dup, and the old entry point
    d_a = torch.full((total,), 0x7e, dtype=torch.uint8, device=DEV)
    d_b = torch.full((total,), 0x7e, dtype=torch.uint8, device=DEV)
    t_a = sam.emit_dev(*emit, d_a.data_ptr(), total, d_off.data_ptr(), **kw)
    import ctypes as C
    from rust_bio_amd import _lib
    t_b = C.c_uint64(0)
    pc = sam.SamParams(FLAGS, 1).to_c()
    rc = _lib.lib().bg_sam_emit_dup_batch_dev(B.fm.h, C.byref(pc), *emit[2:], d_multi.data_ptr(), d_pairs.data_ptr(), None, d_b.data_ptr(), total,
                                              d_off.data_ptr(), C.byref(t_b), stream)
    torch.cuda.synchronize()
    assert rc == 0 and t_a == t_b.value == len(b"".join(plain))
    assert d_a.cpu().numpy()[:t_a].tobytes() == d_b.cpu().numpy()[:t_a].tobytes() == b"".join(plain)
