"""Device-resident timing of the BAM tail next to the SAM tail, in one process
(python tools/exp/time_bam.py [PAIRS] [GENOME_BP] [REPEATS] [OUT]), on the batch of tools/exp/time_sam_sort.py: a random genome
of GENOME_BP (default 100 M) in three contigs indexed on the device, PAIRS (default 500 000) pairs of 150 bp with a tenth planted
duplicates, their FASTQ text parsed on the device, bg_seed_extend_pairs_mapq_batch_dev once outside the timed rounds.
  * bg_bam_emit_batch_dev next to bg_sam_emit_dup_batch_dev (both with the duplicate bytes, both read a total back);
  * bg_bgzf_frame_dev over the sorted records next to a device-to-device copy of the same bytes;
  * the tails: markdup + emit + keys + sort (+ frame for BAM), each call once per round between two device events.
After 2 warm-up rounds, REPEATS (default 9) rounds; the figures are medians with the rounds' min and max.  The framed file is
checked once on the host: gzip.decompress gives the sorted records back, and the first block's CRC-32 is zlib's."""
import gzip
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
torch.cuda.init()
from rust_bio_amd import _lib, bam, fastq, sam, synth, synth_gpu  # noqa: E402
from rust_bio_amd.fmindex import FMIndex  # noqa: E402
from rust_bio_amd.pairwise import Scoring  # noqa: E402
from rust_bio_amd.pipeline import PairParams, PairQualityParams, SeedParams, attach_text, seed_extend_pairs_mapq_dev  # noqa: E402
from rust_bio_amd.suffix_array import bwt_dev, sample_dev, suffix_array_dev  # noqa: E402

N_PAIRS = int(float(sys.argv[1])) if len(sys.argv) > 1 else 500_000
N_GENOME = int(float(sys.argv[2])) if len(sys.argv) > 2 else 100_000_000
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 9
N, L = 2 * N_PAIRS, 150
FLAGS = sam.SAM_PAIRED | sam.SAM_TAG_NM | sam.SAM_TAG_MD
dev = torch.device("cuda:0")
ctx = _lib.Context(0)
stream = torch.cuda.current_stream().cuda_stream
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


# ---- the batch of time_sam_sort.py: genome, index, reads with planted duplicates, parsed FASTQ, hits
g_dev = synth_gpu.genome(N_GENOME, seed=33, device=dev)
cuts = [N_GENOME // 3, 2 * N_GENOME // 3]
g_dev[cuts] = ord("$")
edges = [-1] + cuts + [N_GENOME]
contigs = sam.Contigs([("chr%d" % (c + 1), edges[c] + 1, edges[c + 1] - edges[c] - 1) for c in range(3)])
d_sa = suffix_array_dev(g_dev, ctx=ctx)
d_b = bwt_dev(g_dev, d_sa, ctx=ctx)
ssa = sample_dev(d_sa, d_b, ord("$"), 32, ctx=ctx)
fm = FMIndex.from_device(d_b, 128, b"ACGTNacgtn", ctx=ctx)
fm._d_bwt = None
del d_sa, d_b
ssa.attach(fm)
attach_text(fm, d_text=g_dev)
reads, _, _ = synth_gpu.read_pairs_from_genome(g_dev, N_PAIRS, L, seed=5, min_frag=300, max_frag=500)
rows = reads.view(N_PAIRS, 2 * L)
rng = np.random.default_rng(17)
planted = np.nonzero(rng.random(N_PAIRS) < 0.1)[0]
planted = planted[planted > 0]
source = (rng.random(len(planted)) * planted).astype(np.int64)
rows[torch.from_numpy(planted).to(dev)] = rows[torch.from_numpy(source).to(dev)]
text = synth.fastq_text(N, L, seed=6).copy()
t_rows = text.reshape(N, len(text) // N)
o = int(np.nonzero(t_rows[0] == 10)[0][0]) + 1
t_rows[:, o:o + L] = reads.view(N, L).cpu().numpy()
d_fq = torch.from_numpy(text).to(dev)
n, status, _, d_recs, d_seq, d_so, d_qual, d_qo = fastq.parse_dev(d_fq, ctx=ctx, stream=stream)
assert (n, status) == (N, "ok")
prm, pp, qp, sc = SeedParams(20, 10, 16, 25), PairParams(0, 1000, 17), PairQualityParams(0, 60), Scoring.from_scores(-5, -1, 1, -1)
stride = 2 * L + 2 * prm.pad + 4
d_hits = torch.zeros(N * 96, dtype=torch.uint8, device=dev)
d_ops = torch.zeros(N * stride, dtype=torch.uint8, device=dev)
d_strand = torch.zeros(N, dtype=torch.uint8, device=dev)
d_pairs = torch.zeros(N_PAIRS * 16, dtype=torch.uint8, device=dev)
d_multi = torch.zeros(N * 16, dtype=torch.uint8, device=dev)
seed_extend_pairs_mapq_dev(fm, sc, N_PAIRS, d_seq.data_ptr(), d_so.data_ptr(), L, d_hits.data_ptr(), d_pairs.data_ptr(), d_multi.data_ptr(),
                           d_strand.data_ptr(), d_ops.data_ptr(), stride, prm, pp, qp, stream)
d_contigs = torch.from_numpy(contigs.table.view(np.uint8).copy()).to(dev)
d_names = torch.from_numpy(contigs.names).to(dev)

# ---- the calls
sp, mp = sam.SamParams(FLAGS, 1), sam.MarkdupParams(sam.SAM_PAIRED, 1, 33, 15)
d_dup = torch.zeros(N, dtype=torch.uint8, device=dev)
d_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
d_key = torch.zeros(N, dtype=torch.int64, device=dev)
d_perm = torch.zeros(N, dtype=torch.int64, device=dev)
d_sorted_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
emit_args = (fm, sp, N, d_contigs.data_ptr(), 3, d_names.data_ptr(), d_fq.data_ptr(), d_recs.data_ptr(), d_seq.data_ptr(), d_qual.data_ptr(),
             d_hits.data_ptr(), d_strand.data_ptr(), d_ops.data_ptr())
emit_kw = dict(d_multi=d_multi.data_ptr(), d_pairs=d_pairs.data_ptr(), d_dup=d_dup.data_ptr(), stream=stream)


def markdup():
    return sam.markdup_dev(mp, N, d_contigs.data_ptr(), 3, d_hits.data_ptr(), d_strand.data_ptr(), d_recs.data_ptr(), d_qual.data_ptr(),
                           d_dup.data_ptr(), stream=stream, ctx=ctx)


def keys():
    sam.sort_keys_dev(sp, N, d_contigs.data_ptr(), 3, d_hits.data_ptr(), d_strand.data_ptr(), d_key.data_ptr(), stream=stream, ctx=ctx)


markdup()
sam_total = sam.emit_dev(*emit_args, 0, 0, d_off.data_ptr(), **emit_kw)
bam_total = bam.emit_dev(*emit_args, 0, 0, d_off.data_ptr(), **emit_kw)
framed = bam.framed_bytes(bam_total, bam.BGZF_EOF)
d_text = torch.zeros(sam_total, dtype=torch.uint8, device=dev)
d_text_sorted = torch.zeros(sam_total, dtype=torch.uint8, device=dev)
d_bam = torch.zeros(bam_total, dtype=torch.uint8, device=dev)
d_bam_sorted = torch.zeros(bam_total, dtype=torch.uint8, device=dev)
d_file = torch.zeros(framed, dtype=torch.uint8, device=dev)
d_copy = torch.zeros(bam_total, dtype=torch.uint8, device=dev)


def sort(d_in, total, d_out):
    sam.sort_dev(N, d_key.data_ptr(), d_in.data_ptr(), d_off.data_ptr(), total, d_out.data_ptr(), total, d_sorted_off.data_ptr(),
                 d_perm.data_ptr(), stream=stream, ctx=ctx)


CALLS = [
    ("markdup", "bg_sam_markdup_dev", markdup),
    ("keys", "bg_sam_sort_keys_dev", keys),
    ("sam_emit", "bg_sam_emit_dup_batch_dev (reads its total back)", lambda: sam.emit_dev(*emit_args, d_text.data_ptr(), sam_total, d_off.data_ptr(), **emit_kw)),
    ("sam_sort", "bg_sam_sort_dev over the SAM lines", lambda: sort(d_text, sam_total, d_text_sorted)),
    ("bam_emit", "bg_bam_emit_batch_dev (reads its total and its count back)", lambda: bam.emit_dev(*emit_args, d_bam.data_ptr(), bam_total, d_off.data_ptr(), **emit_kw)),
    ("bam_sort", "bg_sam_sort_dev over the BAM records", lambda: sort(d_bam, bam_total, d_bam_sorted)),
    ("frame", "bg_bgzf_frame_dev over the sorted records, with the end-of-file block",
     lambda: bam.bgzf_frame_dev(d_bam_sorted.data_ptr(), bam_total, d_file.data_ptr(), framed, bam.BGZF_EOF, stream, ctx=ctx)),
    ("copy", "device-to-device copy of the sorted records (the yardstick of the framing)", lambda: d_copy.copy_(d_bam_sorted)),
]
ms = {c[0]: [] for c in CALLS}
for rnd in range(2 + REPEATS):
    for key, _, f in CALLS:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        if rnd >= 2:
            ms[key].append(a.elapsed_time(b))

med, lo, hi = {}, {}, {}
say("%d pairs = %d reads of %d bp on a genome of %d bp in 3 contigs; SAM text %.1f MB (%.0f bytes a line), BAM records %.1f MB (%.0f bytes a "
    "record), framed %.1f MB in %d blocks" % (N_PAIRS, N, L, N_GENOME, sam_total / 1e6, sam_total / N, bam_total / 1e6, bam_total / N, framed / 1e6,
                                              (bam_total + bam.PAYLOAD - 1) // bam.PAYLOAD))
for key, name, _ in CALLS:
    t = sorted(ms[key])
    med[key], lo[key], hi[key] = t[len(t) // 2], t[0], t[-1]
    say("%-82s median %8.3f ms (min %.3f max %.3f)" % (name, med[key], t[0], t[-1]))
say("bg_bam_emit_batch_dev / bg_sam_emit_dup_batch_dev = %.3f (medians; the SAM writer's rounds span %.3f .. %.3f ms, the BAM writer's %.3f .. %.3f)" % (
    med["bam_emit"] / med["sam_emit"], lo["sam_emit"], hi["sam_emit"], lo["bam_emit"], hi["bam_emit"]))
say("bg_bgzf_frame_dev: %.1f GB/s over the records read once and written once; device-to-device copy of the same bytes %.1f GB/s; "
    "frame / copy = %.2f" % (2 * bam_total / med["frame"] / 1e6, 2 * bam_total / med["copy"] / 1e6, med["frame"] / med["copy"]))
sam_tail = med["markdup"] + med["sam_emit"] + med["keys"] + med["sam_sort"]
bam_tail = med["markdup"] + med["bam_emit"] + med["keys"] + med["bam_sort"] + med["frame"]
say("the SAM tail (markdup + emit + keys + sort) %.3f ms; the BAM tail (markdup + emit + keys + sort + frame) %.3f ms; BAM / SAM = %.2f" % (
    sam_tail, bam_tail, bam_tail / sam_tail))
# the bytes are right: the file decompresses to the sorted records, whose keys ascend
torch.cuda.synchronize()
file = d_file.cpu().numpy().tobytes()
body = d_bam_sorted.cpu().numpy().tobytes()
assert gzip.decompress(file) == body and file[18 + 5 + bam.PAYLOAD:][:4] == zlib.crc32(body[:bam.PAYLOAD]).to_bytes(4, "little")
kk = d_key[d_perm].cpu().numpy().view(np.uint64)
assert (kk[1:] >= kk[:-1]).all() and int(d_sorted_off[-1]) == bam_total
say("checked: gzip.decompress(file) == the sorted records; keys ascend")
say("not measured: the host-buffer flavours, single-end batches, K > 1, records beyond the staging limit, counters of any kernel")
if len(sys.argv) > 4:
    open(sys.argv[4], "w").write("tools/exp/time_bam.py %d %d %d on one MI355X, device-resident: every call once per round between two device "
                                 "events, %d rounds after 2 warm-up rounds, medians\n" % (N_PAIRS, N_GENOME, REPEATS, REPEATS) + "\n".join(lines) + "\n")
