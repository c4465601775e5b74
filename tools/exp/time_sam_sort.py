"""Device-resident timing of duplicate marking, the writer with the flag, the key pass and the sort next to the writer they follow,
in one process (python tools/exp/time_sam_sort.py [PAIRS] [GENOME_BP] [REPEATS] [OUT]):
  * a random genome of GENOME_BP (default 100 M) cut into three contigs, indexed on the device as tools/exp/time_seed_extend_pairq.py
    indexes its genome; PAIRS (default 500 000) pairs of 150 bp mates of fragments of 300-500 bp (synth_gpu.read_pairs_from_genome),
    a tenth of them replaced by copies of another pair's reads (planted duplicates); their FASTQ text (ids and qualities of
    synth.fastq_text) parsed on the device; bg_seed_extend_pairs_mapq_batch_dev once, outside the timed rounds;
  * bg_sam_emit_batch_dev (the writer as it was), bg_sam_markdup_dev, bg_sam_emit_dup_batch_dev with the duplicate bytes and
    with a null dup, bg_sam_sort_keys_dev, bg_sam_sort_dev, and a device-to-device copy of the text's bytes, the yardstick of the
    sort's permuted copy;
  * after 2 warm-up rounds, REPEATS (default 9) rounds that run every call once, in turn, between two device events; the figures
    are medians over the rounds.  The writer and the duplicate marker read a total back, so they synchronise once; the key pass and
    the sort do not.  The sort's two halves — rocPRIM's radix sort, and the lengths, their scan and the permuted copy — come from
    bg_get_timing in REPEATS further calls with bg_enable_timing on (the call then waits for its own events).
Algorithmic bytes of the permuted copy: the text read once and written once."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
torch.cuda.init()
from rust_bio_amd import _lib, fastq, sam, synth, synth_gpu  # noqa: E402
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


# ---- the genome in three contigs, its index
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

# ---- the reads, a tenth of the pairs planted duplicates; their FASTQ text parsed on the device
reads, _, _ = synth_gpu.read_pairs_from_genome(g_dev, N_PAIRS, L, seed=5, min_frag=300, max_frag=500)
rows = reads.view(N_PAIRS, 2 * L)
rng = np.random.default_rng(17)
planted = np.nonzero(rng.random(N_PAIRS) < 0.1)[0]
planted = planted[planted > 0]
source = (rng.random(len(planted)) * planted).astype(np.int64)  # an earlier pair
rows[torch.from_numpy(planted).to(dev)] = rows[torch.from_numpy(source).to(dev)]
text = synth.fastq_text(N, L, seed=6).copy()
t_rows = text.reshape(N, len(text) // N)
o = int(np.nonzero(t_rows[0] == 10)[0][0]) + 1
t_rows[:, o:o + L] = reads.view(N, L).cpu().numpy()
d_fq = torch.from_numpy(text).to(dev)
n, status, _, d_recs, d_seq, d_so, d_qual, d_qo = fastq.parse_dev(d_fq, ctx=ctx, stream=stream)
assert (n, status) == (N, "ok")

# ---- hits, once
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
emit_kw = dict(d_multi=d_multi.data_ptr(), d_pairs=d_pairs.data_ptr(), stream=stream)


def markdup():
    return sam.markdup_dev(mp, N, d_contigs.data_ptr(), 3, d_hits.data_ptr(), d_strand.data_ptr(), d_recs.data_ptr(), d_qual.data_ptr(),
                           d_dup.data_ptr(), stream=stream, ctx=ctx)


counts = markdup()
total = sam.emit_dev(*emit_args, 0, 0, d_off.data_ptr(), d_dup=d_dup.data_ptr(), **emit_kw)
d_text = torch.zeros(total, dtype=torch.uint8, device=dev)
d_sorted = torch.zeros(total, dtype=torch.uint8, device=dev)
d_plain = torch.zeros(total, dtype=torch.uint8, device=dev)


def emit_null_dup():
    t = C.c_uint64(0)
    pc = sp.to_c()
    _lib.check(_lib.lib().bg_sam_emit_dup_batch_dev(fm.h, C.byref(pc), *emit_args[2:], d_multi.data_ptr(), d_pairs.data_ptr(), None,
                                                    d_plain.data_ptr(), total, d_off.data_ptr(), C.byref(t), stream), "bg_sam_emit_dup_batch_dev")
    return t.value


def sort():
    sam.sort_dev(N, d_key.data_ptr(), d_text.data_ptr(), d_off.data_ptr(), total, d_sorted.data_ptr(), total, d_sorted_off.data_ptr(),
                 d_perm.data_ptr(), stream=stream, ctx=ctx)


def emit_dup():
    return sam.emit_dev(*emit_args, d_text.data_ptr(), total, d_off.data_ptr(), d_dup=d_dup.data_ptr(), **emit_kw)


CALLS = [
    ("emit", "bg_sam_emit_batch_dev (the writer as it was; reads its total back)", lambda: sam.emit_dev(*emit_args, d_plain.data_ptr(), total, d_off.data_ptr(), **emit_kw)),
    ("emit_null", "bg_sam_emit_dup_batch_dev, dup == NULL", emit_null_dup),
    ("markdup", "bg_sam_markdup_dev (reads its counts back)", markdup),
    ("emit_dup", "bg_sam_emit_dup_batch_dev with the duplicate bytes", emit_dup),
    ("keys", "bg_sam_sort_keys_dev", lambda: sam.sort_keys_dev(sp, N, d_contigs.data_ptr(), 3, d_hits.data_ptr(), d_strand.data_ptr(),
                                                                 d_key.data_ptr(), stream=stream, ctx=ctx)),
    ("sort", "bg_sam_sort_dev (radix sort, lengths, scan, permuted copy)", sort),
    ("copy", "device-to-device copy of the text (the yardstick of the permuted copy)", lambda: d_sorted.copy_(d_text)),
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
# the sort's halves
sort()
torch.cuda.synchronize()
check = d_sorted.clone()
ctx.enable_timing(True)
halves = []
for rnd in range(REPEATS):
    sort()
    t = ctx.timing()
    halves.append((t["fm_ms"], t["fill_ms"]))
ctx.enable_timing(False)
torch.cuda.synchronize()
assert torch.equal(check, d_sorted)
radix = sorted(h[0] for h in halves)[REPEATS // 2]
copy = sorted(h[1] for h in halves)[REPEATS // 2]

med = {}
say("%d pairs = %d reads of %d bp on a genome of %d bp in 3 contigs; %d planted duplicate pairs; SAM text %.1f MB (%.0f bytes a line); "
    "markdup counts: %d reads with an end, %d reads flagged, %d pairs flagged, %d fragments flagged by a pair's end" % (
        N_PAIRS, N, L, N_GENOME, len(planted), total / 1e6, total / N, *counts))
for key, name, _ in CALLS:
    t = sorted(ms[key])
    med[key] = m = t[len(t) // 2]
    say("%-78s median %8.3f ms (min %.3f max %.3f)  %7.1f M reads/s" % (name, m, t[0], t[-1], N / m / 1e3))
say("bg_sam_sort_dev with bg_enable_timing: radix sort of (key, index) median %.3f ms; lengths + scan + permuted copy median %.3f ms "
    "(%.1f GB/s over the text read once and written once)" % (radix, copy, 2 * total / copy / 1e6))
say("device-to-device copy of the same bytes: %.3f ms (%.1f GB/s); permuted copy (with its lengths and scan) / device-to-device copy = %.2f" % (
    med["copy"], 2 * total / med["copy"] / 1e6, copy / med["copy"]))
say("emit_dup with dup == NULL / bg_sam_emit_batch_dev = %.3f; with the duplicate bytes / bg_sam_emit_batch_dev = %.3f" % (
    med["emit_null"] / med["emit"], med["emit_dup"] / med["emit"]))
say("the whole tail (markdup + emit_dup + keys + sort) / bg_sam_emit_batch_dev = %.2f" % (
    (med["markdup"] + med["emit_dup"] + med["keys"] + med["sort"]) / med["emit"]))
# the bytes are right: sorted text is the permutation of the unsorted one, keys ascend
assert sam.emit_dev(*emit_args, d_text.data_ptr(), total, d_off.data_ptr(), d_dup=d_dup.data_ptr(), **emit_kw) == total
sort()
torch.cuda.synchronize()
kk = d_key[d_perm].cpu().numpy().view(np.uint64)
assert (kk[1:] >= kk[:-1]).all() and int(d_sorted_off[-1]) == total
assert torch.equal(torch.bincount(d_sorted, minlength=256), torch.bincount(d_text, minlength=256))
say("not measured: the host-buffer flavours, single-end batches, K > 1, lines beyond %d bytes (the block kernel), counters of any kernel" % 16384)
if len(sys.argv) > 4:
    open(sys.argv[4], "w").write("tools/exp/time_sam_sort.py %d %d %d on one MI355X, device-resident: every call once per round between two "
                                 "device events, %d rounds after 2 warm-up rounds, medians\n" % (N_PAIRS, N_GENOME, REPEATS, REPEATS) + "\n".join(lines) + "\n")
