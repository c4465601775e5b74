"""Device-resident timing of bg_bam_index_dev next to its two yardsticks, in one process
(python tools/exp/time_bam_index.py [PAIRS] [GENOME_BP] [REPEATS] [OUT]), on the batch of tools/exp/time_bam.py (the set-up below is
that tool's): the coordinate-sorted BAM records of PAIRS (default 500 000) pairs of 150 bp, 385 MB in about 5 900 blocks.
  * bg_bam_index_dev over the sorted records with the stored framing (closed form) and with the block table bg_bgzf_deflate_dev
    filled for the same records, each once per round between two device events (the call reads its total back, so the second
    event is recorded behind a synchronisation the call itself makes); after 2 warm-up rounds REPEATS (default 9) rounds,
    medians with the rounds' min and max;
  * the yardsticks, timed in the same rounds: bg_sam_sort_dev over the same records (one pass over per-record data, one radix
    sort, a few scans as well) and bg_bam_emit_batch_dev, the record writer;
  * the sizing call (everything but the three kernels that store the bytes), for the share of the stores.
The index is checked once on the host against tests/bai_oracle.py (both framings) and read by its parser."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
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
bam_total = bam.emit_dev(*emit_args, 0, 0, d_off.data_ptr(), **emit_kw)
framed = bam.framed_bytes(bam_total, bam.BGZF_EOF)
d_bam = torch.zeros(bam_total, dtype=torch.uint8, device=dev)
d_bam_sorted = torch.zeros(bam_total, dtype=torch.uint8, device=dev)


def sort(d_in, total, d_out):
    sam.sort_dev(N, d_key.data_ptr(), d_in.data_ptr(), d_off.data_ptr(), total, d_out.data_ptr(), total, d_sorted_off.data_ptr(),
                 d_perm.data_ptr(), stream=stream, ctx=ctx)


markdup()
keys()
bam.emit_dev(*emit_args, d_bam.data_ptr(), bam_total, d_off.data_ptr(), **emit_kw)
sort(d_bam, bam_total, d_bam_sorted)
n_blocks = (bam_total + bam.PAYLOAD - 1) // bam.PAYLOAD
d_block_off = torch.zeros(n_blocks + 1, dtype=torch.int64, device=dev)
d_zfile = torch.zeros(framed, dtype=torch.uint8, device=dev)
out_bytes = {}


def deflate():
    out_bytes["bam"] = bam.bgzf_deflate_dev(d_bam_sorted.data_ptr(), bam_total, d_zfile.data_ptr(), framed, bam.BGZF_EOF, stream, ctx=ctx,
                                            d_block_off=d_block_off.data_ptr())


deflate()
torch.cuda.synchronize()
BASE = 1234  # stands for the framed header's length
bai_bytes = bam.index_dev(N, d_bam_sorted.data_ptr(), d_sorted_off.data_ptr(), d_contigs.data_ptr(), 3, 0, 0, base=BASE, stream=stream, ctx=ctx)
d_bai = torch.zeros(bai_bytes, dtype=torch.uint8, device=dev)


def index(table):
    return bam.index_dev(N, d_bam_sorted.data_ptr(), d_sorted_off.data_ptr(), d_contigs.data_ptr(), 3, d_bai.data_ptr(), bai_bytes,
                         d_block_off=d_block_off.data_ptr() if table else 0, base=BASE, stream=stream, ctx=ctx)


CALLS = [
    ("bam_emit", "bg_bam_emit_batch_dev (yardstick: the record writer)",
     lambda: bam.emit_dev(*emit_args, d_bam.data_ptr(), bam_total, d_off.data_ptr(), **emit_kw)),
    ("sort", "bg_sam_sort_dev over the same records (yardstick: a radix sort, scans, the permuted copy)", lambda: sort(d_bam, bam_total, d_bam_sorted)),
    ("index_stored", "bg_bam_index_dev, stored framing (closed-form virtual offsets)", lambda: index(False)),
    ("index_table", "bg_bam_index_dev, the block table of bg_bgzf_deflate_dev", lambda: index(True)),
    ("index_size", "bg_bam_index_dev, the sizing call (everything but the stores)",
     lambda: bam.index_dev(N, d_bam_sorted.data_ptr(), d_sorted_off.data_ptr(), d_contigs.data_ptr(), 3, 0, 0, base=BASE, stream=stream, ctx=ctx)),
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
med = {}
say("%d pairs = %d reads of %d bp on a genome of %d bp in 3 contigs; BAM records %.1f MB in %d blocks; the index %d bytes" % (
    N_PAIRS, N, L, N_GENOME, bam_total / 1e6, n_blocks, bai_bytes))
for key, name, _ in CALLS:
    t = sorted(ms[key])
    med[key] = t[len(t) // 2]
    say("%-100s median %8.3f ms (min %.3f max %.3f)" % (name, med[key], t[0], t[-1]))
say("bg_bam_index_dev / bg_sam_sort_dev = %.2f (stored), %.2f (block table); / bg_bam_emit_batch_dev = %.3f, %.3f" % (
    med["index_stored"] / med["sort"], med["index_table"] / med["sort"], med["index_stored"] / med["bam_emit"], med["index_table"] / med["bam_emit"]))

# the bytes are right: the oracle's, under both framings
import bai_oracle as ba  # noqa: E402
import bam_oracle as bo  # noqa: E402
t0 = time.perf_counter()
body = d_bam_sorted.cpu().numpy().tobytes()
off = d_sorted_off.cpu().numpy().astype(np.uint64)
slots = [body[int(off[i]):int(off[i + 1])] for i in range(N)]
entries = [(contigs.name(c), int(contigs.table["start"][c]), int(contigs.table["len"][c])) for c in range(3)]
table = d_block_off.cpu().numpy().astype(np.uint64)
for use_table in (False, True):
    assert index(use_table) == bai_bytes
    torch.cuda.synchronize()
    got = d_bai.cpu().numpy().tobytes()
    assert got == ba.build(slots, entries, ba.table_voff(table, BASE) if use_table else ba.stored_voff(BASE)), use_table
refs, n_no_coor = ba.parse(got)
say("checked: both indexes are the oracle's bytes (%.0f s on the host); per contig (bins, chunks, windows): %s; n_no_coor %d; empty slots %d" % (
    time.perf_counter() - t0, [(len(r["bins"]), sum(len(c) for c in r["bins"].values()), len(r["intv"])) for r in refs], n_no_coor,
    sum(1 for s in slots if not s)))
say("not measured: the host-buffer flavour, the kernels of the call one by one, counters of any kernel")
if len(sys.argv) > 4:
    open(sys.argv[4], "w").write("tools/exp/time_bam_index.py %d %d %d on one MI355X, device-resident: every call once per round between two device "
                                 "events, %d rounds after 2 warm-up rounds, medians\n" % (N_PAIRS, N_GENOME, REPEATS, REPEATS) + "\n".join(lines) + "\n")
