"""Device-resident timing of the pileup, in one process (python tools/exp/time_bam_pileup.py [PAIRS] [GENOME_BP] [REPEATS] [OUT]), on
the batch of tools/exp/time_bam_read.py (the set-up below is that tool's): the coordinate-sorted, duplicate-flagged BAM records of
PAIRS (default 500 000) pairs of 150 bp on a genome of three contigs, as bg_bam_emit_batch_dev and bg_sam_sort_dev leave them.
Two sets of regions, both forms (8 and 16 columns) of each:
  * wide: ONE region, the first SPAN (default 30 000 000, at most chr1) positions of chr1 — 0.96 GB of rows in the 8-column
    form and 1.92 GB in the 16-column form, under the 2 GB a result may have here;
  * targets: 20 000 regions of 300 positions, evenly spread over the three contigs.
Each call once per round between two device events; after 2 warm-up rounds REPEATS (default 9) rounds, medians with the rounds'
min and max.  The yardsticks, in the same process on the same records: bg_bam_index_dev, bg_bam_reads_dev (all columns), and a
device-to-device copy of as many bytes as the wide rows of either form.  Checked on the device: the 16-column rows folded are
the 8-column rows, a target's rows are the wide rows of the same positions, and the span cut into 1 000 regions gives the rows
of the one region (the tests hold the counters themselves to tests/bam_pileup_oracle.py)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from csrc_hash import csrc_sha  # noqa: E402
torch.cuda.init()
from rust_bio_amd import _lib, bam, fastq, sam, synth, synth_gpu  # noqa: E402
from rust_bio_amd.fmindex import FMIndex  # noqa: E402
from rust_bio_amd.pairwise import Scoring  # noqa: E402
from rust_bio_amd.pipeline import PairParams, PairQualityParams, SeedParams, attach_text, seed_extend_pairs_mapq_dev  # noqa: E402
from rust_bio_amd.suffix_array import bwt_dev, sample_dev, suffix_array_dev  # noqa: E402

if os.environ.get("BG_SO"):
    _lib.SO_PATH = os.path.abspath(os.environ["BG_SO"])
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


# ---- the batch of time_bam_read.py: genome, index, reads with planted duplicates, parsed FASTQ, hits, sorted BAM records
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
sp, mp = sam.SamParams(FLAGS, 1), sam.MarkdupParams(sam.SAM_PAIRED, 1, 33, 15)
d_dup = torch.zeros(N, dtype=torch.uint8, device=dev)
d_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
d_key = torch.zeros(N, dtype=torch.int64, device=dev)
d_perm = torch.zeros(N, dtype=torch.int64, device=dev)
d_sorted_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
emit_args = (fm, sp, N, d_contigs.data_ptr(), 3, d_names.data_ptr(), d_fq.data_ptr(), d_recs.data_ptr(), d_seq.data_ptr(), d_qual.data_ptr(),
             d_hits.data_ptr(), d_strand.data_ptr(), d_ops.data_ptr())
emit_kw = dict(d_multi=d_multi.data_ptr(), d_pairs=d_pairs.data_ptr(), d_dup=d_dup.data_ptr(), stream=stream)
sam.markdup_dev(mp, N, d_contigs.data_ptr(), 3, d_hits.data_ptr(), d_strand.data_ptr(), d_recs.data_ptr(), d_qual.data_ptr(), d_dup.data_ptr(),
                stream=stream, ctx=ctx)
sam.sort_keys_dev(sp, N, d_contigs.data_ptr(), 3, d_hits.data_ptr(), d_strand.data_ptr(), d_key.data_ptr(), stream=stream, ctx=ctx)
bam_total = bam.emit_dev(*emit_args, 0, 0, d_off.data_ptr(), **emit_kw)
d_bam = torch.zeros(bam_total, dtype=torch.uint8, device=dev)
d_bam_sorted = torch.zeros(bam_total, dtype=torch.uint8, device=dev)
bam.emit_dev(*emit_args, d_bam.data_ptr(), bam_total, d_off.data_ptr(), **emit_kw)
sam.sort_dev(N, d_key.data_ptr(), d_bam.data_ptr(), d_off.data_ptr(), bam_total, d_bam_sorted.data_ptr(), bam_total, d_sorted_off.data_ptr(),
             d_perm.data_ptr(), stream=stream, ctx=ctx)
del d_bam

# ---- the regions
len1 = int(contigs.table["len"][0])
SPAN = min(int(float(os.environ.get("BG_PILEUP_SPAN", 30_000_000))), len1)
wide = bam.pileup_regions([(0, 0, SPAN)])
pieces = bam.pileup_regions([(0, SPAN * k // 1000, SPAN * (k + 1) // 1000) for k in range(1000)])
N_TARGETS, TARGET = 20_000, 300
targets = []
for c in range(3):
    ln = int(contigs.table["len"][c])
    k = N_TARGETS // 3 + (c < N_TARGETS % 3)
    targets += [(c, int(b), int(b) + TARGET) for b in np.linspace(0, ln - TARGET, k).astype(np.int64)]
targets = bam.pileup_regions(targets)
d_regions = {name: torch.from_numpy(r.view(np.uint8).copy()).to(dev) for name, r in (("wide", wide), ("pieces", pieces), ("targets", targets))}
n_regions = {"wide": 1, "pieces": 1000, "targets": len(targets)}
n_rows = {"wide": SPAN, "pieces": SPAN, "targets": len(targets) * TARGET}
assert SPAN * 64 <= 2_000_000_000
d_rows = {(name, w): torch.zeros(n_rows[name] * w, dtype=torch.int32, device=dev) for name in ("wide", "targets") for w in (8, 16)}
d_row_off = torch.zeros(len(targets) + 1, dtype=torch.int64, device=dev)
d_copy = torch.zeros(SPAN * 16, dtype=torch.int32, device=dev)


def pileup(name, w, d_out=None, row_off=0):
    d_out = d_rows[(name, w)] if d_out is None else d_out
    got = bam.pileup_dev(N, d_bam_sorted.data_ptr(), d_sorted_off.data_ptr(), d_contigs.data_ptr(), 3, d_regions[name].data_ptr(), n_regions[name],
                         d_out.data_ptr(), n_rows[name], row_off, flags=bam.PILEUP_STRANDS if w == 16 else 0, stream=stream, ctx=ctx)
    assert got == n_rows[name]


# ---- the yardsticks
reads_kw = dict(flags=bam.BAM_READS_ORIGINAL, exclude=0x900, stream=stream, ctx=ctx)
k, sb, qb = bam.reads_dev(N, d_bam_sorted.data_ptr(), d_sorted_off.data_ptr(), 3, **reads_kw)
r_recs = torch.zeros(k * 56, dtype=torch.uint8, device=dev)
r_seq, r_qual = torch.zeros(sb, dtype=torch.uint8, device=dev), torch.zeros(qb, dtype=torch.uint8, device=dev)
r_so, r_qo, r_src = (torch.zeros(k + 1, dtype=torch.int64, device=dev) for _ in range(3))


def reads():
    assert bam.reads_dev(N, d_bam_sorted.data_ptr(), d_sorted_off.data_ptr(), 3, r_recs.data_ptr(), k, r_seq.data_ptr(), sb, r_so.data_ptr(), r_qual.data_ptr(),
                         qb, r_qo.data_ptr(), r_src.data_ptr(), **reads_kw) == (k, sb, qb)


d_bai = [torch.zeros(1, dtype=torch.uint8, device=dev)]


def index():
    big = d_bai[0].numel() > 1
    return bam.index_dev(N, d_bam_sorted.data_ptr(), d_sorted_off.data_ptr(), d_contigs.data_ptr(), 3, d_bai[0].data_ptr() if big else 0,
                         d_bai[0].numel() if big else 0, stream=stream, ctx=ctx)


d_bai = [torch.zeros(index(), dtype=torch.uint8, device=dev)]
CALLS = [
    ("index", "bg_bam_index_dev over the same records (yardstick)", index),
    ("reads", "bg_bam_reads_dev over the same records, all columns and src (yardstick)", reads),
    ("copy8", "a device-to-device copy of as many bytes as the wide rows, 8 columns (yardstick)", lambda: d_copy[:SPAN * 8].copy_(d_rows[("wide", 8)])),
    ("copy16", "a device-to-device copy of as many bytes as the wide rows, 16 columns (yardstick)", lambda: d_copy.copy_(d_rows[("wide", 16)])),
    ("wide8", "bg_bam_pileup_dev, one region of %d positions of chr1, 8 columns" % SPAN, lambda: pileup("wide", 8)),
    ("wide16", "bg_bam_pileup_dev, one region of %d positions of chr1, 16 columns (BG_PILEUP_STRANDS)" % SPAN, lambda: pileup("wide", 16)),
    ("targets8", "bg_bam_pileup_dev, %d regions of %d positions over the three contigs, 8 columns" % (len(targets), TARGET), lambda: pileup("targets", 8)),
    ("targets16", "bg_bam_pileup_dev, %d regions of %d positions over the three contigs, 16 columns" % (len(targets), TARGET), lambda: pileup("targets", 16)),
    ("sizing", "bg_bam_pileup_dev, the sizing call of the wide region (the slot pass, the scans, the read-back)",
     lambda: bam.pileup_dev(N, d_bam_sorted.data_ptr(), d_sorted_off.data_ptr(), d_contigs.data_ptr(), 3, d_regions["wide"].data_ptr(), 1, stream=stream, ctx=ctx)),
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
say("%s: %d pairs = %d reads of %d bp on a genome of %d bp in 3 contigs; %.1f MB of sorted records in %d slots; tile %d" % (
    os.path.basename(_lib.SO_PATH), N_PAIRS, N, L, N_GENOME, bam_total / 1e6, N, bam.PILEUP_TILE))
say("regions: wide = chr1:0-%d (%.2f GB of rows with 8 columns, %.2f GB with 16); targets = %d x %d positions, evenly spread over chr1 .. chr3" % (
    SPAN, SPAN * 32 / 1e9, SPAN * 64 / 1e9, len(targets), TARGET))
for key, name, _ in CALLS:
    t = sorted(ms[key])
    med[key] = t[len(t) // 2]
    say("%-110s median %8.3f ms (min %.3f max %.3f)" % (name, med[key], t[0], t[-1]))
say("wide, 8 columns: %.2f x the index, %.2f x the reads, %.2f x the copy of its rows, %.1f GB/s of rows; behind the sizing call's share: %.3f ms" % (
    med["wide8"] / med["index"], med["wide8"] / med["reads"], med["wide8"] / med["copy8"], SPAN * 32 / med["wide8"] / 1e6, med["wide8"] - med["sizing"]))
say("wide, 16 columns: %.2f x the index, %.2f x the reads, %.2f x the copy of its rows, %.1f GB/s of rows; behind the sizing call's share: %.3f ms" % (
    med["wide16"] / med["index"], med["wide16"] / med["reads"], med["wide16"] / med["copy16"], SPAN * 64 / med["wide16"] / 1e6, med["wide16"] - med["sizing"]))
say("targets: 8 columns %.2f x the index, 16 columns %.2f x; against the record writer's 9.77 ms (profiles/bam_read_timing.txt): wide16 %.2f x" % (
    med["targets8"] / med["index"], med["targets16"] / med["index"], med["wide16"] / 9.768))
# ---- checks, on the device
for name in ("wide", "targets"):
    r8, r16 = d_rows[(name, 8)].view(-1, 8), d_rows[(name, 16)].view(-1, 16)
    assert torch.equal(r16[:, :8] + r16[:, 8:], r8), name
d_again = torch.full((SPAN * 8,), -1, dtype=torch.int32, device=dev)
pileup("pieces", 8, d_again)
assert torch.equal(d_again, d_rows[("wide", 8)])
pileup("targets", 8, row_off=d_row_off.data_ptr())
torch.cuda.synchronize()
assert d_row_off.cpu().tolist() == [TARGET * i for i in range(len(targets) + 1)]
t8, w8 = d_rows[("targets", 8)].view(-1, TARGET, 8), d_rows[("wide", 8)].view(-1, 8)
inside = [i for i, (c, beg, end) in enumerate(targets.tolist()) if c == 0 and end <= SPAN]
for i in inside[::max(len(inside) // 200, 1)]:
    assert torch.equal(t8[i], w8[int(targets["beg"][i]):int(targets["end"][i])]), i
depth = w8[:, :5].sum(dim=1, dtype=torch.int64)
say("wide: mean depth %.3f, max %d, %d positions without a base; %d deletions, %d insertions counted" % (
    float(depth.double().mean()), int(depth.max()), int((depth == 0).sum()), int(w8[:, 5].sum()), int(w8[:, 7].sum())))
say("checked: the 16-column rows folded are the 8-column rows (both region sets); the span cut into 1 000 regions gives the rows of the one region; "
    "%d targets inside the span hold the wide rows of their positions; row_off of the targets" % len(inside[::max(len(inside) // 200, 1)]))
say("not measured: the host-buffer flavour, counters of any kernel")
say("source hash (tools/csrc_hash.py): %s" % csrc_sha())
if len(sys.argv) > 4:
    open(sys.argv[4], "w").write("tools/exp/time_bam_pileup.py %d %d %d on one MI355X, device-resident: every call once per round between two device "
                                 "events, %d rounds after 2 warm-up rounds, medians\n" % (N_PAIRS, N_GENOME, REPEATS, REPEATS) + "\n".join(lines) + "\n")
