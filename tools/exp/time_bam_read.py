"""Device-resident timing of reading BAM, in one process (python tools/exp/time_bam_read.py [PAIRS] [GENOME_BP] [REPEATS] [OUT]), on the
batch of tools/exp/time_bgzf_inflate.py (the set-up below is that tool's): the coordinate-sorted BAM records of PAIRS (default
500 000) pairs of 150 bp behind their header, deflated by bg_bgzf_deflate_dev with the end-of-file block into one .bam in HBM.
The file is read back (bg_bgzf_blocks_dev, bg_bgzf_inflate_dev, bg_bam_header_parse), then each call once per round between two
device events; after 2 warm-up rounds REPEATS (default 9) rounds, medians with the rounds' min and max:
  * bg_bam_records_dev (table given; two read-backs) next to bg_bgzf_blocks_dev on the file;
  * bg_bam_reads_dev (BG_BAM_READS_ORIGINAL, exclude 0x900, all columns and src) next to bg_bam_emit_batch_dev, the call that
    wrote the records, and next to a device-to-device copy of as many bytes as the bases and qualities have;
  * bg_bam_sort_keys_dev next to bg_sam_sort_keys_dev; bg_bam_index_blocks_dev next to bg_bam_index_dev;
  * the candidates per record.
The record table is compared with the sorter's offsets, the reads with the parsed FASTQ through src and the sort's permutation, the
keys with the sorted hits' keys, on the device."""
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

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
d_copy = torch.zeros(bam_total, dtype=torch.uint8, device=dev)


def sort(d_in, total, d_out):
    sam.sort_dev(N, d_key.data_ptr(), d_in.data_ptr(), d_off.data_ptr(), total, d_out.data_ptr(), total, d_sorted_off.data_ptr(),
                 d_perm.data_ptr(), stream=stream, ctx=ctx)


markdup()
keys()
sam.emit_dev(*emit_args, d_text.data_ptr(), sam_total, d_off.data_ptr(), **emit_kw)
sort(d_text, sam_total, d_text_sorted)
bam.emit_dev(*emit_args, d_bam.data_ptr(), bam_total, d_off.data_ptr(), **emit_kw)
sort(d_bam, bam_total, d_bam_sorted)
n_blocks = (bam_total + bam.PAYLOAD - 1) // bam.PAYLOAD



# ---- the file, read back
head = bam.header(contigs, sam.SAM_SO_COORDINATE)
H = len(head)
d_stream_in = torch.cat([torch.from_numpy(np.frombuffer(head, np.uint8).copy()).to(dev), d_bam_sorted])
total = int(d_stream_in.numel())
cap = bam.framed_bytes(total, bam.BGZF_EOF)
d_file = torch.zeros(cap, dtype=torch.uint8, device=dev)
size = bam.bgzf_deflate_dev(d_stream_in.data_ptr(), total, d_file.data_ptr(), cap, bam.BGZF_EOF, stream, ctx=ctx)
nb = (total + bam.PAYLOAD - 1) // bam.PAYLOAD + 1
d_block_off = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
d_out_off = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
d_stream = torch.zeros(total, dtype=torch.uint8, device=dev)


def blocks():
    assert bam.bgzf_blocks_dev(d_file.data_ptr(), size, d_block_off.data_ptr(), d_out_off.data_ptr(), nb, stream, ctx=ctx) == (nb, total)


blocks()
bam.bgzf_inflate_dev(d_file.data_ptr(), size, nb, d_block_off.data_ptr(), d_out_off.data_ptr(), d_stream.data_ptr(), total, stream=stream, ctx=ctx)
assert torch.equal(d_stream, d_stream_in)
_, contigs_read, body_off = bam.read_header(lambda k: d_stream[:k].cpu().numpy())
assert body_off == H and (contigs_read.table["start"] == contigs.table["start"]).all() and (contigs_read.table["len"] == contigs.table["len"]).all()
n_rec, n_cand = bam.records_dev(d_stream.data_ptr(), total, body_off, 3, stream=stream, ctx=ctx)
d_rec_off = torch.zeros(n_rec + 1, dtype=torch.int64, device=dev)


def records():
    assert bam.records_dev(d_stream.data_ptr(), total, body_off, 3, d_rec_off.data_ptr(), n_rec, stream=stream, ctx=ctx) == (n_rec, n_cand)


records()
reads_kw = dict(flags=bam.BAM_READS_ORIGINAL, exclude=0x900, stream=stream, ctx=ctx)
k, sb, qb = bam.reads_dev(n_rec, d_stream.data_ptr(), d_rec_off.data_ptr(), 3, **reads_kw)
r_recs = torch.zeros(k * 56, dtype=torch.uint8, device=dev)
r_seq, r_qual = torch.zeros(sb, dtype=torch.uint8, device=dev), torch.zeros(qb, dtype=torch.uint8, device=dev)
r_so, r_qo, r_src = (torch.zeros(k + 1, dtype=torch.int64, device=dev) for _ in range(3))
d_cols_in, d_cols_out = torch.zeros(sb + qb, dtype=torch.uint8, device=dev), torch.zeros(sb + qb, dtype=torch.uint8, device=dev)
r_key = torch.zeros(n_rec, dtype=torch.int64, device=dev)
d_bai = [torch.zeros(1, dtype=torch.uint8, device=dev)] * 2


def reads():
    assert bam.reads_dev(n_rec, d_stream.data_ptr(), d_rec_off.data_ptr(), 3, r_recs.data_ptr(), k, r_seq.data_ptr(), sb, r_so.data_ptr(), r_qual.data_ptr(), qb,
                         r_qo.data_ptr(), r_src.data_ptr(), **reads_kw) == (k, sb, qb)


def emit():
    bam.emit_dev(*emit_args, d_bam.data_ptr(), bam_total, d_off.data_ptr(), **emit_kw)


def keys_records():
    bam.sort_keys_records_dev(n_rec, d_stream.data_ptr(), d_rec_off.data_ptr(), d_contigs.data_ptr(), 3, r_key.data_ptr(), stream=stream, ctx=ctx)


def index_written():
    return bam.index_dev(N, d_bam_sorted.data_ptr(), d_sorted_off.data_ptr(), d_contigs.data_ptr(), 3, d_bai[0].data_ptr() if d_bai[0].numel() > 1 else 0,
                         d_bai[0].numel() if d_bai[0].numel() > 1 else 0, stream=stream, ctx=ctx)


def index_read():
    return bam.index_blocks_dev(n_rec, d_stream.data_ptr(), d_rec_off.data_ptr(), d_contigs.data_ptr(), 3, nb, d_block_off.data_ptr(), d_out_off.data_ptr(),
                                d_bai[1].data_ptr() if d_bai[1].numel() > 1 else 0, d_bai[1].numel() if d_bai[1].numel() > 1 else 0, stream=stream, ctx=ctx)


d_bai = [torch.zeros(index_written(), dtype=torch.uint8, device=dev), torch.zeros(index_read(), dtype=torch.uint8, device=dev)]
CALLS = [
    ("blocks", "bg_bgzf_blocks_dev over the file, both tables (the yardstick of the record table)", blocks),
    ("records", "bg_bam_records_dev over the inflated stream, the table given", records),
    ("emit", "bg_bam_emit_batch_dev (the yardstick of the reads: the call that wrote the records)", emit),
    ("copy", "a device-to-device copy of as many bytes as the bases and qualities", lambda: d_cols_out.copy_(d_cols_in)),
    ("reads", "bg_bam_reads_dev, BG_BAM_READS_ORIGINAL, exclude 0x900, all columns and src", reads),
    ("keys_hits", "bg_sam_sort_keys_dev over the hits", keys),
    ("keys_records", "bg_bam_sort_keys_dev over the records", keys_records),
    ("index_written", "bg_bam_index_dev over the sorted records as written (closed-form offsets)", index_written),
    ("index_read", "bg_bam_index_blocks_dev over the stream read back, with the file's block table", index_read),
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
say("%s: %d pairs = %d reads of %d bp on a genome of %d bp in 3 contigs; the stream %.1f MB (header %d bytes) -> a file of %.1f MB in %d blocks; %d records" % (
    os.path.basename(_lib.SO_PATH), N_PAIRS, N, L, N_GENOME, total / 1e6, H, size / 1e6, nb, n_rec))
for key, name, _ in CALLS:
    t = sorted(ms[key])
    med[key] = t[len(t) // 2]
    say("%-100s median %8.3f ms (min %.3f max %.3f)" % (name, med[key], t[0], t[-1]))
say("positions judged: %.2f x the block table's (%.1f MB against %.1f MB); records / blocks = %.2f" % (
    (total - H) / size, (total - H) / 1e6, size / 1e6, med["records"] / med["blocks"]))
say("candidates: %d for %d records = %.4f a record" % (n_cand, n_rec, n_cand / max(n_rec, 1)))
say("reads / emit = %.3f; reads / copy = %.1f; %.1f GB/s of bases and qualities written; keys: records / hits = %.2f; index: read / written = %.3f" % (
    med["reads"] / med["emit"], med["reads"] / med["copy"], (sb + qb) / med["reads"] / 1e6, med["keys_records"] / med["keys_hits"],
    med["index_read"] / med["index_written"]))
# ---- checks, on the device
lens = d_sorted_off[1:] - d_sorted_off[:-1]
slots = d_perm[lens > 0]  # the slot (= read: K is 1) of the i-th record of the sorted stream
assert n_rec == int((lens > 0).sum()) and torch.equal(d_rec_off[:-1], d_sorted_off[:-1][lens > 0] + H) and int(d_rec_off[-1]) == total
assert k == N and sb == N * L and qb == N * L
read_of = slots[r_src[:k]]
assert torch.equal(r_seq.view(N, L), d_seq[:N * L].view(N, L)[read_of]) and torch.equal(r_qual.view(N, L), d_qual[:N * L].view(N, L)[read_of])
keys()
assert torch.equal(r_key, d_key[slots])
say("checked: the table is the sorter's offsets behind the header, every read's bases and qualities are the parsed FASTQ's (through src and the "
    "sort's permutation), the records' keys are the hits' keys")
say("not measured: the host-buffer flavours, bg_bam_header_parse (host), counters of any kernel")
say("source hash (tools/csrc_hash.py): %s" % csrc_sha())
if len(sys.argv) > 4:
    open(sys.argv[4], "w").write("tools/exp/time_bam_read.py %d %d %d on one MI355X, device-resident: every call once per round between two device "
                                 "events, %d rounds after 2 warm-up rounds, medians\n" % (N_PAIRS, N_GENOME, REPEATS, REPEATS) + "\n".join(lines) + "\n")
