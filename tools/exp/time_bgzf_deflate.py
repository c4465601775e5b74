"""Device-resident timing of bg_bgzf_deflate_dev next to bg_bgzf_frame_dev, in one process
([BG_SO=<variant .so>] python tools/exp/time_bgzf_deflate.py [PAIRS] [GENOME_BP] [REPEATS] [OUT]), on the batch of tools/exp/time_bam.py (the set-up
below is that tool's): the coordinate-sorted BAM records of PAIRS (default 500 000) pairs of 150 bp, 385 MB.
  * bg_bgzf_deflate_dev (reads its total back) and bg_bgzf_frame_dev over the sorted records, each once per round between two
    device events; after 2 warm-up rounds REPEATS (default 9) rounds, medians with the rounds' min and max;
  * the yardstick: bg_bam_emit_batch_dev, the record writer that feeds the call, timed in the same rounds;
  * output bytes and the ratio to the input for three inputs: the BAM records, the SAM text of the same reads, their FASTQ text;
  * zlib level 1 (raw deflate, one stream a payload) over the same payloads on 16 host threads: its size and its wall time.
The compressed file is checked once on the host: gzip.decompress gives the sorted records back and the block table is the one
found by walking BSIZE.  With BG_SO (a knock-out build of tools/exp/ko_build.sh: -DDFL_KO_TAIL stops behind the matches,
-DDFL_KO_EXTEND extends no candidate) the bytes are wrong: the three timings only."""
import gzip
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
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
d_file = torch.zeros(framed, dtype=torch.uint8, device=dev)
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
d_block_off = torch.zeros(n_blocks + 1, dtype=torch.int64, device=dev)
d_zfile = torch.zeros(framed, dtype=torch.uint8, device=dev)
out_bytes = {}


def deflate():
    out_bytes["bam"] = bam.bgzf_deflate_dev(d_bam_sorted.data_ptr(), bam_total, d_zfile.data_ptr(), framed, bam.BGZF_EOF, stream, ctx=ctx,
                                            d_block_off=d_block_off.data_ptr())


CALLS = [
    ("bam_emit", "bg_bam_emit_batch_dev (the yardstick: the writer that feeds the call)",
     lambda: bam.emit_dev(*emit_args, d_bam.data_ptr(), bam_total, d_off.data_ptr(), **emit_kw)),
    ("frame", "bg_bgzf_frame_dev over the sorted records, with the end-of-file block",
     lambda: bam.bgzf_frame_dev(d_bam_sorted.data_ptr(), bam_total, d_file.data_ptr(), framed, bam.BGZF_EOF, stream, ctx=ctx)),
    ("deflate", "bg_bgzf_deflate_dev over the sorted records, with the block table and the end-of-file block", deflate),
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
say("%s: %d pairs = %d reads of %d bp on a genome of %d bp in 3 contigs; BAM records %.1f MB in %d blocks" % (os.path.basename(_lib.SO_PATH), N_PAIRS, N, L, N_GENOME, bam_total / 1e6, n_blocks))
for key, name, _ in CALLS:
    t = sorted(ms[key])
    med[key] = t[len(t) // 2]
    say("%-100s median %8.3f ms (min %.3f max %.3f)" % (name, med[key], t[0], t[-1]))
say("bg_bgzf_deflate_dev: %.1f GB/s of input; deflate / bg_bam_emit_batch_dev = %.2f; deflate / frame = %.1f" % (
    bam_total / med["deflate"] / 1e6, med["deflate"] / med["bam_emit"], med["deflate"] / med["frame"]))
if os.environ.get("BG_SO"):
    if len(sys.argv) > 4:
        open(sys.argv[4], "w").write("\n".join(lines) + "\n")
    sys.exit(0)


def zlib1(data):
    """(bytes of the raw deflate streams + 26 of framing a payload, seconds) of zlib level 1, a payload a task, 16 threads"""
    cut = [data[a:a + bam.PAYLOAD] for a in range(0, len(data), bam.PAYLOAD)]

    def one(d):
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        return len(z.compress(d)) + len(z.flush()) + 26
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        total = sum(ex.map(one, cut))
    return total, time.perf_counter() - t0


for name, d_in, total in (("the BAM records", d_bam_sorted, bam_total), ("the SAM text of the same reads", d_text_sorted, sam_total),
                          ("their FASTQ text", d_fq, d_fq.numel())):
    cap = bam.framed_bytes(total)
    d_tmp = d_zfile if cap <= d_zfile.numel() else torch.zeros(cap, dtype=torch.uint8, device=dev)
    got = bam.bgzf_deflate_dev(d_in.data_ptr(), total, d_tmp.data_ptr(), cap, 0, stream, ctx=ctx)
    host = d_in[:total].cpu().numpy().tobytes()
    assert gzip.decompress(d_tmp[:got].cpu().numpy().tobytes()) == host
    z, sec = zlib1(host)
    say("%-32s %11d bytes -> %11d (%.3f of the input; stored %d); zlib level 1 on 16 host threads %11d (%.3f) in %.0f ms; ours / zlib = %.3f" % (
        name, total, got, got / total, cap, z, z / total, sec * 1e3, got / z))
# the bytes are right: the file decompresses to the sorted records, and the table holds the block starts
deflate()
torch.cuda.synchronize()
file = d_zfile[:out_bytes["bam"]].cpu().numpy().tobytes()
assert gzip.decompress(file) == d_bam_sorted.cpu().numpy().tobytes() and file.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
at, starts = 0, []
while at < len(file) - 28:
    starts.append(at)
    at += struct.unpack_from("<H", file, at + 16)[0] + 1
assert d_block_off.cpu().tolist() == starts + [len(file) - 28]
say("checked: gzip.decompress(file) == the sorted records (all three inputs round-trip); the block table is the walk over BSIZE")
say("not measured: the host-buffer flavour, counters of any kernel")
if len(sys.argv) > 4:
    open(sys.argv[4], "w").write("tools/exp/time_bgzf_deflate.py %d %d %d on one MI355X, device-resident: every call once per round between two device "
                                 "events, %d rounds after 2 warm-up rounds, medians\n" % (N_PAIRS, N_GENOME, REPEATS, REPEATS) + "\n".join(lines) + "\n")
