"""Device-resident timing of bg_bgzf_blocks_dev and bg_bgzf_inflate_dev, in one process
([BG_SO=<variant .so>] python tools/exp/time_bgzf_inflate.py [PAIRS] [GENOME_BP] [REPEATS] [OUT]), on the batch of tools/exp/time_bgzf_deflate.py (the
set-up below is that tool's): the coordinate-sorted BAM records of PAIRS (default 500 000) pairs of 150 bp, 385 MB, deflated by
bg_bgzf_deflate_dev with the end-of-file block, and the same batch's FASTQ text deflated the same way.
  * bg_bgzf_blocks_dev (tables given; reads n_blocks, out_bytes and the error back) and bg_bgzf_inflate_dev (reads its error words
    back) over the compressed file, each once per round between two device events; after 2 warm-up rounds REPEATS (default 9)
    rounds, medians with the rounds' min and max;
  * three yardsticks in the same rounds: bg_bgzf_deflate_dev on the same bytes, a device-to-device copy of the payload, and
    (wall time, once) zlib.decompress over the blocks on 16 host threads;
  * the same two calls on the deflated FASTQ text.
The inflated bytes are compared with the input on the device, the block table with the deflater's.  With BG_SO (a knock-out
build of tools/exp/ko_build.sh: -DINF_KO_COPIES decodes and drops the tokens, -DINF_KO_DECODE builds a block's first tables and
stops) every block fails its checks: the timings only."""
import os
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


KO = bool(os.environ.get("BG_SO"))


class File:
    """an input deflated on the device, and the buffers both calls fill"""

    def __init__(self, d_in, total):
        self.d_in, self.total = d_in, total
        cap = bam.framed_bytes(total, bam.BGZF_EOF)
        self.d_file = torch.zeros(cap, dtype=torch.uint8, device=dev)
        n_payloads = (total + bam.PAYLOAD - 1) // bam.PAYLOAD
        self.d_dfl_off = torch.zeros(n_payloads + 1, dtype=torch.int64, device=dev)
        self.cap = cap
        self.deflate()
        self.n = n_payloads + 1  # the end-of-file block
        self.d_block_off = torch.zeros(self.n + 1, dtype=torch.int64, device=dev)
        self.d_out_off = torch.zeros(self.n + 1, dtype=torch.int64, device=dev)
        self.d_out = torch.zeros(total, dtype=torch.uint8, device=dev)
        self.d_status = torch.zeros(self.n, dtype=torch.uint8, device=dev)

    def deflate(self):
        self.size = bam.bgzf_deflate_dev(self.d_in.data_ptr(), self.total, self.d_file.data_ptr(), self.cap, bam.BGZF_EOF, stream, ctx=ctx,
                                         d_block_off=self.d_dfl_off.data_ptr())

    def blocks(self):
        assert bam.bgzf_blocks_dev(self.d_file.data_ptr(), self.size, self.d_block_off.data_ptr(), self.d_out_off.data_ptr(), self.n, stream, ctx=ctx) == (self.n, self.total)

    def inflate(self):
        try:
            bam.bgzf_inflate_dev(self.d_file.data_ptr(), self.size, self.n, self.d_block_off.data_ptr(), self.d_out_off.data_ptr(), self.d_out.data_ptr(),
                                 self.total, self.d_status.data_ptr(), stream, ctx=ctx)
        except bam.BgzfError:
            if not KO:
                raise


records, fq = File(d_bam_sorted, bam_total), File(d_fq, d_fq.numel())
CALLS = [
    ("deflate", "bg_bgzf_deflate_dev over the sorted records (the yardstick: the call that made the file)", records.deflate),
    ("copy", "a device-to-device copy of the payload", lambda: d_copy.copy_(d_bam_sorted)),
    ("blocks", "bg_bgzf_blocks_dev over the compressed records, both tables", records.blocks),
    ("inflate", "bg_bgzf_inflate_dev over the compressed records, with the status bytes", records.inflate),
    ("fq_blocks", "bg_bgzf_blocks_dev over the compressed FASTQ text", fq.blocks),
    ("fq_inflate", "bg_bgzf_inflate_dev over the compressed FASTQ text", fq.inflate),
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
say("%s: %d pairs = %d reads of %d bp on a genome of %d bp in 3 contigs; BAM records %.1f MB -> %.1f MB in %d blocks; FASTQ text %.1f MB -> %.1f MB in %d blocks" % (
    os.path.basename(_lib.SO_PATH), N_PAIRS, N, L, N_GENOME, bam_total / 1e6, records.size / 1e6, records.n, fq.total / 1e6, fq.size / 1e6, fq.n))
for key, name, _ in CALLS:
    t = sorted(ms[key])
    med[key] = t[len(t) // 2]
    say("%-100s median %8.3f ms (min %.3f max %.3f)" % (name, med[key], t[0], t[-1]))
say("bg_bgzf_inflate_dev: %.1f GB/s of payload; inflate / deflate = %.3f; inflate / copy = %.1f; blocks / inflate = %.3f" % (
    bam_total / med["inflate"] / 1e6, med["inflate"] / med["deflate"], med["inflate"] / med["copy"], med["blocks"] / med["inflate"]))
if not KO:
    for f in (records, fq):
        assert torch.equal(f.d_out, f.d_in[:f.total]) and not bool(f.d_status.any())
        assert f.d_block_off[:f.n].tolist() == f.d_dfl_off.tolist() and int(f.d_block_off[f.n]) == f.size
    say("checked: both inflated payloads equal their inputs, every status is 0, the block tables are the deflater's")
    file = records.d_file[:records.size].cpu().numpy().tobytes()
    off = records.d_block_off.cpu().tolist()
    members = [file[a:b] for a, b in zip(off, off[1:])]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        total = sum(ex.map(lambda m: len(zlib.decompress(m, 31)), members))
    sec = time.perf_counter() - t0
    assert total == bam_total
    say("zlib.decompress over the %d blocks on 16 host threads: %.0f ms (wall, once)" % (len(members), sec * 1e3))
say("not measured: the host-buffer flavours, counters of any kernel")
if len(sys.argv) > 4:
    open(sys.argv[4], "w").write("tools/exp/time_bgzf_inflate.py %d %d %d on one MI355X, device-resident: every call once per round between two device "
                                 "events, %d rounds after 2 warm-up rounds, medians\n" % (N_PAIRS, N_GENOME, REPEATS, REPEATS) + "\n".join(lines) + "\n")
