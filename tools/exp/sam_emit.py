"""SAM emission (bg_sam_emit_batch_dev) against the mapping call that feeds it, on bench.py's seed_extend workload:

    python tools/exp/sam_emit.py [genome_bp=3000000000] [reads=1250000] [repeats=7] [--out profiles/sam_emit.json] [--profile LANES]

Genome, device-built index, SeedParams(20, 10, 16, 25), scoring (-5, -1, 1, -1) and reads are those of
tools/exp/time_seed_extend_multi.py (bench.py's seed_extend leg; a seeded half of the reads reverse-complemented).  The reads
are written as a four-line FASTQ in HBM and parsed by bg_fastq_parse_dev; the multi call (K = 4, both strands) maps them; the
genome is declared as 24 contigs.  After a warm-up, event-timed in one process, interleaved over the repeats:
    mapping      bg_seed_extend_multi_batch_dev (the yardstick: the parent's code, untouched by the emission)
    emit_16/32   bg_sam_emit_batch_dev with NM and MD, one line per read, 16 or 32 lanes per line in the write pass
    size         the same call with d_out = NULL: the length pass, the scan and the read-back of the total
    emit_sec     emit_16 with BG_SAM_SECONDARY (up to four lines per read)
One JSON line (also written to --out): medians, bytes written, GB/s, the split length pass / write passes (write_pass_ms is
the full call minus the sizing call: the write kernel and the CIGAR / MD kernel), 16 against 32 lanes, and emission / mapping.  --profile LANES makes exactly one emission
call after the set-up, for `rocprofv3 --kernel-trace --stats`, and prints nothing else."""
import argparse
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.init()
from rust_bio_amd import _lib, fastq, sam, synth_gpu  # noqa: E402
from rust_bio_amd.fmindex import FMIndex  # noqa: E402
from rust_bio_amd.pairwise import Scoring  # noqa: E402
from rust_bio_amd.pipeline import MultiParams, SeedParams, attach_text, revcomp_dev, seed_extend_multi_dev  # noqa: E402
from rust_bio_amd.suffix_array import bwt_dev, sample_dev, suffix_array_dev  # noqa: E402

N_ALPHABET = b"ACGTNacgtn"
ap = argparse.ArgumentParser()
ap.add_argument("genome", nargs="?", type=float, default=3e9)
ap.add_argument("reads", nargs="?", type=float, default=1.25e6)
ap.add_argument("repeats", nargs="?", type=int, default=7)
ap.add_argument("--out", default="")
ap.add_argument("--profile", type=int, default=0)
args = ap.parse_args()
n_genome, n_reads, repeats = int(args.genome), int(args.reads), max(args.repeats, 5)
L, K, CAP = 150, 4, 60
dev = torch.device("cuda:0")
ctx = _lib.Context(0)
stream = torch.cuda.current_stream().cuda_stream

t0 = time.perf_counter()
g_dev = synth_gpu.genome(n_genome, seed=33, device=dev)
d_sa = suffix_array_dev(g_dev, ctx=ctx)
d_b = bwt_dev(g_dev, d_sa, ctx=ctx)
ssa = sample_dev(d_sa, d_b, ord("$"), 32, ctx=ctx)
fm = FMIndex.from_device(d_b, 128, N_ALPHABET, ctx=ctx)
fm._d_bwt = None
del d_sa, d_b
ssa.attach(fm)
attach_text(fm, d_text=g_dev)
torch.cuda.synchronize()
t_index = time.perf_counter() - t0

reads, _ = synth_gpu.reads_from_genome(g_dev, n_reads, L, seed=5)
d_roff = torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * L
rc = torch.empty_like(reads)
revcomp_dev(n_reads, reads.data_ptr(), d_roff.data_ptr(), rc.data_ptr(), ctx=ctx, stream=stream)
rev = torch.from_numpy(np.random.default_rng(7).random(n_reads) < 0.5).to(dev)
half = torch.where(rev[:, None], rc.view(n_reads, L), reads.view(n_reads, L))
del rc, reads

# the reads as FASTQ text in HBM: "@r<8 digits>\n<150 bases>\n+\n<150 qualities>\n", then bg_fastq_parse_dev
idx = torch.arange(n_reads, device=dev)
digits = torch.stack([(idx // 10 ** p) % 10 + 48 for p in range(7, -1, -1)], dim=1).to(torch.uint8)
qual = (torch.randint(0, 41, (n_reads, L), device=dev, generator=torch.Generator(device=dev).manual_seed(3)) + 33).to(torch.uint8)


def const(s):
    return torch.tensor(list(s), dtype=torch.uint8, device=dev).expand(n_reads, len(s))


d_fq = torch.cat([const(b"@r"), digits, const(b"\n"), half, const(b"\n+\n"), qual, const(b"\n")], dim=1).reshape(-1).contiguous()
del digits, qual, half, idx
n_parsed, status, _, d_recs, d_seq, d_seq_off, d_qual, _ = fastq.parse_dev(d_fq, ctx=ctx, stream=stream)
assert (n_parsed, status) == (n_reads, "ok"), (n_parsed, status)

n_contigs = 24
edges = np.linspace(0, n_genome, n_contigs + 1).astype(np.int64)
contigs = sam.Contigs([("chr%d" % (c + 1), int(edges[c]), int(edges[c + 1] - edges[c] - 1)) for c in range(n_contigs)])
d_contigs = torch.from_numpy(contigs.table.view(np.uint8).copy()).to(dev)
d_names = torch.from_numpy(contigs.names).to(dev)

prm = SeedParams(20, 10, 16, 25)
sc = Scoring.from_scores(-5, -1, 1, -1)
mp = MultiParams(K, -2**31, CAP)
stride = 2 * L + 2 * prm.pad + 4
d_hits = torch.empty(n_reads * K * 96, dtype=torch.uint8, device=dev)
d_ops = torch.empty(n_reads * K * stride, dtype=torch.uint8, device=dev)
d_strand = torch.empty(n_reads * K, dtype=torch.uint8, device=dev)
d_multi = torch.empty(n_reads * 16, dtype=torch.uint8, device=dev)
d_off = torch.empty(n_reads * K + 1, dtype=torch.int64, device=dev)
TAGS = sam.SAM_TAG_NM | sam.SAM_TAG_MD


def mapping():
    seed_extend_multi_dev(fm, sc, n_reads, d_seq.data_ptr(), d_seq_off.data_ptr(), L, d_hits.data_ptr(), d_multi.data_ptr(),
                          d_strand.data_ptr(), d_ops.data_ptr(), stride, prm, mp, _lib.STRAND_BOTH, stream)


def emit(flags, d_out, cap):
    return sam.emit_dev(fm, sam.SamParams(flags, K), n_reads, d_contigs.data_ptr(), n_contigs, d_names.data_ptr(), d_fq.data_ptr(),
                        d_recs.data_ptr(), d_seq.data_ptr(), d_qual.data_ptr(), d_hits.data_ptr(), d_strand.data_ptr(), d_ops.data_ptr(),
                        d_out.data_ptr() if d_out is not None else 0, cap, d_off.data_ptr(), d_multi=d_multi.data_ptr(), stream=stream)


mapping()
torch.cuda.synchronize()
total = {f: emit(f, None, 0) for f in (TAGS, TAGS | sam.SAM_SECONDARY)}
d_out = torch.empty(max(total.values()), dtype=torch.uint8, device=dev)


def lanes(n):
    ctx.set_option("sam_lanes", n)


calls = {"mapping": mapping,
         "emit_16": lambda: (lanes(16), emit(TAGS, d_out, total[TAGS])),
         "emit_32": lambda: (lanes(32), emit(TAGS, d_out, total[TAGS])),
         "size": lambda: emit(TAGS, None, 0),
         "emit_sec": lambda: (lanes(16), emit(TAGS | sam.SAM_SECONDARY, d_out, total[TAGS | sam.SAM_SECONDARY]))}
if args.profile:
    lanes(args.profile)
    emit(TAGS, d_out, total[TAGS])
    torch.cuda.synchronize()
    sys.exit(0)
names = list(calls)
for name in names:  # warm-up: code objects, scratch
    calls[name]()
    calls[name]()
torch.cuda.synchronize()
ms = {n: [] for n in names}
for rep in range(repeats):
    for name in (names if rep % 2 == 0 else names[::-1]):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        calls[name]()
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1))

# what was written: the 16- and the 32-lane text are the same bytes, one line per slot that has a length
lanes(32)
emit(TAGS, d_out, total[TAGS])
torch.cuda.synchronize()
text32 = d_out[:total[TAGS]].clone()
lanes(16)
emit(TAGS, d_out, total[TAGS])
torch.cuda.synchronize()
n_lines = int((d_out[:total[TAGS]] == 10).sum().item())
off = d_off.cpu()
check_ok = bool((text32 == d_out[:total[TAGS]]).all().item()) and n_lines == n_reads == int((off[1:] > off[:-1]).sum().item())
lanes(0)

med = {n: float(np.median(ms[n])) for n in names}
res = {"workload": f"{n_reads} x {L} bp reads as FASTQ in HBM, half of them reverse-complemented, vs a {n_genome} bp genome in {n_contigs} "
                   f"contigs (bench.py seed_extend leg), multi call K = {K}, NM + MD",
       "index_build_s": round(t_index, 2), "repeats": repeats,
       "ms_median": {n: round(med[n], 3) for n in names}, "ms_all": {n: [round(x, 3) for x in ms[n]] for n in names},
       "mapping_reads_per_s": round(n_reads / (med["mapping"] * 1e-3), 1),
       "bytes_written": total[TAGS], "bytes_per_line": round(total[TAGS] / n_reads, 1),
       "emit_GB_per_s": {n: round(total[TAGS] / (med[n] * 1e-3) / 1e9, 2) for n in ("emit_16", "emit_32")},
       "length_pass_scan_readback_ms": round(med["size"], 3),
       "write_pass_ms": {n: round(med[n] - med["size"], 3) for n in ("emit_16", "emit_32")},
       "lanes_32_over_16_time": round(med["emit_32"] / med["emit_16"], 4),
       "emission_over_mapping": round(min(med["emit_16"], med["emit_32"]) / med["mapping"], 4),
       "default_lanes_emission_over_mapping": round(med["emit_16"] / med["mapping"], 4),
       "secondary": {"bytes_written": total[TAGS | sam.SAM_SECONDARY], "ms_median": round(med["emit_sec"], 3),
                     "over_mapping": round(med["emit_sec"] / med["mapping"], 4)},
       "check_ok": check_ok}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(line + "\n")
sys.exit(0 if check_ok else 1)
