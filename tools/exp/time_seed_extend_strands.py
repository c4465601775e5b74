"""Seed-and-extend on both strands against the forward-only call, on bench.py's seed_extend workload:

    python tools/exp/time_seed_extend_strands.py [genome_bp=3000000000] [reads=1250000] [repeats=8] [--chunk N] [--profile]

The genome, the device-built index (Occ k = 128 over n_alphabet, suffix-array samples at rate 32), SeedParams(20, 10, 16, 25),
the scoring (-5, -1, 1, -1) and the reads (synth_gpu.reads_from_genome, 150 bp, seed 5) are those of bench.py's seed_extend
leg.  A seeded half of the reads is turned into its reverse complement on the device (bg_revcomp_batch_dev).  After a warm-up,
three calls are timed with events, alternating over the repeats:
    fwd_only    bg_seed_extend_batch_dev on the forward reads (bench.py's figure)
    both_fwd    bg_seed_extend_strands_batch_dev, strands = 3, on the same reads
    both_half   the same on the half-reversed set
One JSON line: reads/s of each call (median over the repeats), mapped fraction, fraction at the origin (|ref_start - start|
<= 8), fraction on the strand the read was drawn from, totals, and the per-stage kernel ms of one more call of each (ctx
timing).  It checks that both_fwd gives fwd_only's alignment wherever the forward strand wins, and nothing where it maps none.
--chunk N sets the ctx option seed_chunk_reads (caller reads per pass) for all three calls.  --profile makes exactly one
stranded call (both_fwd) after the index is built, for `rocprofv3 --kernel-trace --stats`, and prints nothing else."""
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
from rust_bio_amd import _lib, synth_gpu  # noqa: E402
from rust_bio_amd.fmindex import FMIndex  # noqa: E402
from rust_bio_amd.pairwise import MIN_SCORE, Scoring  # noqa: E402
from rust_bio_amd.pipeline import SeedParams, attach_text, revcomp_dev, seed_extend_dev, seed_extend_strands_dev  # noqa: E402
from rust_bio_amd.suffix_array import bwt_dev, sample_dev, suffix_array_dev  # noqa: E402

N_ALPHABET = b"ACGTNacgtn"
ap = argparse.ArgumentParser()
ap.add_argument("genome", nargs="?", type=float, default=3e9)
ap.add_argument("reads", nargs="?", type=float, default=1.25e6)
ap.add_argument("repeats", nargs="?", type=int, default=8)
ap.add_argument("--chunk", type=int, default=0)
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()
n_genome, n_reads, repeats = int(args.genome), int(args.reads), args.repeats
L = 150
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

reads, starts = synth_gpu.reads_from_genome(g_dev, n_reads, L, seed=5)
d_roff = torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * L
rc = torch.empty_like(reads)
revcomp_dev(n_reads, reads.data_ptr(), d_roff.data_ptr(), rc.data_ptr(), ctx=ctx, stream=stream)
rev = torch.from_numpy(np.random.default_rng(7).random(n_reads) < 0.5).to(dev)
half = torch.where(rev[:, None], rc.view(n_reads, L), reads.view(n_reads, L)).reshape(-1).contiguous()
del rc

prm = SeedParams(20, 10, 16, 25)
sc = Scoring.from_scores(-5, -1, 1, -1)
stride = 2 * L + 2 * prm.pad + 4
out = {}
for name in ("fwd_only", "both_fwd", "both_half"):
    out[name] = {"hits": torch.empty(n_reads * 96, dtype=torch.uint8, device=dev),
                 "ops": torch.empty(n_reads * stride, dtype=torch.uint8, device=dev),
                 "strand": torch.empty(n_reads, dtype=torch.uint8, device=dev), "tot": np.zeros(2, dtype=np.uint64)}


def call(name):
    o = out[name]
    if name == "fwd_only":
        seed_extend_dev(fm, sc, n_reads, reads.data_ptr(), d_roff.data_ptr(), L, o["hits"].data_ptr(), o["ops"].data_ptr(), stride, prm,
                        stream, o["tot"])
    else:
        rd = reads if name == "both_fwd" else half
        seed_extend_strands_dev(fm, sc, n_reads, rd.data_ptr(), d_roff.data_ptr(), L, o["hits"].data_ptr(), o["strand"].data_ptr(),
                                o["ops"].data_ptr(), stride, prm, _lib.STRAND_BOTH, stream, o["tot"])


names = list(out)
ctx.set_option("seed_chunk_reads", args.chunk)
if args.profile:
    call("both_fwd")
    torch.cuda.synchronize()
    sys.exit(0)
for name in names:  # warm-up: code objects, scratch of both pass sizes
    call(name)
    call(name)
torch.cuda.synchronize()
ms = {n: [] for n in names}
for rep in range(repeats):
    order = names if rep % 2 == 0 else names[::-1]
    for name in order:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call(name)
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1))

stages = {}
for name in names:
    ctx.enable_timing(True)
    call(name)
    torch.cuda.synchronize()
    tm = ctx.timing()
    ctx.enable_timing(False)
    stages[name] = {"seed_search": round(tm["fm_ms"], 3), "align_fill": round(tm["fill_ms"], 3),
                    "align_traceback": round(tm["traceback_ms"], 3)}

res = {"workload": f"{n_reads} x {L} bp reads vs a {n_genome} bp genome (bench.py seed_extend leg), half of them reverse-complemented "
                   "for both_half", "index_build_s": round(t_index, 2), "repeats": repeats, "seed_chunk_reads": args.chunk}
want_rev = rev.to(torch.uint8)
for name in names:
    o = out[name]
    h32 = o["hits"].view(torch.int32).view(n_reads, 24)
    h64 = o["hits"].view(torch.int64).view(n_reads, 12)
    mapped = h32[:, 0] > MIN_SCORE
    near = ((h64[:, 9] - starts).abs() <= 8) & mapped
    if name == "fwd_only":
        on_strand = mapped
    else:
        on_strand = mapped & (o["strand"] == (want_rev if name == "both_half" else 0))
    med = float(np.median(ms[name]))
    res[name] = {"reads_per_s": round(n_reads / (med * 1e-3), 1), "ms_median": round(med, 3), "ms_min": round(min(ms[name]), 3),
                 "ms_all": [round(x, 3) for x in ms[name]], "mapped_frac": round(mapped.float().mean().item(), 4),
                 "mapped_at_origin_frac": round(near.float().mean().item(), 4),
                 "at_origin_on_strand_frac": round((near & on_strand).float().mean().item(), 4),
                 "seed_hits": int(o["tot"][0]), "candidates": int(o["tot"][1]), "kernel_ms": stages[name]}
res["both_over_fwd_rate"] = round(res["both_fwd"]["reads_per_s"] / res["fwd_only"]["reads_per_s"], 3)
res["both_half_over_fwd_rate"] = round(res["both_half"]["reads_per_s"] / res["fwd_only"]["reads_per_s"], 3)
# both_fwd against fwd_only: the same alignment (record, window, operations) wherever the forward strand wins; where the
# reverse strand wins it scores higher than the forward one; unmapped where the forward-only call maps nothing and nor does revcomp
a, b = out["fwd_only"], out["both_fwd"]
ha, hb = a["hits"].view(n_reads, 96), b["hits"].view(n_reads, 96)
fw = b["strand"] == _lib.HIT_FORWARD
same_rec = (ha[:, :56] == hb[:, :56]).all(dim=1) & (ha[:, 64:88] == hb[:, 64:88]).all(dim=1)  # aln up to ops_off; window / ref span
oa, ob = a["ops"].view(n_reads, stride), b["ops"].view(n_reads, stride)
n_ops = ha.view(torch.int32)[:, 7].to(torch.int64)
tail = torch.arange(stride, device=dev)[None, :] >= (stride - n_ops)[:, None]
same_ops = ((oa == ob) | ~tail).all(dim=1)
sa32, sb32 = ha.view(torch.int32)[:, 0], hb.view(torch.int32)[:, 0]
rv = b["strand"] == _lib.HIT_REVERSE
res["check_both_fwd_vs_fwd_only"] = {
    "forward_winners": int(fw.sum().item()), "reverse_winners": int(rv.sum().item()),
    "forward_winners_differing": int((fw & ~(same_rec & same_ops)).sum().item()),
    "reverse_winners_not_above_forward": int((rv & (sb32 <= sa32)).sum().item()),
    "unmapped_but_forward_mapped": int(((b["strand"] == _lib.HIT_NONE) & (sa32 > MIN_SCORE)).sum().item())}
ok = all(v == 0 for k, v in res["check_both_fwd_vs_fwd_only"].items() if not k.endswith("winners"))
res["check_ok"] = ok
print(json.dumps(res))
sys.exit(0 if ok else 1)
