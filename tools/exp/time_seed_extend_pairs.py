"""Read pairs in seed-and-extend against the strands call on the same reads, on bench.py's seed_extend workload:

    python tools/exp/time_seed_extend_pairs.py [genome_bp=3000000000] [pairs=625000] [repeats=8] [--profile]

The genome, the device-built index (Occ k = 128 over n_alphabet, suffix-array samples at rate 32), SeedParams(20, 10, 16, 25)
and the scoring (-5, -1, 1, -1) are those of bench.py's seed_extend leg; the reads are 2 x `pairs` x 150 bp interleaved mates of
fragments of 300-500 bp (synth_gpu.read_pairs_from_genome, seed 5), PairParams(0, 1000, 17).  After a warm-up, two calls are
timed with events, alternating over the repeats:
    pairs     bg_seed_extend_pairs_batch_dev
    strands   bg_seed_extend_strands_batch_dev, strands = 3, on the same 2n reads
One JSON line: reads/s of each (median over the repeats), the proper fraction, the fraction of pairs with both mates at their
origin (|ref_start - origin| <= 8) under each call, and the pair stage's cost: pairs minus strands (median ms; the two calls
differ only in their last stage).  The kernel itself: --profile makes exactly one pairs call after the index is built, for
`rocprofv3 --kernel-trace --stats` (se_pair_kernel against se_best_kernel<2> of one strands call), and prints nothing else."""
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
from rust_bio_amd.pipeline import PairParams, SeedParams, attach_text, seed_extend_pairs_dev, seed_extend_strands_dev  # noqa: E402
from rust_bio_amd.suffix_array import bwt_dev, sample_dev, suffix_array_dev  # noqa: E402

N_ALPHABET = b"ACGTNacgtn"
ap = argparse.ArgumentParser()
ap.add_argument("genome", nargs="?", type=float, default=3e9)
ap.add_argument("pairs", nargs="?", type=float, default=6.25e5)
ap.add_argument("repeats", nargs="?", type=int, default=8)
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()
n_genome, n_pairs, repeats = int(args.genome), int(args.pairs), args.repeats
n_reads, L = 2 * n_pairs, 150
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

reads, origin, rev = synth_gpu.read_pairs_from_genome(g_dev, n_pairs, L, seed=5, min_frag=300, max_frag=500)
d_roff = torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * L

prm = SeedParams(20, 10, 16, 25)
pp = PairParams(0, 1000, 17)
sc = Scoring.from_scores(-5, -1, 1, -1)
stride = 2 * L + 2 * prm.pad + 4
out = {}
for name in ("pairs", "strands"):
    out[name] = {"hits": torch.empty(n_reads * 96, dtype=torch.uint8, device=dev),
                 "ops": torch.empty(n_reads * stride, dtype=torch.uint8, device=dev),
                 "strand": torch.empty(n_reads, dtype=torch.uint8, device=dev), "tot": np.zeros(2, dtype=np.uint64)}
d_pairs = torch.empty(n_pairs * 16, dtype=torch.uint8, device=dev)


def call(name):
    o = out[name]
    if name == "pairs":
        seed_extend_pairs_dev(fm, sc, n_pairs, reads.data_ptr(), d_roff.data_ptr(), L, o["hits"].data_ptr(), d_pairs.data_ptr(),
                              o["strand"].data_ptr(), o["ops"].data_ptr(), stride, prm, pp, stream, o["tot"])
    else:
        seed_extend_strands_dev(fm, sc, n_reads, reads.data_ptr(), d_roff.data_ptr(), L, o["hits"].data_ptr(), o["strand"].data_ptr(),
                                o["ops"].data_ptr(), stride, prm, _lib.STRAND_BOTH, stream, o["tot"])


names = list(out)
if args.profile:
    call("pairs")
    torch.cuda.synchronize()
    sys.exit(0)
for name in names:  # warm-up: code objects, scratch
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

res = {"workload": f"{n_pairs} pairs = {n_reads} x {L} bp interleaved mates (fragments 300-500 bp) vs a {n_genome} bp genome "
                   "(bench.py seed_extend leg's index and parameters), PairParams(0, 1000, 17)",
       "index_build_s": round(t_index, 2), "repeats": repeats}
ph = d_pairs.view(n_pairs, 16)
proper = ph[:, 12] == 1
for name in names:
    o = out[name]
    h32 = o["hits"].view(torch.int32).view(n_reads, 24)
    h64 = o["hits"].view(torch.int64).view(n_reads, 12)
    mapped = h32[:, 0] > MIN_SCORE
    near = ((h64[:, 9] - origin).abs() <= 8) & mapped
    both = near.view(n_pairs, 2).all(dim=1)
    med = float(np.median(ms[name]))
    res[name] = {"reads_per_s": round(n_reads / (med * 1e-3), 1), "ms_median": round(med, 3), "ms_min": round(min(ms[name]), 3),
                 "ms_all": [round(x, 3) for x in ms[name]], "mapped_frac": round(mapped.float().mean().item(), 4),
                 "both_mates_at_origin_frac": round(both.float().mean().item(), 4),
                 "seed_hits": int(o["tot"][0]), "candidates": int(o["tot"][1])}
res["pairs"]["proper_frac"] = round(proper.float().mean().item(), 4)
res["pairs_over_strands_rate"] = round(res["pairs"]["reads_per_s"] / res["strands"]["reads_per_s"], 3)
res["pair_stage_ms_est"] = round(res["pairs"]["ms_median"] - res["strands"]["ms_median"], 3)
# the two calls run the same stages up to the last one: equal totals; a pair that is not proper reports the strands call's hits
same_hits = (out["pairs"]["hits"].view(n_reads, 96) == out["strands"]["hits"].view(n_reads, 96)).all(dim=1).view(n_pairs, 2).all(dim=1)
res["check"] = {"totals_equal": bool((out["pairs"]["tot"] == out["strands"]["tot"]).all()),
                "improper_pairs_differing": int((~proper & ~same_hits).sum().item())}
ok = res["check"]["totals_equal"] and res["check"]["improper_pairs_differing"] == 0
res["check_ok"] = ok
print(json.dumps(res))
sys.exit(0 if ok else 1)
