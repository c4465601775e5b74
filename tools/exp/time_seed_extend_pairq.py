"""The pairs-mapq call (a MAPQ for each mate, judged against the pair) against the paired call on the same reads, on bench.py's
seed_extend workload:

    python tools/exp/time_seed_extend_pairq.py [genome_bp=3000000000] [pairs=625000] [repeats=5] [--profile NAME]

The genome, the device-built index (Occ k = 128 over n_alphabet, suffix-array samples at rate 32), SeedParams(20, 10, 16, 25),
the scoring (-5, -1, 1, -1), the reads (2 x `pairs` x 150 bp interleaved mates of fragments of 300-500 bp,
synth_gpu.read_pairs_from_genome, seed 5) and PairParams(0, 1000, 17) are those of tools/exp/time_seed_extend_pairs.py;
PairQualityParams(min_score 0, mapq_cap 60).  After a warm-up, two calls are timed with events in one process, alternating over the
repeats:
    pairs     bg_seed_extend_pairs_batch_dev
    pairq     bg_seed_extend_pairs_mapq_batch_dev
One JSON line: the median ms and pairs/s of each, the ratio pairq / pairs of the medians, the proper fraction, the MAPQ
histogram in three bins (0, between, the cap), the mates with an alternative, and a check that hits, strand, pairs and totals of
the two calls are the same bytes.  The kernel itself: --profile NAME (pairs | pairq) makes exactly one such call after the index
is built, for `rocprofv3 --kernel-trace --stats` (se_pairq_kernel against se_pair_kernel), and prints nothing else."""
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
from rust_bio_amd.pipeline import (PairParams, PairQualityParams, SeedParams, attach_text, seed_extend_pairs_dev,  # noqa: E402
                                   seed_extend_pairs_mapq_dev)
from rust_bio_amd.suffix_array import bwt_dev, sample_dev, suffix_array_dev  # noqa: E402

N_ALPHABET = b"ACGTNacgtn"
ap = argparse.ArgumentParser()
ap.add_argument("genome", nargs="?", type=float, default=3e9)
ap.add_argument("pairs", nargs="?", type=float, default=6.25e5)
ap.add_argument("repeats", nargs="?", type=int, default=5)
ap.add_argument("--profile", default="")
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
qp = PairQualityParams(0, 60)
sc = Scoring.from_scores(-5, -1, 1, -1)
stride = 2 * L + 2 * prm.pad + 4
out = {}
for name in ("pairs", "pairq"):
    # (zeroed, not empty: the two calls' buffers are compared whole at the end, operation slots included)
    out[name] = {"hits": torch.zeros(n_reads * 96, dtype=torch.uint8, device=dev),
                 "ops": torch.zeros(n_reads * stride, dtype=torch.uint8, device=dev),
                 "strand": torch.zeros(n_reads, dtype=torch.uint8, device=dev),
                 "pairs": torch.zeros(n_pairs * 16, dtype=torch.uint8, device=dev), "tot": np.zeros(2, dtype=np.uint64)}
d_multi = torch.zeros(n_reads * 16, dtype=torch.uint8, device=dev)


def call(name):
    o = out[name]
    if name == "pairs":
        seed_extend_pairs_dev(fm, sc, n_pairs, reads.data_ptr(), d_roff.data_ptr(), L, o["hits"].data_ptr(), o["pairs"].data_ptr(),
                              o["strand"].data_ptr(), o["ops"].data_ptr(), stride, prm, pp, stream, o["tot"])
    else:
        seed_extend_pairs_mapq_dev(fm, sc, n_pairs, reads.data_ptr(), d_roff.data_ptr(), L, o["hits"].data_ptr(), o["pairs"].data_ptr(),
                                   d_multi.data_ptr(), o["strand"].data_ptr(), o["ops"].data_ptr(), stride, prm, pp, qp, stream, o["tot"])


names = list(out)
if args.profile:
    call(args.profile)
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
                   "(bench.py seed_extend leg's index and parameters), PairParams(0, 1000, 17), PairQualityParams(0, 60)",
       "index_build_s": round(t_index, 2), "repeats": repeats}
for name in names:
    med = float(np.median(ms[name]))
    res[name] = {"pairs_per_s": round(n_pairs / (med * 1e-3), 1), "ms_median": round(med, 3), "ms_min": round(min(ms[name]), 3),
                 "ms_all": [round(x, 3) for x in ms[name]], "seed_hits": int(out[name]["tot"][0]), "candidates": int(out[name]["tot"][1])}
res["pairq_over_pairs_ms"] = round(res["pairq"]["ms_median"] / res["pairs"]["ms_median"], 4)
proper = out["pairq"]["pairs"].view(n_pairs, 16)[:, 12] == 1
m = d_multi.view(n_reads, 16)
mapq = m[:, 9]
mapped = out["pairq"]["hits"].view(torch.int32).view(n_reads, 24)[:, 0] > MIN_SCORE
res["pairq"].update({"proper_frac": round(proper.float().mean().item(), 4), "mapped_frac": round(mapped.float().mean().item(), 4),
                     "mapq_0_frac": round((mapq == 0).float().mean().item(), 4),
                     "mapq_between_frac": round(((mapq > 0) & (mapq < qp.mapq_cap)).float().mean().item(), 4),
                     "mapq_cap_frac": round((mapq == qp.mapq_cap).float().mean().item(), 4),
                     "mates_with_an_alternative": int((m[:, 4:8].contiguous().view(torch.int32).view(-1) == 2).sum().item())})
same = {k: bool(torch.equal(out["pairs"][k], out["pairq"][k])) for k in ("hits", "strand", "pairs", "ops")}
same["totals"] = bool((out["pairs"]["tot"] == out["pairq"]["tot"]).all())
res["check"] = same
res["check_ok"] = all(same.values())
print(json.dumps(res))
sys.exit(0 if res["check_ok"] else 1)
