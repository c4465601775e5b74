"""The rescue-mapq call (mate rescue plus a mapping quality per mate) against the rescue call, device-resident, 150 bp mates:

    python tools/exp/time_seed_extend_rescueq.py [genome_bp=3000000000] [pairs=625000] [repeats=5] [--broken 0.05] [--profile NAME]

Genome, device-built index, SeedParams(20, 10, 16, 25) and scoring (-5, -1, 1, -1) are those of tools/exp/time_seed_extend_multi.py
(bench.py's seed_extend leg); the pairs are synth_gpu.read_pairs_from_genome's.  Two workloads:
    clean    the pairs as generated, sub = 1 %, no indels (nearly all proper from their seeds): what the rescue call costs when there
             is nothing to do
    broken   the same, and in a fraction --broken of the pairs mate 2 carries a substitution every 15 bases from base 7 (no 20-base
             seed survives): what rescue costs and yields
After a warm-up, on each workload the rescue call and the rescue-mapq call (max_anchors = 2, min_score = 75; PairQualityParams(0, 60))
are timed with events in one process, interleaved over the repeats (the order alternates).  One JSON line: pairs/s of each (median),
the ratio, rescue alignments run, pairs rescued, whether the two calls' hits, strand, pairs and rescued bytes are equal, and the
MAPQ histogram (0, between, cap) of the mates of rescued pairs.  --profile NAME (rescue | rescueq) makes exactly one such call on
the chosen workload (--load clean | broken) after the index is built, for `rocprofv3 --kernel-trace --stats`, and prints nothing
else."""
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
from rust_bio_amd.pairwise import Scoring  # noqa: E402
from rust_bio_amd.pipeline import (PairParams, PairQualityParams, RescueParams, SeedParams, attach_text,  # noqa: E402
                                   seed_extend_pairs_rescue_dev, seed_extend_pairs_rescue_mapq_dev)
from rust_bio_amd.suffix_array import bwt_dev, sample_dev, suffix_array_dev  # noqa: E402

N_ALPHABET = b"ACGTNacgtn"
ap = argparse.ArgumentParser()
ap.add_argument("genome", nargs="?", type=float, default=3e9)
ap.add_argument("pairs", nargs="?", type=float, default=625e3)
ap.add_argument("repeats", nargs="?", type=int, default=5)
ap.add_argument("--broken", type=float, default=0.05)
ap.add_argument("--profile", default="")
ap.add_argument("--load", default="broken")
args = ap.parse_args()
n_genome, n_pairs, repeats = int(args.genome), int(args.pairs), args.repeats
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

clean, _, _ = synth_gpu.read_pairs_from_genome(g_dev, n_pairs, L, seed=5, sub=0.01, ins=0.0, dele=0.0)
clean = clean.view(2 * n_pairs, L)
broken = clean.clone()
hit = torch.from_numpy(np.random.default_rng(7).random(n_pairs) < args.broken).to(dev)
rows = 2 * torch.nonzero(hit).view(-1) + 1  # mate 2 of the chosen pairs
cols = torch.arange(7, L, 15, device=dev)
old = broken[rows][:, cols]
lut = torch.arange(256, dtype=torch.uint8, device=dev)
for a, b in zip(b"ACGT", b"CGTA"):
    lut[a] = b
sub = broken[rows]
sub[:, cols] = lut[old.long()]
broken[rows] = sub
READS = {"clean": clean.reshape(-1).contiguous(), "broken": broken.reshape(-1).contiguous()}
d_roff = torch.arange(2 * n_pairs + 1, dtype=torch.int64, device=dev) * L

prm, pp, rp, qp = SeedParams(20, 10, 16, 25), PairParams(0, 1000, 17), RescueParams(2, 75), PairQualityParams(0, 60)
sc = Scoring.from_scores(-5, -1, 1, -1)
stride = L + max(L + 2 * prm.pad, pp.max_span) + 4
o = {"hits": torch.empty(2 * n_pairs * 96, dtype=torch.uint8, device=dev), "ops": torch.empty(2 * n_pairs * stride, dtype=torch.uint8, device=dev),
     "strand": torch.empty(2 * n_pairs, dtype=torch.uint8, device=dev), "pairs": torch.empty(n_pairs * 16, dtype=torch.uint8, device=dev),
     "rescued": torch.empty(n_pairs, dtype=torch.uint8, device=dev), "multi": torch.empty(2 * n_pairs * 16, dtype=torch.uint8, device=dev)}
tot = {}


def call(name, load):
    reads = READS[load]
    t = tot.setdefault((name, load), np.zeros(4, dtype=np.uint64))
    if name == "rescue":
        seed_extend_pairs_rescue_dev(fm, sc, n_pairs, reads.data_ptr(), d_roff.data_ptr(), L, o["hits"].data_ptr(), o["pairs"].data_ptr(),
                                     o["rescued"].data_ptr(), o["strand"].data_ptr(), o["ops"].data_ptr(), stride, prm, pp, rp, stream, t)
    else:
        seed_extend_pairs_rescue_mapq_dev(fm, sc, n_pairs, reads.data_ptr(), d_roff.data_ptr(), L, o["hits"].data_ptr(),
                                          o["pairs"].data_ptr(), o["rescued"].data_ptr(), o["multi"].data_ptr(), o["strand"].data_ptr(),
                                          o["ops"].data_ptr(), stride, prm, pp, rp, qp, stream, t)


if args.profile:
    call(args.profile, args.load)
    torch.cuda.synchronize()
    sys.exit(0)
res = {"workload": f"{n_pairs} pairs of {L} bp mates vs a {n_genome} bp genome; broken: mate 2 of {args.broken:.0%} of the pairs without a seed",
       "index_build_s": round(t_index, 2), "repeats": repeats}
names = ["rescue", "rescueq"]
for load in READS:
    for name in names:  # warm-up: code objects, scratch
        call(name, load)
        call(name, load)
    torch.cuda.synchronize()
    ms = {n: [] for n in names}
    kept = {}
    for rep in range(repeats):
        for name in names if rep % 2 == 0 else names[::-1]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(name, load)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
            if rep == repeats - 1:
                kept[name] = [o[k].clone() for k in ("hits", "strand", "pairs", "rescued")]
    r = {}
    for name in names:
        med = float(np.median(ms[name]))
        r[name] = {"pairs_per_s": round(n_pairs / (med * 1e-3), 1), "ms_median": round(med, 3), "ms_all": [round(x, 3) for x in ms[name]]}
    t = tot[("rescueq", load)]
    in_rescued = (kept["rescueq"][3] != 0).repeat_interleave(2)
    mapq = o["multi"].view(2 * n_pairs, 16)[:, 9][in_rescued]
    r["rescueq"].update({"rescue_alignments": int(t[2]), "pairs_rescued": int(t[3]),
                         "same_outputs_as_the_rescue_call": all(torch.equal(a, b) for a, b in zip(kept["rescue"], kept["rescueq"])),
                         "mapq_of_rescued_pairs": {"0": int((mapq == 0).sum()), "between": int(((mapq > 0) & (mapq < qp.mapq_cap)).sum()),
                                                   "cap": int((mapq == qp.mapq_cap).sum())}})
    r["rescueq_over_rescue_rate"] = round(r["rescueq"]["pairs_per_s"] / r["rescue"]["pairs_per_s"], 4)
    res[load] = r
print(json.dumps(res))
