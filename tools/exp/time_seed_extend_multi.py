"""The multi call (runner-up loci + MAPQ) against the strands call, on bench.py's seed_extend workload:

    python tools/exp/time_seed_extend_multi.py [genome_bp=3000000000] [reads=1250000] [repeats=5] [--chunk N] [--profile K]

Genome, device-built index, SeedParams(20, 10, 16, 25), scoring (-5, -1, 1, -1) and reads are those of
tools/exp/time_seed_extend_strands.py (bench.py's seed_extend leg); a seeded half of the reads is reverse-complemented.  After
a warm-up, three calls are timed with events in one process, interleaved over the repeats (the order alternates):
    strands     bg_seed_extend_strands_batch_dev, strands = 3
    multi_k1    bg_seed_extend_multi_batch_dev, strands = 3, K = 1, min_score = INT32_MIN, mapq_cap = 60
    multi_k4    the same with K = 4
One JSON line: reads/s of each call (median over the repeats), the two ratios against the strands call, the fractions of the
reads with mapq == 0 and with mapq == mapq_cap, the n_loci histogram, and a check that slot 0 of both multi calls is the strands
call's hit (record, window, strand, operations).  --profile K makes exactly one multi call with that K after the index is
built, for `rocprofv3 --kernel-trace --stats`, and prints nothing else."""
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
from rust_bio_amd.pipeline import (MultiParams, SeedParams, attach_text, revcomp_dev, seed_extend_multi_dev,  # noqa: E402
                                   seed_extend_strands_dev)
from rust_bio_amd.suffix_array import bwt_dev, sample_dev, suffix_array_dev  # noqa: E402

N_ALPHABET = b"ACGTNacgtn"
ap = argparse.ArgumentParser()
ap.add_argument("genome", nargs="?", type=float, default=3e9)
ap.add_argument("reads", nargs="?", type=float, default=1.25e6)
ap.add_argument("repeats", nargs="?", type=int, default=5)
ap.add_argument("--chunk", type=int, default=0)
ap.add_argument("--profile", type=int, default=0)
args = ap.parse_args()
n_genome, n_reads, repeats = int(args.genome), int(args.reads), args.repeats
L, CAP = 150, 60
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
del rc, reads

prm = SeedParams(20, 10, 16, 25)
sc = Scoring.from_scores(-5, -1, 1, -1)
stride = 2 * L + 2 * prm.pad + 4
KS = {"strands": 1, "multi_k1": 1, "multi_k4": 4}
if args.profile:
    KS = {"profile": args.profile}
out = {}
for name, K in KS.items():
    out[name] = {"hits": torch.empty(n_reads * K * 96, dtype=torch.uint8, device=dev),
                 "ops": torch.empty(n_reads * K * stride, dtype=torch.uint8, device=dev),
                 "strand": torch.empty(n_reads * K, dtype=torch.uint8, device=dev),
                 "multi": torch.empty(n_reads * 16, dtype=torch.uint8, device=dev), "tot": np.zeros(2, dtype=np.uint64)}


def call(name):
    o = out[name]
    if name == "strands":
        seed_extend_strands_dev(fm, sc, n_reads, half.data_ptr(), d_roff.data_ptr(), L, o["hits"].data_ptr(), o["strand"].data_ptr(),
                                o["ops"].data_ptr(), stride, prm, _lib.STRAND_BOTH, stream, o["tot"])
    else:
        seed_extend_multi_dev(fm, sc, n_reads, half.data_ptr(), d_roff.data_ptr(), L, o["hits"].data_ptr(), o["multi"].data_ptr(),
                              o["strand"].data_ptr(), o["ops"].data_ptr(), stride, prm, MultiParams(KS[name], -2**31, CAP),
                              _lib.STRAND_BOTH, stream, o["tot"])


names = list(out)
ctx.set_option("seed_chunk_reads", args.chunk)
if args.profile:
    call("profile")
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

res = {"workload": f"{n_reads} x {L} bp reads, half of them reverse-complemented, vs a {n_genome} bp genome (bench.py seed_extend leg)",
       "index_build_s": round(t_index, 2), "repeats": repeats, "seed_chunk_reads": args.chunk}
for name in names:
    med = float(np.median(ms[name]))
    res[name] = {"reads_per_s": round(n_reads / (med * 1e-3), 1), "ms_median": round(med, 3), "ms_min": round(min(ms[name]), 3),
                 "ms_all": [round(x, 3) for x in ms[name]], "seed_hits": int(out[name]["tot"][0]), "candidates": int(out[name]["tot"][1])}
for name in ("multi_k1", "multi_k4"):
    res[name + "_over_strands_time"] = round(res[name]["ms_median"] / res["strands"]["ms_median"], 4)
    m = out[name]["multi"].view(n_reads, 16)
    mapq, n_loci = m[:, 9], m[:, 4:8].contiguous().view(torch.int32).view(-1)
    res[name].update({"mapq_0_frac": round((mapq == 0).float().mean().item(), 4), "mapq_cap_frac": round((mapq == CAP).float().mean().item(), 4),
                      "n_loci_hist": torch.bincount(n_loci, minlength=5).tolist()})
# slot 0 of the multi calls against the strands call: the whole hit record, strand, operations
s = out["strands"]
hs = s["hits"].view(n_reads, 96)
n_ops = hs.view(torch.int32)[:, 7].to(torch.int64)
tail = torch.arange(stride, device=dev)[None, :] >= (stride - n_ops)[:, None]
ok = True
for name in ("multi_k1", "multi_k4"):
    K = KS[name]
    hm = out[name]["hits"].view(n_reads, K, 96)[:, 0]
    same = (hs[:, :32] == hm[:, :32]).all(dim=1) & (hs[:, 40:] == hm[:, 40:]).all(dim=1)  # all but ops_off, which goes with the slot
    same &= s["strand"] == out[name]["strand"].view(n_reads, K)[:, 0]
    om = out[name]["ops"].view(n_reads, K, stride)[:, 0]
    same &= ((s["ops"].view(n_reads, stride) == om) | ~tail).all(dim=1)
    res[name]["slot0_differing"] = int((~same).sum().item())
    ok = ok and res[name]["slot0_differing"] == 0
res["check_ok"] = ok
print(json.dumps(res))
sys.exit(0 if ok else 1)
