"""The tiered call against the strands call and the SMEM-seeded call, on 150-bp reads at three substitution rates:

    python tools/exp/time_seed_extend_tiered.py [genome_bp=50000000] [reads=200000] [repeats=3] [--out FILE]

One genome T, two device-built indexes: a forward index of T$ for bg_seed_extend_strands_batch_dev (SeedParams(20, 10, 16, 25),
BG_STRAND_BOTH) and an FMD index of T$R$ for bg_seed_extend_smem_batch_dev (SmemSeedParams(19, 16, 16, 25), BG_STRAND_BOTH) and
bg_seed_extend_tiered_batch_dev (the same two parameter sets as its tiers, reseed_below = 142: the score of a read with four
substitutions, so a read with five or more, or without a hit, is re-seeded);
both with a suffix array sampled at 32 and scoring (-5, -1, 1, -1).  Reads are windows of T with substitutions only, at rates
0, 2 and 7 %, a seeded half of them reverse-complemented.  After a warm-up, each call is timed with events, interleaved over
the repeats.  One JSON line (also written to --out): per rate and call reads/s (median), suffix-array rows, candidates, reads
re-seeded (tiered call), and the fraction of the reads mapped at their truth (ref_start == origin, on the strand they were drawn from)."""
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
from rust_bio_amd.pipeline import (SeedParams, SmemSeedParams, TieredSeedParams, attach_text, revcomp_dev,  # noqa: E402
                                   seed_extend_smem_dev, seed_extend_strands_dev, seed_extend_tiered_dev)
from rust_bio_amd.suffix_array import bwt_dev, sample_dev, suffix_array_dev  # noqa: E402

N_ALPHABET = b"ACGTNacgtn"
ap = argparse.ArgumentParser()
ap.add_argument("genome", nargs="?", type=float, default=5e7)
ap.add_argument("reads", nargs="?", type=float, default=2e5)
ap.add_argument("repeats", nargs="?", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()
n_genome, n_reads, repeats = int(args.genome), int(args.reads), args.repeats
L = 150
dev = torch.device("cuda:0")
ctx = _lib.Context(0)
stream = torch.cuda.current_stream().cuda_stream


def build_index(d_text):
    d_sa = suffix_array_dev(d_text, ctx=ctx)
    d_b = bwt_dev(d_text, d_sa, ctx=ctx)
    ssa = sample_dev(d_sa, d_b, ord("$"), 32, ctx=ctx)
    fm = FMIndex.from_device(d_b, 128, N_ALPHABET, ctx=ctx)
    fm._d_bwt = None
    del d_sa, d_b
    ssa.attach(fm)
    attach_text(fm, d_text=d_text)
    torch.cuda.synchronize()
    return fm


t0 = time.perf_counter()
g_dev = synth_gpu.genome(n_genome, seed=33, device=dev)  # T$
fm_fwd = build_index(g_dev)
t_fwd = time.perf_counter() - t0
t0 = time.perf_counter()
one = torch.tensor([0, n_genome], dtype=torch.int64, device=dev)
rc_t = torch.empty(n_genome, dtype=torch.uint8, device=dev)
revcomp_dev(1, g_dev.data_ptr(), one.data_ptr(), rc_t.data_ptr(), ctx=ctx, stream=stream)
fmd_text = torch.cat([g_dev, rc_t, g_dev[-1:]])  # T$R$
del rc_t
fm_fmd = build_index(fmd_text)
t_fmd = time.perf_counter() - t0

sc = Scoring.from_scores(-5, -1, 1, -1)
fixed, smem = SeedParams(20, 10, 16, 25), SmemSeedParams(19, 16, 16, 25)
RESEED_BELOW = L - 2 * 4  # a match scores 1, a mismatch -1: four substitutions
tiered = TieredSeedParams(fixed, smem, RESEED_BELOW)
stride = 2 * L + 2 * 25 + 4
d_roff = torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * L
rev = torch.from_numpy(np.random.default_rng(7).random(n_reads) < 0.5).to(dev)
bufs = {name: {"hits": torch.empty(n_reads * 96, dtype=torch.uint8, device=dev), "ops": torch.empty(n_reads * stride, dtype=torch.uint8, device=dev),
               "strand": torch.empty(n_reads, dtype=torch.uint8, device=dev), "tier": torch.empty(n_reads, dtype=torch.uint8, device=dev), "tot": np.zeros(3, dtype=np.uint64)}
        for name in ("strands", "smem", "tiered")}


def call(name, reads):
    o = bufs[name]
    if name == "strands":
        seed_extend_strands_dev(fm_fwd, sc, n_reads, reads.data_ptr(), d_roff.data_ptr(), L, o["hits"].data_ptr(), o["strand"].data_ptr(),
                                o["ops"].data_ptr(), stride, fixed, _lib.STRAND_BOTH, stream, o["tot"])
    else:
        try:
            if name == "smem":
                seed_extend_smem_dev(fm_fmd, sc, n_reads, reads.data_ptr(), d_roff.data_ptr(), L, o["hits"].data_ptr(), o["strand"].data_ptr(),
                                     o["ops"].data_ptr(), stride, smem, _lib.STRAND_BOTH, stream, o["tot"])
            else:
                seed_extend_tiered_dev(fm_fmd, sc, n_reads, reads.data_ptr(), d_roff.data_ptr(), L, o["hits"].data_ptr(),
                                       o["strand"].data_ptr(), o["tier"].data_ptr(), o["ops"].data_ptr(), stride, tiered, _lib.STRAND_BOTH,
                                       stream, o["tot"])
        except _lib.BiogpuError as e:  # a read with more than max_smems records: answered from the first ones
            if e.status != -9:
                raise
            o["truncated"] = True


res = {"workload": f"{n_reads} x {L} bp reads (substitutions only, half reverse-complemented) vs a {n_genome} bp genome",
       "index_build_s": {"forward": round(t_fwd, 2), "fmd": round(t_fmd, 2)}, "repeats": repeats,
       "fixed": "SeedParams(20, 10, 16, 25)", "smem": "SmemSeedParams(19, 16, 16, 25)", "reseed_below": RESEED_BELOW, "rates": {}}
for rate in (0.0, 0.02, 0.07):
    reads, starts = synth_gpu.reads_from_genome(g_dev, n_reads, L, seed=5, sub=rate, ins=0.0, dele=0.0)
    rc = torch.empty_like(reads)
    revcomp_dev(n_reads, reads.data_ptr(), d_roff.data_ptr(), rc.data_ptr(), ctx=ctx, stream=stream)
    half = torch.where(rev[:, None], rc.view(n_reads, L), reads.view(n_reads, L)).reshape(-1).contiguous()
    del rc, reads
    names = ["strands", "smem", "tiered"]
    for name in names:  # warm-up: code objects, scratch
        call(name, half)
    torch.cuda.synchronize()
    ms = {n: [] for n in names}
    for rep in range(repeats):
        for name in names[rep % 3:] + names[:rep % 3]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(name, half)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    row = {}
    for name in names:
        o = bufs[name]
        med = float(np.median(ms[name]))
        ref_start = o["hits"].view(n_reads, 96)[:, 72:80].contiguous().view(torch.int64).view(-1)
        truth = (ref_start == starts) & (o["strand"] == rev.to(torch.uint8))
        row[name] = {"reads_per_s": round(n_reads / (med * 1e-3), 1), "ms_median": round(med, 3), "ms_all": [round(x, 3) for x in ms[name]],
                     "seed_hits": int(o["tot"][0]), "candidates": int(o["tot"][1]),
                     "mapped_frac": round((o["strand"] != 255).float().mean().item(), 4),
                     "mapped_at_truth_frac": round(truth.float().mean().item(), 4), "truncated": bool(o.get("truncated", False))}
    row["tiered"]["reseeded"] = int(bufs["tiered"]["tot"][2])
    row["tiered"]["answered_by_tier_2"] = int((bufs["tiered"]["tier"] == _lib.TIER_SECOND).sum().item())
    row["smem_over_strands_time"] = round(row["smem"]["ms_median"] / row["strands"]["ms_median"], 3)
    row["tiered_over_strands_time"] = round(row["tiered"]["ms_median"] / row["strands"]["ms_median"], 3)
    res["rates"][str(rate)] = row
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
