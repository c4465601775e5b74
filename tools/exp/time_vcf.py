"""Device-resident timing of the VCF writer (bg_vcf_emit_dev), in one process (python tools/exp/time_vcf.py [SITES] [EVENTS]
[GENOME_BP] [REPEATS] [OUT]), on inputs made here with numpy — no mapping and no FASTQ: a reference text of GENOME_BP (default
30 000 000) upper-case bases in one contig, SITES (default 2 750 000) SNV sites and EVENTS (default 600 000) indel events at
sorted drawn positions of one region, the counts DESIGN.md 4.18 / 4.19 report for the wide region.  Two mixes:
  * short: deletions and insertions of 1 .. 3 bases, half and half;
  * long:  the same sites and insertions, deletions of 1 .. 10 000 bases.
Each call once per round between two device events; after 2 warm-up rounds REPEATS (default 9) rounds, medians with the rounds'
min and max: the sizing call, the full call, and a device-to-device copy of the bytes the full call wrote, in the same run.
Checked: the first lines of each mix's output, those of the 10 000 elements with the smallest positions, are what
tests/vcf_oracle.py gives for these elements."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from csrc_hash import csrc_sha  # noqa: E402
torch.cuda.init()
import vcf_oracle as vo  # noqa: E402
from rust_bio_amd import _lib, sam, vcf  # noqa: E402

N_SITES = int(float(sys.argv[1])) if len(sys.argv) > 1 else 2_750_000
N_EVENTS = int(float(sys.argv[2])) if len(sys.argv) > 2 else 600_000
N_GENOME = int(float(sys.argv[3])) if len(sys.argv) > 3 else 30_000_000
REPEATS = int(sys.argv[4]) if len(sys.argv) > 4 else 9
SAMPLE = 10_000
dev = torch.device("cuda:0")
ctx = _lib.Context(0)
stream = torch.cuda.current_stream().cuda_stream
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


# ---- the inputs
rng = np.random.default_rng(41)
text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, N_GENOME + 1)]
text[N_GENOME] = ord("$")
contigs = sam.Contigs([("chr1", 0, N_GENOME)])
entries = [(b"chr1", 0, N_GENOME)]
sites = np.zeros(N_SITES, dtype=_lib.BAM_SITE_DTYPE)
sites["pos"] = np.sort(rng.integers(0, N_GENOME, N_SITES)).astype(np.int32)
sites["ref_base"] = text[sites["pos"]]
sites["alt"] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), sites["ref_base"])]
sites["depth"] = rng.integers(20, 60, N_SITES)
sites["alt_fwd"], sites["alt_rev"] = rng.integers(1, 10, N_SITES), rng.integers(1, 10, N_SITES)
sites["ref_count"] = sites["depth"] - sites["alt_fwd"] - sites["alt_rev"]


def events_of(max_del):
    ev = np.zeros(N_EVENTS, dtype=_lib.BAM_INDEL_DTYPE)
    ev["pos"] = np.sort(rng.integers(0, N_GENOME - max_del - 1, N_EVENTS)).astype(np.int32)
    ev["kind"] = 1 + (np.arange(N_EVENTS) & 1)
    ev["len"] = np.where(ev["kind"] == 1, rng.integers(1, max_del + 1, N_EVENTS), rng.integers(1, 4, N_EVENTS))
    # an anchor's deletions in front of its insertions, as bg_bam_indels returns them
    order = np.lexsort((ev["kind"], ev["pos"]))
    ev = ev[order]
    ev["depth"] = rng.integers(20, 60, N_EVENTS)
    ev["alt_fwd"], ev["alt_rev"] = rng.integers(1, 10, N_EVENTS), rng.integers(1, 10, N_EVENTS)
    ins = np.where(ev["kind"] == 2, ev["len"], 0).astype(np.uint64)
    ev["seq_off"] = np.cumsum(ins) - ins
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(ins.sum()))]
    return ev, seq


def up(a):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).to(dev)


d_text, d_sites, d_contigs, d_names = up(text), up(sites), up(contigs.table), up(contigs.names)
MIXES = {}
for name, max_del in (("short", 3), ("long", 10_000)):
    ev, seq = events_of(max_del)
    m = dict(ev=ev, seq=seq, d_ev=up(ev), d_seq=up(seq))
    m["lists"] = (N_SITES, d_sites.data_ptr(), N_EVENTS, m["d_ev"].data_ptr(), m["d_seq"].data_ptr(), len(seq), d_contigs.data_ptr(), 1, d_names.data_ptr(),
                  d_text.data_ptr(), N_GENOME + 1)
    m["n_lines"], m["bytes"] = vcf.emit_dev(*m["lists"], stream=stream, ctx=ctx)
    m["d_out"] = torch.zeros(m["bytes"], dtype=torch.uint8, device=dev)
    m["d_copy"] = torch.zeros(m["bytes"], dtype=torch.uint8, device=dev)
    m["d_line_off"] = torch.zeros(m["n_lines"] + 1, dtype=torch.int64, device=dev)
    MIXES[name] = m


def sizing(m):
    assert vcf.emit_dev(*m["lists"], stream=stream, ctx=ctx) == (m["n_lines"], m["bytes"])


def full(m):
    assert vcf.emit_dev(*m["lists"], m["d_out"].data_ptr(), m["bytes"], m["d_line_off"].data_ptr(), stream=stream, ctx=ctx) == (m["n_lines"], m["bytes"])


CALLS = []
for name, m in MIXES.items():
    what = "%s mix (%d lines, %d bytes)" % (name, m["n_lines"], m["bytes"])
    CALLS += [("size_" + name, "bg_vcf_emit_dev, the sizing call: " + what, lambda m=m: sizing(m)),
              ("full_" + name, "bg_vcf_emit_dev, text and line offsets: " + what, lambda m=m: full(m)),
              ("copy_" + name, "a device-to-device copy of the bytes of the " + what, lambda m=m: m["d_copy"].copy_(m["d_out"]))]
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
say("%s: %d SNV sites and %d events (half deletions, half insertions of 1 .. 3 bases; deletions of 1 .. 3 bases in the short mix, of 1 .. 10 000 in the long) on one contig of %d bp" % (
    os.path.basename(_lib.SO_PATH), N_SITES, N_EVENTS, N_GENOME))
for key, name, _ in CALLS:
    t = sorted(ms[key])
    med[key] = t[len(t) // 2]
    say("%-125s median %8.3f ms (min %.3f max %.3f)" % (name, med[key], t[0], t[-1]))
for name, m in MIXES.items():
    size, whole, copy = med["size_" + name], med["full_" + name], med["copy_" + name]
    say("%s: the sizing call %.3f ms, the full call %.3f ms (the write pass and the offsets' copy %.3f ms); %d bytes = %.1f GB/s of output over the full call, "
        "%.1f GB/s over the write pass; the copy of these bytes %.3f ms: the full call is %.1f x the copy, the write pass %.1f x" % (
            name, size, whole, whole - size, m["bytes"], m["bytes"] / whole / 1e6, m["bytes"] / (whole - size) / 1e6, copy, whole / copy, (whole - size) / copy))
say("on record for comparison: bg_sam_sort_dev's permuted copy 1.8 x a copy; the SAM writer 439 MB in 10.3 ms = 42.6 GB/s")
# ---- checks: the lines of the SAMPLE elements with the smallest positions, out of the full call's output
for name, m in MIXES.items():
    full(m)
    torch.cuda.synchronize()
    ev = m["ev"]
    k = SAMPLE * N_SITES // (N_SITES + N_EVENTS)
    cut = int(sites["pos"][k])  # every element in front of this position
    ns, ne = int(np.searchsorted(sites["pos"], cut)), int(np.searchsorted(ev["pos"], cut))
    n_seq = int(ev["seq_off"][ne]) if ne < N_EVENTS else len(m["seq"])
    want, want_off = vo.emit(sites[:ns], ev[:ne], m["seq"][:n_seq].tobytes(), entries, text[:N_GENOME + 1].tobytes())
    got = m["d_out"][:len(want)].cpu().numpy().tobytes()
    got_off = m["d_line_off"][:ns + ne + 1].cpu().numpy().tolist()
    assert got == want and got_off == want_off, name
    say("checked, %s: the first %d lines (%d sites, %d events, %d bytes) and their offsets are tests/vcf_oracle.py's" % (name, ns + ne, ns, ne, len(want)))
say("not measured: the host-buffer flavour, counters of any kernel")
say("source hash (tools/csrc_hash.py): %s" % csrc_sha())
if len(sys.argv) > 5:
    open(sys.argv[5], "w").write("tools/exp/time_vcf.py %d %d %d %d on one MI355X, device-resident: every call once per round between two device events, "
                                 "%d rounds after 2 warm-up rounds, medians\n" % (N_SITES, N_EVENTS, N_GENOME, REPEATS, REPEATS) + "\n".join(lines) + "\n")
