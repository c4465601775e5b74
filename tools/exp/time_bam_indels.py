"""Device-resident timing of the indel events (bg_bam_indels_dev), in one process (python tools/exp/time_bam_indels.py [PAIRS]
[GENOME_BP] [REPEATS] [OUT]), on the batch and the regions of tools/exp/time_bam_sites.py (the set-up below is that tool's): the
coordinate-sorted, duplicate-flagged BAM records of PAIRS (default 500 000) pairs of 150 bp on a genome of three contigs; the
reads carry one inserted and one deleted base in a hundred, so the batch has raw events by the hundred thousand.  Regions:
  * wide: ONE region, the first SPAN (default 30 000 000, at most chr1) positions of chr1;
  * targets: 20 000 regions of 300 positions, evenly spread over the three contigs;
  * genome: every contig whole.
Each call once per round between two device events; after 2 warm-up rounds REPEATS (default 9) rounds, medians with the rounds'
min and max.  The yardstick, in the same process on the same regions: bg_bam_sites_dev with the strict thresholds.  The passes
are told apart by differences of whole calls: the ctx option indels_stop_after ends the call behind the count pass, the emit
pass or the sort.  bg_bam_pileup_dev and bg_bam_sites_dev are timed again and held to the spreads recorded in
profiles/bam_pileup_timing.txt and profiles/bam_sites_timing.txt.
Checked: the events and sequences of the wide region are those of the same span cut into 1 000 regions, the region index aside;
the events of a 1 Mbp sample are what tests/bam_indels_oracle.py gives on the sample's records, with the depth from the
16-column pileup's rows."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from csrc_hash import csrc_sha  # noqa: E402
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


# ---- the batch of time_bam_read.py: genome, index, reads with planted duplicates, parsed FASTQ, hits, sorted BAM records
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
print("set-up: the index stands", flush=True)
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
print("set-up: the reads are mapped", flush=True)
d_contigs = torch.from_numpy(contigs.table.view(np.uint8).copy()).to(dev)
d_names = torch.from_numpy(contigs.names).to(dev)
sp, mp = sam.SamParams(FLAGS, 1), sam.MarkdupParams(sam.SAM_PAIRED, 1, 33, 15)
d_dup = torch.zeros(N, dtype=torch.uint8, device=dev)
d_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
d_key = torch.zeros(N, dtype=torch.int64, device=dev)
d_perm = torch.zeros(N, dtype=torch.int64, device=dev)
d_sorted_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
emit_args = (fm, sp, N, d_contigs.data_ptr(), 3, d_names.data_ptr(), d_fq.data_ptr(), d_recs.data_ptr(), d_seq.data_ptr(), d_qual.data_ptr(),
             d_hits.data_ptr(), d_strand.data_ptr(), d_ops.data_ptr())
emit_kw = dict(d_multi=d_multi.data_ptr(), d_pairs=d_pairs.data_ptr(), d_dup=d_dup.data_ptr(), stream=stream)
sam.markdup_dev(mp, N, d_contigs.data_ptr(), 3, d_hits.data_ptr(), d_strand.data_ptr(), d_recs.data_ptr(), d_qual.data_ptr(), d_dup.data_ptr(),
                stream=stream, ctx=ctx)
sam.sort_keys_dev(sp, N, d_contigs.data_ptr(), 3, d_hits.data_ptr(), d_strand.data_ptr(), d_key.data_ptr(), stream=stream, ctx=ctx)
bam_total = bam.emit_dev(*emit_args, 0, 0, d_off.data_ptr(), **emit_kw)
d_bam = torch.zeros(bam_total, dtype=torch.uint8, device=dev)
d_bam_sorted = torch.zeros(bam_total, dtype=torch.uint8, device=dev)
bam.emit_dev(*emit_args, d_bam.data_ptr(), bam_total, d_off.data_ptr(), **emit_kw)
sam.sort_dev(N, d_key.data_ptr(), d_bam.data_ptr(), d_off.data_ptr(), bam_total, d_bam_sorted.data_ptr(), bam_total, d_sorted_off.data_ptr(),
             d_perm.data_ptr(), stream=stream, ctx=ctx)
del d_bam
print("set-up: the records are sorted", flush=True)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests"))
import bam_indels_oracle as io  # noqa: E402

# ---- the regions
len1 = int(contigs.table["len"][0])
SPAN = min(int(float(os.environ.get("BG_PILEUP_SPAN", 30_000_000))), len1)
SAMPLE = min(1_000_000, SPAN)
N_TARGETS, TARGET = 20_000, 300
targets = []
for c in range(3):
    ln = int(contigs.table["len"][c])
    k = N_TARGETS // 3 + (c < N_TARGETS % 3)
    targets += [(c, int(b), int(b) + TARGET) for b in np.linspace(0, ln - TARGET, k).astype(np.int64)]
REGIONS = {"wide": [(0, 0, SPAN)], "pieces": [(0, SPAN * k // 1000, SPAN * (k + 1) // 1000) for k in range(1000)], "targets": targets,
           "genome": [(c, 0, int(contigs.table["len"][c])) for c in range(3)], "sample": [(0, SPAN - SAMPLE, SPAN)]}
d_regions = {name: torch.from_numpy(bam.pileup_regions(r).view(np.uint8).copy()).to(dev) for name, r in REGIONS.items()}
n_rows = {name: sum(e - b for _, b, e in r) for name, r in REGIONS.items()}
assert SPAN * 64 <= 2_000_000_000
d_rows = torch.zeros(SPAN * 16, dtype=torch.int32, device=dev)
STRICT = dict(min_depth=2, min_alt=2, min_alt_permille=200)  # a caller's thresholds, those of time_bam_sites.py
LAX = dict()                                                 # every event
KW = {"strict": STRICT, "lax": LAX}
head = (N, d_bam_sorted.data_ptr(), d_sorted_off.data_ptr(), d_contigs.data_ptr(), 3)


def pileup(name, w, out=True):
    got = bam.pileup_dev(*head, d_regions[name].data_ptr(), len(REGIONS[name]), d_rows.data_ptr() if out else 0, n_rows[name] if out else 0, 0,
                         flags=bam.PILEUP_STRANDS if w == 16 else 0, stream=stream, ctx=ctx)
    assert got == n_rows[name]


def sites(name, d_sites=0, cap=0, d_site_off=0, d_summary=0):
    return bam.sites_dev(*head, g_dev.data_ptr(), N_GENOME, d_regions[name].data_ptr(), len(REGIONS[name]), d_sites, cap, d_site_off, d_summary,
                         stream=stream, ctx=ctx, **STRICT)


def indels(name, tag, d_events=0, cap=0, d_seq=0, seq_cap=0, d_event_off=0):
    return bam.indels_dev(*head, d_regions[name].data_ptr(), len(REGIONS[name]), d_events, cap, d_seq, seq_cap, d_event_off, stream=stream, ctx=ctx, **KW[tag])


def staged(name, stop):
    """the lax sizing call ended behind pass `stop`"""
    ctx.set_option("indels_stop_after", stop)
    try:
        assert indels(name, "lax") == (0, 0)
    finally:
        ctx.set_option("indels_stop_after", 0)


n_sites = {name: sites(name) for name in ("wide", "targets", "genome")}
d_sites = torch.zeros(max(n_sites.values()) * 32, dtype=torch.uint8, device=dev)
d_site_off = torch.zeros(N_TARGETS + 1, dtype=torch.int64, device=dev)
d_summary = torch.zeros(N_TARGETS * 48, dtype=torch.uint8, device=dev)
totals = {(name, tag): indels(name, tag) for name in REGIONS for tag in KW}
d_events = torch.zeros(max(t[0] for t in totals.values()) * 40 + 8, dtype=torch.uint8, device=dev)
d_iseq = torch.zeros(max(t[1] for t in totals.values()) + 1, dtype=torch.uint8, device=dev)
d_event_off = torch.zeros(N_TARGETS + 1, dtype=torch.int64, device=dev)


def full_sites(name):
    assert sites(name, d_sites.data_ptr(), n_sites[name], d_site_off.data_ptr(), d_summary.data_ptr()) == n_sites[name]


def full(name, tag):
    n, n_seq = totals[(name, tag)]
    assert indels(name, tag, d_events.data_ptr(), n, d_iseq.data_ptr(), n_seq, d_event_off.data_ptr()) == (n, n_seq)


CALLS = [
    ("wide8", "bg_bam_pileup_dev, one region of %d positions of chr1, 8 columns" % SPAN, lambda: pileup("wide", 8)),
    ("wide16", "bg_bam_pileup_dev, one region of %d positions of chr1, 16 columns" % SPAN, lambda: pileup("wide", 16)),
    ("targets8", "bg_bam_pileup_dev, %d regions of %d positions over the three contigs, 8 columns" % (len(targets), TARGET), lambda: pileup("targets", 8)),
    ("targets16", "bg_bam_pileup_dev, %d regions of %d positions, 16 columns" % (len(targets), TARGET), lambda: pileup("targets", 16)),
    ("sizing", "bg_bam_pileup_dev, the sizing call of the wide region (the front alone)", lambda: pileup("wide", 8, out=False)),
    ("sizing_targets", "bg_bam_pileup_dev, the sizing call of the targets (the front alone)", lambda: pileup("targets", 8, out=False)),
    ("sizing_genome", "bg_bam_pileup_dev, the sizing call of the whole contigs (the front alone)", lambda: pileup("genome", 8, out=False)),
]
for name in ("wide", "targets", "genome"):
    CALLS.append(("sites_size_%s" % name, "bg_bam_sites_dev, the sizing call: %s, strict thresholds (%d sites)" % (name, n_sites[name]), lambda name=name: sites(name)))
    CALLS.append(("sites_%s" % name, "bg_bam_sites_dev, sites, offsets and summaries: %s, strict thresholds (%d sites) (the yardstick)" % (name, n_sites[name]),
                  lambda name=name: full_sites(name)))
    for stop, what in ((1, "the count pass"), (2, "the emit pass"), (3, "the sort")):
        CALLS.append(("stop%d_%s" % (stop, name), "bg_bam_indels_dev, %s, ended behind %s (indels_stop_after = %d)" % (name, what, stop),
                      lambda name=name, stop=stop: staged(name, stop)))
    for tag in ("lax", "strict"):
        what = "%s, %s thresholds (%d events, %d sequence bytes)" % ((name, tag) + totals[(name, tag)])
        CALLS.append(("size_%s_%s" % (name, tag), "bg_bam_indels_dev, the sizing call: " + what, lambda name=name, tag=tag: indels(name, tag)))
        CALLS.append(("full_%s_%s" % (name, tag), "bg_bam_indels_dev, events, sequences and offsets: " + what, lambda name=name, tag=tag: full(name, tag)))
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
say("%s: %d pairs = %d reads of %d bp on a genome of %d bp in 3 contigs; %.1f MB of sorted records in %d slots; tile %d" % (
    os.path.basename(_lib.SO_PATH), N_PAIRS, N, L, N_GENOME, bam_total / 1e6, N, bam.PILEUP_TILE))
say("regions: wide = chr1:0-%d; targets = %d x %d positions; genome = the three contigs whole, %d positions; strict = %r, lax = min_alt 1 alone" % (
    SPAN, len(targets), TARGET, n_rows["genome"], STRICT))
for key, name, _ in CALLS:
    t = sorted(ms[key])
    med[key] = t[len(t) // 2]
    say("%-135s median %8.3f ms (min %.3f max %.3f)" % (name, med[key], t[0], t[-1]))
# ---- the raw events: what the lax call keeps counts every record of every event once
for name in ("wide", "targets", "genome"):
    full(name, "lax")
    torch.cuda.synchronize()
    ev = d_events[:40 * totals[(name, "lax")][0]].cpu().numpy().view(_lib.BAM_INDEL_DTYPE)
    n_raw = int(ev["alt_fwd"].sum(dtype=np.uint64) + ev["alt_rev"].sum(dtype=np.uint64))
    front = med[{"wide": "sizing", "targets": "sizing_targets", "genome": "sizing_genome"}[name]]
    s1, s2, s3, size = med["stop1_" + name], med["stop2_" + name], med["stop3_" + name], med["size_%s_lax" % name]
    whole, yard = med["full_%s_lax" % name], med["sites_" + name]
    say("%s: %d raw events in %d events (%d DEL, %d INS, longest insertion %d), %d events under the strict thresholds" % (
        name, n_raw, len(ev), int((ev["kind"] == 1).sum()), int((ev["kind"] == 2).sum()), int(ev["len"][ev["kind"] == 2].max(initial=0)),
        totals[(name, "strict")][0]))
    say("%s, lax: the front %.3f ms, the count pass with its scan and read-back %.3f ms, the emit pass %.3f ms, the sort %.3f ms (%.0f %% of the sizing call), "
        "heads, runs, verdicts, four scans and the third read-back %.3f ms, records and sequences out %.3f ms; the full call %.3f ms = %.2f x the yardstick, "
        "the strict one %.3f ms = %.2f x; the sites' count pass takes %.3f ms" % (
            name, front, s1 - front, s2 - s1, s3 - s2, 100 * (s3 - s2) / size, size - s3, whole - size, whole, whole / yard, med["full_%s_strict" % name],
            med["full_%s_strict" % name] / yard, med["sites_size_" + name] - front))
# ---- the pileup's and the sites' figures against the spreads on record
import re  # noqa: E402
prof = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "profiles")
if N_PAIRS == 500_000 and N_GENOME == 100_000_000 and SPAN == 30_000_000:
    held = [("bam_pileup_timing.txt", "bg_bam_pileup_dev", {"wide8": "8 columns  ", "wide16": "16 columns (BG_PILEUP_STRANDS)", "targets8": "three contigs, 8 columns",
                                                            "targets16": "three contigs, 16 columns", "sizing": "the sizing call"}),
            ("bam_sites_timing.txt", "bg_bam_sites_dev", {"sites_%s" % n: "sites, offsets and summaries: %s, strict" % n for n in ("wide", "targets", "genome")})]
    for fname, starts, labels in held:
        if not os.path.exists(os.path.join(prof, fname)):
            continue
        for key, label in labels.items():
            line = next(ln for ln in open(os.path.join(prof, fname)) if ln.startswith(starts) and label in ln)
            lo, hi = map(float, re.search(r"\(min ([\d.]+) max ([\d.]+)\)", line).groups())
            say("%s: %.3f ms now, %.3f .. %.3f ms on record: %s" % (key, med[key], lo, hi, "inside" if lo <= med[key] <= hi else
                                                                      "OUTSIDE by %+.1f %%" % (100 * (med[key] / (hi if med[key] > hi else lo) - 1))))
# ---- checks
EVENT = _lib.BAM_INDEL_DTYPE


def fetch(name, tag):
    full(name, tag)
    torch.cuda.synchronize()
    n, n_seq = totals[(name, tag)]
    return d_events[:40 * n].cpu().numpy().view(EVENT), d_iseq[:n_seq].cpu().numpy().tobytes(), d_event_off[:len(REGIONS[name]) + 1].cpu().numpy().astype(np.uint64)


entries = [(b"chr%d" % (c + 1), int(contigs.table["start"][c]), int(contigs.table["len"][c])) for c in range(3)]
off_host = d_sorted_off.cpu().numpy().astype(np.int64)
for tag in ("strict", "lax"):
    w_ev, w_seq, _ = fetch("wide", tag)
    p_ev, p_seq, p_off = fetch("pieces", tag)
    a, b = w_ev.copy(), p_ev.copy()
    a["region"] = b["region"] = 0
    assert totals[("wide", tag)] == totals[("pieces", tag)] and a.tobytes() == b.tobytes() and w_seq == p_seq, tag
    assert (np.searchsorted(p_off, np.arange(len(p_ev)), side="right") - 1 == p_ev["region"]).all(), tag
    s_ev, s_seq, s_off = fetch("sample", tag)
    pileup("sample", 16)
    torch.cuda.synchronize()
    rows = d_rows[:SAMPLE * 16].cpu().numpy().view(np.uint32).reshape(SAMPLE, 16)
    if tag == "strict":  # the sample's records: every live slot on chr1 that starts inside [SPAN - SAMPLE - 1000, SPAN)
        raw = d_bam_sorted.cpu().numpy()
        live = np.nonzero(off_host[1:] > off_host[:-1])[0]
        ref_pos = raw[off_host[live][:, None] + np.arange(4, 12)[None, :]].copy().view("<i4")
        pick = live[(ref_pos[:, 0] == 0) & (ref_pos[:, 1] >= SPAN - SAMPLE - 1000) & (ref_pos[:, 1] < SPAN)]
        slots = [raw[off_host[i]:off_host[i + 1]].tobytes() for i in pick]
    want, want_seq, want_off = io.from_rows(slots, rows, [0, SAMPLE], REGIONS["sample"], **KW[tag])
    assert io.as_tuples(s_ev) == want and s_seq == want_seq and s_off.tolist() == want_off, tag
say("checked, both thresholds: the span cut into 1 000 regions gives the events and sequences of the one region (their region index aside); the events, "
    "sequences and offsets of the last %d positions of the span are tests/bam_indels_oracle.py's on the sample's %d records, with the depth from the "
    "16-column pileup's rows" % (SAMPLE, len(slots)))
say("not measured: the host-buffer flavour, counters of any kernel")
say("source hash (tools/csrc_hash.py): %s" % csrc_sha())
if len(sys.argv) > 4:
    open(sys.argv[4], "w").write("tools/exp/time_bam_indels.py %d %d %d on one MI355X, device-resident: every call once per round between two device "
                                 "events, %d rounds after 2 warm-up rounds, medians\n" % (N_PAIRS, N_GENOME, REPEATS, REPEATS) + "\n".join(lines) + "\n")
