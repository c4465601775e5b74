"""Device-resident timing of the left-aligned indel events (bg_bam_indels_left_dev), in one process (python
tools/exp/time_bam_indels_left.py [PAIRS] [GENOME_BP] [REPEATS] [OUT]), on the batch and the three region sets of
tools/exp/time_bam_indels.py (the set-up below is that tool's): wide, targets, genome.  Each call once per round between two
device events; after 2 warm-up rounds REPEATS (default 9) rounds, medians with the rounds' min and max.  The yardstick, in the same
process on the same regions: bg_bam_indels_dev, full and sizing, lax thresholds.  Timed: the full and the sizing call at max_shift
0 and without a limit; the count pass, the emit pass and the sort by differences of whole calls (the ctx option
indels_stop_after).  bg_bam_indels_dev, bg_bam_sites_dev and bg_bam_pileup_dev are timed again and held to the spreads recorded
in profiles/bam_indels_timing.txt.  Counted: the raw events against the events before and behind the shift (how many merged);
the histogram of k over the records of a 1 Mbp sample (tests/bam_indels_left_oracle.py: the device hands no k out).
Checked: max_shift 0 gives the bytes of bg_bam_indels_dev; the events of the sample are what the oracle gives on the sample's
records, with the depth from the 16-column pileup's rows."""
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
import bam_indels_left_oracle as lo  # noqa: E402
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
LAX = dict()
NO_LIMIT = 0xFFFFFFFF
TEXT = (g_dev.data_ptr(), N_GENOME)


def pileup(name, w, out=True):
    got = bam.pileup_dev(*head, d_regions[name].data_ptr(), len(REGIONS[name]), d_rows.data_ptr() if out else 0, n_rows[name] if out else 0, 0,
                         flags=bam.PILEUP_STRANDS if w == 16 else 0, stream=stream, ctx=ctx)
    assert got == n_rows[name]


def sites(name, d_sites=0, cap=0, d_site_off=0, d_summary=0):
    return bam.sites_dev(*head, *TEXT, d_regions[name].data_ptr(), len(REGIONS[name]), d_sites, cap, d_site_off, d_summary, stream=stream, ctx=ctx, **STRICT)


def plain(name, d_events=0, cap=0, d_seq=0, seq_cap=0, d_event_off=0, **kw):
    return bam.indels_dev(*head, d_regions[name].data_ptr(), len(REGIONS[name]), d_events, cap, d_seq, seq_cap, d_event_off, stream=stream, ctx=ctx, **kw)


def left(name, max_shift, d_events=0, cap=0, d_seq=0, seq_cap=0, d_event_off=0):
    return bam.indels_left_dev(*head, *TEXT, d_regions[name].data_ptr(), len(REGIONS[name]), d_events, cap, d_seq, seq_cap, d_event_off, stream=stream, ctx=ctx,
                               max_shift=max_shift)


def staged(fn, stop):
    """a lax sizing call ended behind pass `stop`"""
    ctx.set_option("indels_stop_after", stop)
    try:
        assert fn() == (0, 0)
    finally:
        ctx.set_option("indels_stop_after", 0)


NAMES = ("wide", "targets", "genome")
n_sites = {name: sites(name) for name in NAMES}
d_sites = torch.zeros(max(n_sites.values()) * 32, dtype=torch.uint8, device=dev)
d_site_off = torch.zeros(N_TARGETS + 1, dtype=torch.int64, device=dev)
d_summary = torch.zeros(N_TARGETS * 48, dtype=torch.uint8, device=dev)
totals = {(name, "plain"): plain(name) for name in REGIONS}
totals.update({(name, "plain_strict"): plain(name, **STRICT) for name in NAMES})
totals.update({(name, ms_): left(name, ms_) for name in REGIONS for ms_ in (0, NO_LIMIT)})
d_events = torch.zeros(max(t[0] for t in totals.values()) * 40 + 8, dtype=torch.uint8, device=dev)
d_iseq = torch.zeros(max(t[1] for t in totals.values()) + 1, dtype=torch.uint8, device=dev)
d_event_off = torch.zeros(N_TARGETS + 1, dtype=torch.int64, device=dev)
OUT = lambda key: (d_events.data_ptr(), totals[key][0], d_iseq.data_ptr(), totals[key][1], d_event_off.data_ptr())  # noqa: E731


def full_sites(name):
    assert sites(name, d_sites.data_ptr(), n_sites[name], d_site_off.data_ptr(), d_summary.data_ptr()) == n_sites[name]


def full_plain(name, tag="plain", **kw):
    assert plain(name, *OUT((name, tag)), **kw) == totals[(name, tag)]


def full_left(name, max_shift):
    assert left(name, max_shift, *OUT((name, max_shift))) == totals[(name, max_shift)]


CALLS = [
    ("wide8", "bg_bam_pileup_dev, one region of %d positions of chr1, 8 columns" % SPAN, lambda: pileup("wide", 8)),
    ("wide16", "bg_bam_pileup_dev, one region of %d positions of chr1, 16 columns" % SPAN, lambda: pileup("wide", 16)),
    ("targets8", "bg_bam_pileup_dev, %d regions of %d positions over the three contigs, 8 columns" % (len(targets), TARGET), lambda: pileup("targets", 8)),
    ("targets16", "bg_bam_pileup_dev, %d regions of %d positions, 16 columns" % (len(targets), TARGET), lambda: pileup("targets", 16)),
    ("sizing", "bg_bam_pileup_dev, the sizing call of the wide region (the front alone)", lambda: pileup("wide", 8, out=False)),
    ("sizing_targets", "bg_bam_pileup_dev, the sizing call of the targets (the front alone)", lambda: pileup("targets", 8, out=False)),
    ("sizing_genome", "bg_bam_pileup_dev, the sizing call of the whole contigs (the front alone)", lambda: pileup("genome", 8, out=False)),
]
for name in NAMES:
    CALLS.append(("sites_%s" % name, "bg_bam_sites_dev, sites, offsets and summaries: %s, strict thresholds (%d sites)" % (name, n_sites[name]),
                  lambda name=name: full_sites(name)))
    what = "%s, lax thresholds (%d events, %d sequence bytes)" % ((name,) + totals[(name, "plain")])
    CALLS.append(("size_%s_lax" % name, "bg_bam_indels_dev, the sizing call: " + what + " (the yardstick)", lambda name=name: plain(name)))
    CALLS.append(("full_%s_lax" % name, "bg_bam_indels_dev, events, sequences and offsets: " + what + " (the yardstick)", lambda name=name: full_plain(name)))
    what = "%s, strict thresholds (%d events, %d sequence bytes)" % ((name,) + totals[(name, "plain_strict")])
    CALLS.append(("full_%s_strict" % name, "bg_bam_indels_dev, events, sequences and offsets: " + what, lambda name=name: full_plain(name, "plain_strict", **STRICT)))
    for stop, pass_ in ((1, "the count pass"), (2, "the emit pass"), (3, "the sort")):
        CALLS.append(("pstop%d_%s" % (stop, name), "bg_bam_indels_dev, %s, ended behind %s" % (name, pass_), lambda name=name, stop=stop: staged(lambda: plain(name), stop)))
    for ms_, label in ((0, "max_shift 0"), (NO_LIMIT, "no limit")):
        what = "%s, %s, lax thresholds (%d events, %d sequence bytes)" % ((name, label) + totals[(name, ms_)])
        CALLS.append(("lsize_%s_%d" % (name, ms_), "bg_bam_indels_left_dev, the sizing call: " + what, lambda name=name, ms_=ms_: left(name, ms_)))
        CALLS.append(("lfull_%s_%d" % (name, ms_), "bg_bam_indels_left_dev, events, sequences and offsets: " + what, lambda name=name, ms_=ms_: full_left(name, ms_)))
        for stop, pass_ in ((1, "the count pass"), (2, "the emit pass"), (3, "the sort")):
            CALLS.append(("lstop%d_%s_%d" % (stop, name, ms_), "bg_bam_indels_left_dev, %s, %s, ended behind %s" % (name, label, pass_),
                          lambda name=name, ms_=ms_, stop=stop: staged(lambda: left(name, ms_), stop)))
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
    say("%-150s median %8.3f ms (min %.3f max %.3f)" % (name, med[key], t[0], t[-1]))
EVENT = _lib.BAM_INDEL_DTYPE


def fetch(fn, key):
    fn()
    torch.cuda.synchronize()
    n, n_seq = totals[key]
    return (d_events[:40 * n].cpu().numpy().view(EVENT).copy(), d_iseq[:n_seq].cpu().numpy().tobytes(),
            d_event_off[:len(REGIONS[key[0]]) + 1].cpu().numpy().astype(np.uint64))


for name in NAMES:
    front = med[{"wide": "sizing", "targets": "sizing_targets", "genome": "sizing_genome"}[name]]
    p_ev, p_seq, p_off = fetch(lambda: full_plain(name), (name, "plain"))
    z_ev, z_seq, z_off = fetch(lambda: full_left(name, 0), (name, 0))
    assert p_ev.tobytes() == z_ev.tobytes() and p_seq == z_seq and p_off.tobytes() == z_off.tobytes(), name
    l_ev, _, _ = fetch(lambda: full_left(name, NO_LIMIT), (name, NO_LIMIT))
    n_raw = int(p_ev["alt_fwd"].sum(dtype=np.uint64) + p_ev["alt_rev"].sum(dtype=np.uint64))
    assert n_raw == int(l_ev["alt_fwd"].sum(dtype=np.uint64) + l_ev["alt_rev"].sum(dtype=np.uint64)) or name == "targets"
    say("%s: %d raw events; %d events as spelt, %d left-aligned (%d fewer, %.2f %%); events with alt >= 2: %d as spelt, %d left-aligned" % (
        name, n_raw, len(p_ev), len(l_ev), len(p_ev) - len(l_ev), 100 * (len(p_ev) - len(l_ev)) / max(len(p_ev), 1),
        int((p_ev["alt_fwd"] + p_ev["alt_rev"] >= 2).sum()), int((l_ev["alt_fwd"] + l_ev["alt_rev"] >= 2).sum())))
    for label, pre, suf, size, whole in (("bg_bam_indels_dev", "pstop", "_" + name, "size_%s_lax" % name, "full_%s_lax" % name),
                                         ("bg_bam_indels_left_dev, max_shift 0", "lstop", "_%s_0" % name, "lsize_%s_0" % name, "lfull_%s_0" % name),
                                         ("bg_bam_indels_left_dev, no limit", "lstop", "_%s_%d" % (name, NO_LIMIT), "lsize_%s_%d" % (name, NO_LIMIT),
                                          "lfull_%s_%d" % (name, NO_LIMIT))):
        s1, s2, s3 = (med["%s%d%s" % (pre, k, suf)] for k in (1, 2, 3))
        say("%s, %s: the front %.3f ms, the count pass with its scan and read-back %.3f ms, the emit pass %.3f ms, the sort %.3f ms, heads to the third read-back "
            "%.3f ms, records and sequences out %.3f ms; sizing %.3f ms = %.3f x the yardstick's, full %.3f ms = %.3f x the yardstick's" % (
                name, label, front, s1 - front, s2 - s1, s3 - s2, med[size] - s3, med[whole] - med[size], med[size], med[size] / med["size_%s_lax" % name],
                med[whole], med[whole] / med["full_%s_lax" % name]))
# ---- the unchanged calls against the spreads on record
import re  # noqa: E402
prof = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "profiles", "bam_indels_timing.txt")
if N_PAIRS == 500_000 and N_GENOME == 100_000_000 and SPAN == 30_000_000 and os.path.exists(prof):
    for key, _, _ in CALLS:
        if key.startswith(("l", "pstop")):
            continue
        label = next(c[1] for c in CALLS if c[0] == key).split(" (")[0].replace(" (the yardstick)", "")
        line = next((ln for ln in open(prof) if ln.startswith(label) and "median" in ln), None)
        if line is None:
            say("%s: %.3f ms now, no line on record" % (key, med[key]))
            continue
        lo_, hi_ = map(float, re.search(r"\(min ([\d.]+) max ([\d.]+)\)", line).groups())
        say("%s: %.3f ms now, %.3f .. %.3f ms on record: %s" % (key, med[key], lo_, hi_, "inside" if lo_ <= med[key] <= hi_ else
                                                                  "OUTSIDE by %+.1f %%" % (100 * (med[key] / (hi_ if med[key] > hi_ else lo_) - 1))))
# ---- the sample: the oracle's events and the histogram of k
entries = [(b"chr%d" % (c + 1), int(contigs.table["start"][c]), int(contigs.table["len"][c])) for c in range(3)]
off_host = d_sorted_off.cpu().numpy().astype(np.int64)
raw = d_bam_sorted.cpu().numpy()
live = np.nonzero(off_host[1:] > off_host[:-1])[0]
ref_pos = raw[off_host[live][:, None] + np.arange(4, 12)[None, :]].copy().view("<i4")
pick = live[(ref_pos[:, 0] == 0) & (ref_pos[:, 1] >= SPAN - SAMPLE - 1000) & (ref_pos[:, 1] < SPAN)]
slots = [raw[off_host[i]:off_host[i + 1]].tobytes() for i in pick]
chr1 = g_dev[:int(contigs.table["len"][0]) + 1].cpu().numpy().tobytes()
s_ev, s_seq, s_off = fetch(lambda: full_left("sample", NO_LIMIT), ("sample", NO_LIMIT))
pileup("sample", 16)
torch.cuda.synchronize()
rows = d_rows[:SAMPLE * 16].cpu().numpy().view(np.uint32).reshape(SAMPLE, 16)
want, want_seq, want_off = lo.from_rows(slots, entries[:1], chr1, rows, [0, SAMPLE], REGIONS["sample"])
assert io.as_tuples(s_ev) == want and s_seq == want_seq and s_off.tolist() == want_off
hist = {}
for _, _, _, _, k, _ in lo.shifted_events(slots, entries[:1], chr1, lo.params()):
    hist[k] = hist.get(k, 0) + 1
say("k over the %d raw events of the sample's %d records: %s" % (sum(hist.values()), len(slots), ", ".join("%d: %d" % kv for kv in sorted(hist.items()))))
say("checked: max_shift 0 gives the bytes of bg_bam_indels_dev on all three region sets; the left-aligned events, sequences and offsets of the last %d "
    "positions of the span are tests/bam_indels_left_oracle.py's on the sample's records, with the depth from the 16-column pileup's rows" % SAMPLE)
say("not measured: the host-buffer flavour, counters of any kernel, wider text loads in the step loop")
say("source hash (tools/csrc_hash.py): %s" % csrc_sha())
if len(sys.argv) > 4:
    open(sys.argv[4], "w").write("tools/exp/time_bam_indels_left.py %d %d %d on one MI355X, device-resident: every call once per round between two device "
                                 "events, %d rounds after 2 warm-up rounds, medians\n" % (N_PAIRS, N_GENOME, REPEATS, REPEATS) + "\n".join(lines) + "\n")
