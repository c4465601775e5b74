"""Device-resident timing of the candidate sites (bg_bam_sites_dev), in one process (python tools/exp/time_bam_sites.py [PAIRS] [GENOME_BP]
[REPEATS] [OUT]), on the batch of tools/exp/time_bam_pileup.py (the set-up below is that tool's): the coordinate-sorted,
duplicate-flagged BAM records of PAIRS (default 500 000) pairs of 150 bp on a genome of three contigs, held against the genome
text they were drawn from.  Three sets of regions:
  * wide: ONE region, the first SPAN (default 30 000 000, at most chr1) positions of chr1;
  * targets: 20 000 regions of 300 positions, evenly spread over the three contigs;
  * genome: every contig whole, the input whose rows bg_bam_pileup cannot return.
Each call once per round between two device events; after 2 warm-up rounds REPEATS (default 9) rounds, medians with the rounds'
min and max.  The yardstick, in the same process on the same regions: bg_bam_pileup_dev with 16 columns, whose code this tool's
commit does not change; the 8- and 16-column pileup are timed again and held to the spread recorded in
profiles/bam_pileup_timing.txt.  The passes are told apart by differences of whole calls: the count pass is the sites' sizing
call less the pileup's (the same front); the scan, the summaries' reduction and the emit pass are the full call less the sizing call.
Checked: the sites of the wide region are those of the same span cut into 1 000 regions and the summaries add up; the sites and
the summary of a 1 Mbp sample are what tests/bam_sites_oracle.py's from_rows gives on the pileup's rows."""
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
import bam_sites_oracle as so  # noqa: E402

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
STRICT = dict(min_depth=2, min_alt=2, min_alt_permille=200)  # a caller's thresholds
LAX = dict()                                                 # every mismatch, deleted position and insertion
head = (N, d_bam_sorted.data_ptr(), d_sorted_off.data_ptr(), d_contigs.data_ptr(), 3)


def pileup(name, w, out=True):
    got = bam.pileup_dev(*head, d_regions[name].data_ptr(), len(REGIONS[name]), d_rows.data_ptr() if out else 0, n_rows[name] if out else 0, 0,
                         flags=bam.PILEUP_STRANDS if w == 16 else 0, stream=stream, ctx=ctx)
    assert got == n_rows[name]


def sites(name, kw, d_sites=0, cap=0, d_site_off=0, d_summary=0):
    return bam.sites_dev(*head, g_dev.data_ptr(), N_GENOME, d_regions[name].data_ptr(), len(REGIONS[name]), d_sites, cap, d_site_off, d_summary,
                         stream=stream, ctx=ctx, **kw)


n_sites = {(name, tag): sites(name, kw) for name in REGIONS for tag, kw in (("strict", STRICT), ("lax", LAX))}
d_sites = torch.zeros(max(n_sites.values()) * 32, dtype=torch.uint8, device=dev)
d_site_off = torch.zeros(N_TARGETS + 1, dtype=torch.int64, device=dev)
d_summary = torch.zeros(N_TARGETS * 48, dtype=torch.uint8, device=dev)


def full(name, tag):
    kw = STRICT if tag == "strict" else LAX
    assert sites(name, kw, d_sites.data_ptr(), n_sites[(name, tag)], d_site_off.data_ptr(), d_summary.data_ptr()) == n_sites[(name, tag)]


CALLS = [
    ("wide8", "bg_bam_pileup_dev, one region of %d positions of chr1, 8 columns" % SPAN, lambda: pileup("wide", 8)),
    ("wide16", "bg_bam_pileup_dev, one region of %d positions of chr1, 16 columns (the yardstick)" % SPAN, lambda: pileup("wide", 16)),
    ("targets8", "bg_bam_pileup_dev, %d regions of %d positions over the three contigs, 8 columns" % (len(targets), TARGET), lambda: pileup("targets", 8)),
    ("targets16", "bg_bam_pileup_dev, %d regions of %d positions, 16 columns (the yardstick)" % (len(targets), TARGET), lambda: pileup("targets", 16)),
    ("sizing", "bg_bam_pileup_dev, the sizing call of the wide region (the front alone)", lambda: pileup("wide", 8, out=False)),
    ("sizing_targets", "bg_bam_pileup_dev, the sizing call of the targets (the front alone)", lambda: pileup("targets", 8, out=False)),
    ("sizing_genome", "bg_bam_pileup_dev, the sizing call of the whole contigs (the front alone)", lambda: pileup("genome", 8, out=False)),
]
for name in ("wide", "targets", "genome"):
    for tag in ("strict", "lax"):
        what = "%s, %s thresholds (%d sites)" % (name, tag, n_sites[(name, tag)])
        CALLS.append(("size_%s_%s" % (name, tag), "bg_bam_sites_dev, the sizing call: " + what, lambda name=name, tag=tag: sites(name, STRICT if tag == "strict" else LAX)))
        CALLS.append(("full_%s_%s" % (name, tag), "bg_bam_sites_dev, sites, offsets and summaries: " + what, lambda name=name, tag=tag: full(name, tag)))
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
    say("%-125s median %8.3f ms (min %.3f max %.3f)" % (name, med[key], t[0], t[-1]))
for name, yard, front in (("wide", "wide16", "sizing"), ("targets", "targets16", "sizing_targets"), ("genome", None, "sizing_genome")):
    for tag in ("strict", "lax"):
        size, whole = med["size_%s_%s" % (name, tag)], med["full_%s_%s" % (name, tag)]
        say("%s, %s: the front %.3f ms, the count pass %.3f ms, the scan and second read-back with the emit pass and the summaries %.3f ms; the full call %s" % (
            name, tag, med[front], size - med[front], whole - size,
            "%.2f x the 16-column pileup; its tile pass alone takes %.3f ms" % (whole / med[yard], med[yard] - med[front]) if yard else
            "%.3f ms for rows the pileup cannot return (%.1f GB with 16 columns)" % (whole, n_rows[name] * 64 / 1e9)))
# ---- the factoring cost nothing: the pileup's figures against the spread on record
record = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "profiles", "bam_pileup_timing.txt")
labels = {"wide8": "8 columns  ", "wide16": "16 columns (BG_PILEUP_STRANDS)", "targets8": "three contigs, 8 columns", "targets16": "three contigs, 16 columns",
          "sizing": "the sizing call"}
if os.path.exists(record) and N_PAIRS == 500_000 and N_GENOME == 100_000_000 and SPAN == 30_000_000:
    import re
    for key, label in labels.items():
        line = next(ln for ln in open(record) if ln.startswith("bg_bam_pileup_dev") and label in ln)
        lo, hi = map(float, re.search(r"\(min ([\d.]+) max ([\d.]+)\)", line).groups())
        say("%s: %.3f ms now, %.3f .. %.3f ms on record: %s" % (key, med[key], lo, hi, "inside" if lo <= med[key] <= hi else
                                                                  "OUTSIDE by %+.1f %%" % (100 * (med[key] / (hi if med[key] > hi else lo) - 1))))
# ---- checks
SITE, SUMMARY = _lib.BAM_SITE_DTYPE, _lib.BAM_REGION_SUMMARY_DTYPE


def fetch(name, tag):
    full(name, tag)
    torch.cuda.synchronize()
    n, nr = n_sites[(name, tag)], len(REGIONS[name])
    return (d_sites[:32 * n].cpu().numpy().view(SITE), d_site_off[:nr + 1].cpu().numpy().astype(np.uint64), d_summary[:48 * nr].cpu().numpy().view(SUMMARY))


for tag in ("strict", "lax"):
    w_sites, _, w_sum = fetch("wide", tag)
    p_sites, p_off, p_sum = fetch("pieces", tag)
    a, b = w_sites.copy(), p_sites.copy()
    a["region"] = b["region"] = 0
    assert n_sites[("wide", tag)] == n_sites[("pieces", tag)] and a.tobytes() == b.tobytes(), tag
    assert (np.searchsorted(p_off, np.arange(len(p_sites)), side="right") - 1 == p_sites["region"]).all(), tag
    for f in ("sum_depth", "match", "mismatch", "n_ref_other"):
        assert int(p_sum[f].sum()) == int(w_sum[f][0]), (tag, f)
    assert (p_sum["covered"].sum(axis=0) == w_sum["covered"][0]).all() and int(p_sum["max_depth"].max()) == int(w_sum["max_depth"][0]), tag
    s_sites, s_off, s_sum = fetch("sample", tag)
    pileup("sample", 16)
    torch.cuda.synchronize()
    rows = d_rows[:SAMPLE * 16].cpu().numpy().view(np.uint32).reshape(SAMPLE, 16)
    entries = [(b"chr%d" % (c + 1), int(contigs.table["start"][c]), int(contigs.table["len"][c])) for c in range(3)]
    text = g_dev[:SPAN].cpu().numpy().tobytes()
    want, want_off, want_sum = so.from_rows(rows, [0, SAMPLE], REGIONS["sample"], entries, text, so.params(**(STRICT if tag == "strict" else LAX)))
    assert so.as_tuples(s_sites) == want and s_off.tolist() == want_off and so.as_dicts(s_sum) == want_sum, tag
    if tag == "lax":
        say("wide: mean depth %.3f, max %d, %d positions at depth 0; match %d, mismatch %d; sites: %d SNV, %d DEL, %d INS (lax), %d in all (strict)" % (
            int(w_sum["sum_depth"][0]) / SPAN, int(w_sum["max_depth"][0]), SPAN - int(w_sum["covered"][0][0]), int(w_sum["match"][0]), int(w_sum["mismatch"][0]),
            int((w_sites["kind"] == 0).sum()), int((w_sites["kind"] == 1).sum()), int((w_sites["kind"] == 2).sum()), n_sites[("wide", "strict")]))
say("checked, both thresholds: the span cut into 1 000 regions gives the sites of the one region (their region index aside) and summaries that add up; "
    "the sites, offsets and summary of the last %d positions of the span are from_rows' on the 16-column pileup's rows" % SAMPLE)
say("not measured: the host-buffer flavour, counters of any kernel")
say("source hash (tools/csrc_hash.py): %s" % csrc_sha())
if len(sys.argv) > 4:
    open(sys.argv[4], "w").write("tools/exp/time_bam_sites.py %d %d %d on one MI355X, device-resident: every call once per round between two device "
                                 "events, %d rounds after 2 warm-up rounds, medians\n" % (N_PAIRS, N_GENOME, REPEATS, REPEATS) + "\n".join(lines) + "\n")
