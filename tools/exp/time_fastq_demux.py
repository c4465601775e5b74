"""Device-resident timing of the demultiplexer next to the calls around it, in one process
(python tools/exp/time_fastq_demux.py [READS] [REPEATS] [OUT]):
  * READS (default 1 M) reads of 150 bp generated as bench.py's FASTQ leg generates them (synth.fastq_text), the first 8 bases of
    95 % of them overwritten by one of 96 barcodes (any two at least 3 substitutions apart), a fifth of those with one
    substitution; parsed on the device;
  * bg_myers_best_batch_dev (96 patterns, k = 1, coordinates only), bg_fastq_demux_assign_dev (ANCHOR_5P, margin 1),
    bg_fastq_trim_dev (5', n_pat = 1, on assign's one record per read), bg_fastq_demux_split_dev (without the host offsets; with
    and without the hit records, and at 1024 bins on the same records), bg_fastq_emit_dev over the split columns, and as yardsticks bg_fastq_filter_dev (min_len 1:
    a copy of the same trimmed records) and bg_fastq_parse_dev;
  * after 2 warm-up rounds, REPEATS (default 9) rounds that run every call once, in turn, between two device events; the
    figures are medians over the rounds.
Algorithmic bytes of assign: the four words of every record it looks at in a 64-byte line (counted as the line), 72 bytes out;
of split and filter: records, offsets, sequences and qualities once read and once written (split: plus bin, perm and two
lengths per record and the (group, tile) table twice)."""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from rust_bio_amd import _lib, fastq, myers, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 9
L, K, N_BC, COPY_GBS = 150, 1, 96, 6290.0
rng = np.random.default_rng(12)


def barcodes():
    out = []
    while len(out) < N_BC:
        c = rng.integers(0, 4, size=8)
        if all((c != o).sum() >= 3 for o in out):
            out.append(c)
    return np.frombuffer(b"ACGT", np.uint8)[np.array(out)]


def reads_text(bcs):
    text = synth.fastq_text(N, L, seed=6).copy()
    rows = text.reshape(N, len(text) // N)
    o = int(np.nonzero(rows[0] == 10)[0][0]) + 1
    with_bc = np.nonzero(rng.random(N) < 0.95)[0]
    bc = bcs[rng.integers(0, N_BC, size=len(with_bc))].copy()
    sub = np.nonzero(rng.random(len(with_bc)) < 0.2)[0]
    bc[sub, rng.integers(0, 8, size=len(sub))] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=len(sub))]
    rows[with_bc, o:o + 8] = bc
    return text


lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


ctx = _lib.default_context()
stream = torch.cuda.current_stream().cuda_stream
bcs = barcodes()
d_fq = torch.from_numpy(reads_text(bcs)).cuda()
bufs = fastq.alloc_dev(d_fq.numel(), d_fq.device)
n, status, _, d_recs, d_seq, d_so, d_qual, d_qo = fastq.parse_dev(d_fq, bufs=bufs, stream=stream)
assert (n, status) == (N, "ok")
pats = [myers.Myers(b.tobytes()) for b in bcs]
pat_bin = np.arange(N_BC, dtype=np.uint32)
hits = myers.best_batch_dev(pats, d_seq, d_so, K, stream=stream)
prm = dict(flags=fastq.DMX_ANCHOR_5P, min_margin=1, max_offset=1)
asg = fastq.demux_assign_dev(N, hits[0], N_BC, pat_bin, N_BC, stream=stream, **prm)
d_bin, d_hit = asg[0], asg[1]
trim = myers.trim_dev(myers.TRIM_5P, d_hit, 1, N, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream)
t_recs, t_seq, t_so, t_qual, t_qo, (t_sb, t_qb) = trim
spl = fastq.demux_split_dev(N, d_bin, N_BC, t_recs, t_seq, t_so, t_qual, t_qo, d_hit=d_hit, stream=stream)
bin_off = spl[8]
spl_cols = fastq.demux_split_dev(N, d_bin, N_BC, t_recs, t_seq, t_so, t_qual, t_qo, stream=stream)
# the same records over 1024 bins: the bin of a read spread by its index
d_bin_wide = (d_bin.to(torch.int64) + N_BC * (torch.arange(N, device=d_bin.device) % 10)).to(torch.int32)
spl_wide = fastq.demux_split_dev(N, d_bin_wide, 1024, t_recs, t_seq, t_so, t_qual, t_qo, stream=stream)
flt = fastq.filter_dev(N, t_recs, t_seq, t_so, t_qual, t_qo, min_len=1, stream=stream)
kept, f_sb, f_qb = flt[6]
emt = fastq.emit_dev(N, d_fq, spl[0], spl[1], spl[3], stream=stream)
texts = fastq.demux_texts(emt[0], emt[1], bin_off, N_BC)
assert sum(int(t.numel()) for t in texts) == emt[2]

col_bytes = 2 * (56 * N + 2 * 8 * N + t_sb + t_qb)
tiles = (N + 2047) // 2048
extra = 4 * N + 2 * 8 * N + 4 * 4 * N  # bin, perm and the two lengths, written and read


def split_call(bins, n_bins, out, **kw):
    return lambda: fastq.demux_split_dev(N, bins, n_bins, t_recs, t_seq, t_so, t_qual, t_qo, stream=stream, want_bin_off=False, out=out, **kw)


CALLS = [
    ("parse", "bg_fastq_parse_dev (yardstick)", d_fq.numel(), lambda: fastq.parse_dev(d_fq, bufs=bufs, stream=stream)),
    ("best", "bg_myers_best_batch_dev, 96 patterns, k = 1, coordinates only", N * L + 8 * N + 64 * N * N_BC,
     lambda: myers.best_batch_dev(pats, d_seq, d_so, K, stream=stream, out=hits)),
    ("assign", "bg_fastq_demux_assign_dev, 96 patterns -> 96 bins", 64 * N * N_BC + 72 * N,
     lambda: fastq.demux_assign_dev(N, hits[0], N_BC, pat_bin, N_BC, stream=stream, out=asg, **prm)),
    ("trim", "bg_fastq_trim_dev 5', n_pat 1, on assign's records (no totals)", 64 * N + 2 * 56 * N + 4 * 8 * N + 2 * (N * L + t_sb),
     lambda: myers.trim_dev(myers.TRIM_5P, d_hit, 1, N, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream, want_totals=False, out=trim)),
    ("split", "bg_fastq_demux_split_dev, 96 bins, columns only (no host offsets)", col_bytes + extra + 2 * 12 * 98 * tiles,
     split_call(d_bin, N_BC, spl_cols)),
    ("split_hit", "bg_fastq_demux_split_dev, 96 bins, with the hit records", col_bytes + 2 * 64 * N + extra + 2 * 12 * 98 * tiles,
     split_call(d_bin, N_BC, spl, d_hit=d_hit)),
    ("split_wide", "bg_fastq_demux_split_dev, 1024 bins, columns only", col_bytes + extra + 2 * 12 * 1026 * tiles,
     split_call(d_bin_wide, 1024, spl_wide)),
    ("filter", "bg_fastq_filter_dev min_len 1 on the same records (yardstick; no totals)", 56 * (N + kept) + 2 * 8 * (N + kept) + 2 * (f_sb + f_qb),
     lambda: fastq.filter_dev(N, t_recs, t_seq, t_so, t_qual, t_qo, min_len=1, stream=stream, want_totals=False, out=flt)),
    ("emit", "bg_fastq_emit_dev step 1 over the split columns: every sample's text", 2 * emt[2] + 64 * N,
     lambda: fastq.emit_dev(N, d_fq, spl[0], spl[1], spl[3], stream=stream, out=emt[:2])),
]
ms = {c[0]: [] for c in CALLS}
for rnd in range(2 + REPEATS):
    for key, _, _, f in CALLS:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        if rnd >= 2:
            ms[key].append(a.elapsed_time(b))
med = {}
for key, name, nbytes, _ in CALLS:
    t = sorted(ms[key])
    med[key] = m = t[len(t) // 2]
    gbs = nbytes / m / 1e6
    say("%-74s median %8.3f ms (min %.3f max %.3f)  %7.1f M reads/s  %8.1f MB algorithmic, %6.1f GB/s = %.3f of copy" % (
        name, m, t[0], t[-1], N / m / 1e3, nbytes / 1e6, gbs, gbs / COPY_GBS))
b = d_bin.cpu().numpy().view(np.uint32)
say("assign: %d of %d reads assigned, %d unassigned, %d ambiguous; the trim keeps %d of %d bases; the emit writes %.1f MB: %d sample texts of "
    "%.2f .. %.2f MB, then the unassigned and the ambiguous reads" % (
        (b < N_BC).sum(), N, (b == N_BC).sum(), (b == N_BC + 1).sum(), t_sb, N * L, emt[2] / 1e6, N_BC,
        min(int(t.numel()) for t in texts[:N_BC]) / 1e6, max(int(t.numel()) for t in texts[:N_BC]) / 1e6))
say("split / filter, both moving the same %.1f MB of records, offsets, sequences and qualities: %.2f at 96 bins, %.2f at 1024 bins; "
    "%.2f with the %.1f MB of hit records carried along" % (col_bytes / 2e6, med["split"] / med["filter"], med["split_wide"] / med["filter"],
                                                           med["split_hit"] / med["filter"], 64 * N / 1e6))
after = med["assign"] + med["trim"] + med["split_hit"] + med["emit"]
say("assign + trim + split + emit: %.3f ms = %.3f of the Myers call that feeds them" % (after, after / med["best"]))
if len(sys.argv) > 3:
    open(sys.argv[3], "w").write("tools/exp/time_fastq_demux.py %d %d on one MI355X, device-resident: every call once per round between two "
                                 "device events, %d rounds after 2 warm-up rounds, medians\n" % (N, REPEATS, REPEATS) + "\n".join(lines) + "\n")
