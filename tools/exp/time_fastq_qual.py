"""Device-resident timing of the quality calls next to the calls around them, in one process
(python tools/exp/time_fastq_qual.py [READS] [REPEATS] [OUT]):
  * READS (default 1 M) reads of 150 bp generated as bench.py's FASTQ leg generates them (synth.fastq_text), their qualities
    overwritten: 38 +- 3 with a tail of 0 .. 30 symbols of 2 .. 12, a tenth of the reads 2 .. 40 throughout; 30 % of the reads
    end in 10 .. 18 bases of an adapter; parsed on the device;
  * yardsticks: bg_fastq_parse_dev (the ingest), bg_myers_best_batch_dev + bg_fastq_trim_dev (the adapter trim),
    bg_fastq_filter_dev with max_n counting (reads the sequence column as the cut and the select read the quality column), and
    a device-to-device copy of the quality column alone;
  * bg_fastq_qual_cut_dev (RUNSUM at both ends; RUNSUM 5' + WINDOW 4), bg_fastq_qual_select_dev (without and with a weight
    table), bg_fastq_qc_tables_dev (max_cycles 150 and 1024), and the cut followed by the two trims;
  * after 2 warm-up rounds, REPEATS (default 9) rounds that run every call once, in turn, between two device events; the
    figures are medians over the rounds.  No call asks for a host total, so none synchronises.
Algorithmic bytes: the quality column and its offsets once, plus 64 (cut) or 36 (select: statistics and bin) bytes per read
written; the tables: both columns and both offset columns."""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from rust_bio_amd import _lib, fastq, myers, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 9
L, K, CUTOFF = 150, 2, 20
ADAPTER = b"AGATCGGAAGAGCACACG"
rng = np.random.default_rng(21)


def reads_text():
    text = synth.fastq_text(N, L, seed=6).copy()
    rows = text.reshape(N, len(text) // N)
    o = int(np.nonzero(rows[0] == 10)[0][0]) + 1
    q = rng.integers(35, 42, size=(N, L))
    tail = rng.integers(0, 31, size=N)
    low = rng.integers(2, 13, size=(N, L))
    q = np.where(np.arange(L)[None, :] >= (L - tail)[:, None], low, q)
    mixed = rng.random(N) < 0.1
    q[mixed] = rng.integers(2, 41, size=(int(mixed.sum()), L))
    rows[:, o + L + 3:o + 2 * L + 3] = (q + 33).astype(np.uint8)
    ad = np.frombuffer(ADAPTER, np.uint8)
    for r in np.nonzero(rng.random(N) < 0.3)[0]:
        k = int(rng.integers(10, len(ad) + 1))
        rows[r, o + L - k:o + L] = ad[:k]
    return text


lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


ctx = _lib.default_context()
stream = torch.cuda.current_stream().cuda_stream
d_fq = torch.from_numpy(reads_text()).cuda()
bufs = fastq.alloc_dev(d_fq.numel(), d_fq.device)
n, status, _, d_recs, d_seq, d_so, d_qual, d_qo = fastq.parse_dev(d_fq, bufs=bufs, stream=stream)
assert (n, status) == (N, "ok")
pats = [myers.Myers(ADAPTER[:10])]
hits = myers.best_batch_dev(pats, d_seq, d_so, K, stream=stream)
atrim = myers.trim_dev(myers.TRIM_3P, hits[0], 1, N, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream)
flt = fastq.filter_dev(N, d_recs, d_seq, d_so, d_qual, d_qo, max_n=5, stream=stream)
kept, f_sb, f_qb = flt[6]
q_copy = torch.empty(N * L, dtype=torch.uint8, device=d_qual.device)
both = dict(method_5p=fastq.QCUT_RUNSUM, method_3p=fastq.QCUT_RUNSUM, cutoff_5p=CUTOFF, cutoff_3p=CUTOFF)
win = dict(method_5p=fastq.QCUT_RUNSUM, method_3p=fastq.QCUT_WINDOW, cutoff_5p=CUTOFF, cutoff_3p=CUTOFF, window=4)
cut, cut_tot = fastq.qual_cut_dev(N, d_qual, d_qo, stream=stream, want_totals=True, **both)
cut_w, cut_w_tot = fastq.qual_cut_dev(N, d_qual, d_qo, stream=stream, want_totals=True, **win)
sp = dict(min_mean_q=25, low_q=15, max_low_pct=20)
sel = fastq.qual_select_dev(N, d_qual, d_qo, stream=stream, want_totals=True, **sp)
weight = fastq.ee_weights(33)
sel_w = fastq.qual_select_dev(N, d_qual, d_qo, weight=weight, max_weight=2 << 20, stream=stream, want_totals=True, **sp)
tab150 = fastq.qc_tables_dev(N, d_seq, d_so, d_qual, d_qo, 150, stream=stream)
tab1024 = fastq.qc_tables_dev(N, d_seq, d_so, d_qual, d_qo, 1024, stream=stream)
t3 = myers.trim_dev(myers.TRIM_3P, cut, 1, N, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream)
t5 = myers.trim_dev(myers.TRIM_5P, cut, 1, N, *t3[:5], stream=stream)
torch.cuda.synchronize()
assert int(tab150.n_reads[0]) == N == int(tab1024.n_reads[0]) and int(tab150.base[:150].sum()) == N * L
assert N * L - t5[5][1] == cut_tot[1]


def cut_and_trims():
    fastq.qual_cut_dev(N, d_qual, d_qo, stream=stream, out=cut, **both)
    myers.trim_dev(myers.TRIM_3P, cut, 1, N, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream, want_totals=False, out=t3)
    myers.trim_dev(myers.TRIM_5P, cut, 1, N, *t3[:5], stream=stream, want_totals=False, out=t5)


qcol = N * L + 8 * N
CALLS = [
    ("parse", "bg_fastq_parse_dev (the ingest; yardstick of the tables)", d_fq.numel(), lambda: fastq.parse_dev(d_fq, bufs=bufs, stream=stream)),
    ("adapter", "bg_myers_best_batch_dev (1 pattern, k = 2) + bg_fastq_trim_dev 3' (the adapter trim)", 2 * N * L + 64 * N,
     lambda: (myers.best_batch_dev(pats, d_seq, d_so, K, stream=stream, out=hits),
              myers.trim_dev(myers.TRIM_3P, hits[0], 1, N, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream, want_totals=False, out=atrim))),
    ("filter", "bg_fastq_filter_dev max_n 5 (counts N in the sequence column; no totals)", 56 * (N + kept) + 2 * 8 * (N + kept) + N * L + 2 * (f_sb + f_qb),
     lambda: fastq.filter_dev(N, d_recs, d_seq, d_so, d_qual, d_qo, max_n=5, stream=stream, want_totals=False, out=flt)),
    ("copy", "device-to-device copy of the quality column", 2 * N * L, lambda: q_copy.copy_(d_qual[:N * L])),
    ("cut", "bg_fastq_qual_cut_dev, RUNSUM at both ends", qcol + 64 * N, lambda: fastq.qual_cut_dev(N, d_qual, d_qo, stream=stream, out=cut, **both)),
    ("cut_win", "bg_fastq_qual_cut_dev, RUNSUM 5' and WINDOW 4 at the 3' end", qcol + 64 * N,
     lambda: fastq.qual_cut_dev(N, d_qual, d_qo, stream=stream, out=cut_w, **win)),
    ("select", "bg_fastq_qual_select_dev, no weight table", qcol + 36 * N, lambda: fastq.qual_select_dev(N, d_qual, d_qo, stream=stream, out=sel, **sp)),
    ("select_w", "bg_fastq_qual_select_dev, expected-error table", qcol + 36 * N,
     lambda: fastq.qual_select_dev(N, d_qual, d_qo, weight=weight, max_weight=2 << 20, stream=stream, out=sel_w, **sp)),
    ("tab150", "bg_fastq_qc_tables_dev, max_cycles 150", 2 * qcol, lambda: fastq.qc_tables_dev(N, d_seq, d_so, d_qual, d_qo, 150, stream=stream, out=tab150.buf)),
    ("tab1024", "bg_fastq_qc_tables_dev, max_cycles 1024", 2 * qcol,
     lambda: fastq.qc_tables_dev(N, d_seq, d_so, d_qual, d_qo, 1024, stream=stream, out=tab1024.buf)),
    ("cut_trim", "cut (RUNSUM both ends) + bg_fastq_trim_dev 3' + 5' (no totals)", qcol + 64 * N + 2 * (2 * 64 * N + 2 * 56 * N + 4 * 8 * N + 4 * N * L),
     cut_and_trims),
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
    say("%-92s median %8.3f ms (min %.3f max %.3f)  %7.1f M reads/s  %7.1f MB algorithmic, %6.1f GB/s" % (
        name, m, t[0], t[-1], N / m / 1e3, nbytes / 1e6, nbytes / m / 1e6))
say("cut: %d of %d reads cut, %d of %d symbols removed (WINDOW: %d reads, %d symbols); select: %d pass without the table, %d with it" % (
    cut_tot[0], N, cut_tot[1], N * L, cut_w_tot[0], cut_w_tot[1], sel[2], sel_w[2]))
for key in ("cut", "cut_win", "select", "select_w"):
    say("%-9s / copy of the quality column %.2f, / filter with max_n %.2f" % (key, med[key] / med["copy"], med[key] / med["filter"]))
for key in ("tab150", "tab1024"):
    say("%-9s / ingest %.2f" % (key, med[key] / med["parse"]))
say("cut + trim 3' + trim 5' / adapter trim %.2f" % (med["cut_trim"] / med["adapter"]))
say("not measured: the host-buffer flavours, the paired select, reads longer than 150 symbols, calls that ask for host totals")
if len(sys.argv) > 3:
    open(sys.argv[3], "w").write("tools/exp/time_fastq_qual.py %d %d on one MI355X, device-resident: every call once per round between two "
                                 "device events, %d rounds after 2 warm-up rounds, medians\n" % (N, REPEATS, REPEATS) + "\n".join(lines) + "\n")
