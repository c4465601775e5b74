"""Device-resident timing of the Myers calls and the trim next to the FASTQ ingest, in one process
(python tools/exp/myers_timing.py [READS] [OUT]; through tools/exp/run.sh: py:tools/exp/myers_timing.py:1000000,OUT):
  * READS (default 1 M) reads of 150 bp generated as bench.py's FASTQ leg generates them (synth.fastq_text), 30 % of them
    carrying a 3' copy of a 33-symbol adapter with 0 to 2 edits, parsed on the device;
  * one pattern and four patterns, max_dist = 3: bg_myers_best_batch_dev (coordinates only, and with operations),
    bg_myers_find_all_batch_dev (ENDS_ONLY, and with starts; max_hits 4), bg_fastq_trim_dev (3', without totals);
  * bg_fastq_parse_dev of the same reads as the yardstick.
Per call: 3 warm-up calls, then the median and spread of 10 timed with device events; the outputs are allocated once, outside
the timed calls (what stays inside a Myers call besides its kernels is the host's compaction of the peq tables into byte classes).  Algorithmic bytes of a Myers call: the
sequences once per pattern group + 8 bytes of offsets per read + 64 per record (+ the operations written); of the trim: hits and
records read, records written, sequences and qualities read and written once.  Fractions are of the 6.29 TB/s copy bandwidth
measured on this part (DESIGN.md 4.7 and bench.py's HBM_PEAK_GBS comment; 8 TB/s specified)."""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from rust_bio_amd import fastq, myers, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
L, K, COPY_GBS = 150, 3, 6290.0
ADAPTERS = [b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT", b"CTGTCTCTTATACACATCTCCGAGCCCACGAGA",
            b"CTGTCTCTTATACACATCTGACGCTGCCGACGA"]
rng = np.random.default_rng(9)


def reads_text():
    """synth.fastq_text with the tail of 30 % of the reads overwritten by (a prefix of) the first adapter with 0 - 2 substitutions"""
    text = synth.fastq_text(N, L, seed=6).copy()
    rec = len(text) // N
    rows = text.reshape(N, rec)
    o = int(np.nonzero(rows[0] == 10)[0][0]) + 1
    ad = np.frombuffer(ADAPTERS[0], np.uint8)
    with_ad = np.nonzero(rng.random(N) < 0.3)[0]
    keep = rng.integers(40, L - len(ad) + 1, size=len(with_ad))  # insert lengths: the adapter is whole
    for r, ins in zip(with_ad, keep):
        a = ad.copy()
        for _ in range(int(rng.integers(0, 3))):
            a[int(rng.integers(0, len(a)))] = ord("ACGT"[int(rng.integers(0, 4))])
        rows[r, o + ins:o + ins + len(a)] = a
    return text, len(with_ad)


def timed(f, n=10, warm=3):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


lines = []


def report(name, nbytes, t, base=None):
    med, lo, hi = t
    gbs = nbytes / med / 1e6
    s = "%-44s median %8.3f ms (min %.3f max %.3f)  %6.1f M reads/s  %7.1f MB algorithmic, %6.1f GB/s = %.3f of copy" % (
        name, med, lo, hi, N / med / 1e3, nbytes / 1e6, gbs, gbs / COPY_GBS)
    if base:
        s += "  %.2f x the parse" % (med / base)
    lines.append(s)
    print(s, flush=True)
    return med


text, n_ad = reads_text()
stream = torch.cuda.current_stream().cuda_stream
d_fq = torch.from_numpy(text).cuda()
bufs = fastq.alloc_dev(d_fq.numel(), d_fq.device)
n, status, _, d_recs, d_seq, d_so, d_qual, d_qo = fastq.parse_dev(d_fq, bufs=bufs, stream=stream)
assert (n, status) == (N, "ok")
parse_ms = report("bg_fastq_parse_dev (yardstick)", d_fq.numel(), timed(lambda: fastq.parse_dev(d_fq, bufs=bufs, stream=stream)))
seq_bytes = N * L
for n_pat in (1, 4):
    pats = [myers.Myers(a) for a in ADAPTERS[:n_pat]]
    jobs = N * n_pat
    base = seq_bytes + 8 * N + 64 * jobs  # one pattern group: the text once
    d_hits, _ = myers.best_batch_dev(pats, d_seq, d_so, K, stream=stream)
    hits = myers.records(d_hits)
    found = int((hits["score"] != myers.MIN_SCORE).sum())
    tag = "%d pattern%s: " % (n_pat, "s" if n_pat > 1 else "")
    lines.append("%s%d of %d jobs have a hit (%d reads carry the first adapter)" % (tag, found, jobs, n_ad))
    print(lines[-1], flush=True)
    o = (d_hits, None)
    report(tag + "best, coordinates only", base, timed(lambda: myers.best_batch_dev(pats, d_seq, d_so, K, stream=stream, out=o)), parse_ms)
    n_ops = int(hits["n_ops"].sum())
    o = myers.best_batch_dev(pats, d_seq, d_so, K, ops_stride=66, stream=stream)
    report(tag + "best, with operations (stride 66)", base + n_ops,
           timed(lambda: myers.best_batch_dev(pats, d_seq, d_so, K, ops_stride=66, stream=stream, out=o)), parse_ms)
    o = myers.find_all_batch_dev(pats, d_seq, d_so, K, 4, True, stream=stream)
    report(tag + "find_all ENDS_ONLY (max_hits 4)", seq_bytes + 8 * N + (4 * 64 + 4) * jobs,
           timed(lambda: myers.find_all_batch_dev(pats, d_seq, d_so, K, 4, True, stream=stream, out=o)), parse_ms)
    report(tag + "find_all with starts (max_hits 4)", seq_bytes + 8 * N + (4 * 64 + 4) * jobs,
           timed(lambda: myers.find_all_batch_dev(pats, d_seq, d_so, K, 4, False, stream=stream, out=o)), parse_ms)
    o = myers.trim_dev(myers.TRIM_3P, d_hits, n_pat, N, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream)
    kept = o[5][0]
    report(tag + "bg_fastq_trim_dev 3' (no totals)", 64 * jobs + 2 * 56 * N + 4 * 8 * N + 2 * (seq_bytes + kept),
           timed(lambda: myers.trim_dev(myers.TRIM_3P, d_hits, n_pat, N, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream, want_totals=False,
                                        out=o)), parse_ms)
    del o
    lines.append("%strim keeps %d of %d bases" % (tag, kept, seq_bytes))
    print(lines[-1], flush=True)
if len(sys.argv) > 2:
    open(sys.argv[2], "w").write("tools/exp/myers_timing.py %d on one MI355X, device-resident, max_dist %d, median of 10 calls after 3 warm-up calls "
                                 "(device events around the call; outputs allocated beforehand)\n" % (N, K) + "\n".join(lines) + "\n")
