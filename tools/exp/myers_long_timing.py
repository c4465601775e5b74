"""Device-resident timing of the block-based Myers calls (csrc/myers_long.hip) next to the u64 calls, in one process
(python tools/exp/myers_long_timing.py [READS] [OUT]; through tools/exp/run.sh: py:tools/exp/myers_long_timing.py:1000000,OUT).
The workload of tools/exp/myers_timing.py: READS (default 1 M) reads of 150 bp (synth.fastq_text), 30 % of them carrying a 3'
copy of the adapter with 0 to 2 substitutions, parsed on the device; median of 10 calls after 3 warm-up calls, device events
around the call, outputs allocated beforehand.
  * m = 33 and m = 64 through bg_myers_long_*_batch_dev against bg_myers_*_batch_dev, same process, same texts, max_dist 3:
    what the block machinery costs at one block;
  * m = 66, 130, 300 (2, 3, 5 blocks; the last in the 8-block kernels) at max_dist 3 and m / 10: best (coordinates only),
    find_all ENDS_ONLY, find_all with starts (max_hits 4), and best + bg_fastq_trim_dev.  An adapter longer than the room
    behind a 20-base insert is cut at the read's end (m = 300: 130 of its symbols, so nothing is within m / 10).
"per block" is the call's time divided by its pattern's block count and by the u64 call's time for the 33-symbol adapter (same
kind of call, one block).  Algorithmic bytes and the copy bandwidth as in profiles/myers_timing.txt."""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from rust_bio_amd import fastq, myers, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
L, COPY_GBS = 150, 6290.0
rng = np.random.default_rng(9)
STEM = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"  # the 33 symbols of myers_timing.py
TEXT = synth.fastq_text(N, L, seed=6)
lines = []


def adapter(m):
    return (STEM + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=max(0, m - len(STEM)))))[:m] if m != 33 else STEM


def reads_with(ad):
    """the reads with the tail of 30 % of them overwritten by the adapter (cut at the read's end) with 0 - 2 substitutions"""
    text = TEXT.copy()
    rows = text.reshape(N, len(text) // N)
    o = int(np.nonzero(rows[0] == 10)[0][0]) + 1
    a = np.frombuffer(ad, np.uint8)
    with_ad = np.nonzero(rng.random(N) < 0.3)[0]
    whole = min(len(a), L - 20)
    ins = rng.integers(20, L - whole + 1, size=len(with_ad))
    copies = np.tile(a[:L - 20], (len(with_ad), 1))
    for e in range(2):  # the e-th substitution in a third / two thirds of the copies
        sel = np.nonzero(rng.integers(0, 3, size=len(with_ad)) > e)[0]
        copies[sel, rng.integers(0, whole, size=len(sel))] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=len(sel))]
    col = ins[:, None] + np.arange(copies.shape[1])[None, :]
    ok = col < L
    rows[np.repeat(with_ad, ok.sum(axis=1)), o + col[ok]] = copies[ok]
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


def say(s):
    lines.append(s)
    print(s, flush=True)


def report(name, nbytes, t, blocks=None, base=None):
    med, lo, hi = t
    gbs = nbytes / med / 1e6
    s = "%-50s median %8.3f ms (min %.3f max %.3f)  %6.1f M reads/s  %6.1f GB/s = %.3f of copy" % (
        name, med, lo, hi, N / med / 1e3, gbs, gbs / COPY_GBS)
    if base:
        s += "  %.2f x u64 m=33, %.2f per block" % (med / base, med / base / blocks)
    say(s)
    return med


stream = torch.cuda.current_stream().cuda_stream
seq_bytes = N * L
B_BEST, B_ALL = seq_bytes + 8 * N + 64 * N, seq_bytes + 8 * N + (4 * 64 + 4) * N
KINDS = ["best", "ends", "all", "best+trim"]


def calls(best, find_all, pats, k, parsed):
    """the four timed calls for one pattern set: {kind: (median, min, max)}"""
    _, d_recs, d_seq, d_so, d_qual, d_qo = parsed
    d_hits, _ = best(pats, d_seq, d_so, k, stream=stream)
    found = int((myers.records(d_hits)["score"] != myers.MIN_SCORE).sum())
    ob = (d_hits, None)
    oe = find_all(pats, d_seq, d_so, k, 4, True, stream=stream)
    ot = myers.trim_dev(myers.TRIM_3P, d_hits, 1, N, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream)

    def best_trim():
        best(pats, d_seq, d_so, k, stream=stream, out=ob)
        myers.trim_dev(myers.TRIM_3P, d_hits, 1, N, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream, want_totals=False, out=ot)

    return found, {"best": timed(lambda: best(pats, d_seq, d_so, k, stream=stream, out=ob)),
                   "ends": timed(lambda: find_all(pats, d_seq, d_so, k, 4, True, stream=stream, out=oe)),
                   "all": timed(lambda: find_all(pats, d_seq, d_so, k, 4, False, stream=stream, out=oe)),
                   "best+trim": timed(best_trim)}


def parse(text):
    d_fq = torch.from_numpy(text).cuda()
    n, status, _, d_recs, d_seq, d_so, d_qual, d_qo = fastq.parse_dev(d_fq, stream=stream)
    assert (n, status) == (N, "ok")
    return d_fq, d_recs, d_seq, d_so, d_qual, d_qo


NAMES = {"best": "best, coordinates only", "ends": "find_all ENDS_ONLY (max_hits 4)", "all": "find_all with starts (max_hits 4)",
         "best+trim": "best + bg_fastq_trim_dev 3' (no totals)"}
BYTES = {"best": B_BEST, "ends": B_ALL, "all": B_ALL, "best+trim": B_BEST + 64 * N + 2 * 56 * N + 4 * 8 * N + 4 * seq_bytes}
base = {}
for m in (33, 64):
    ad = adapter(m)
    text, n_ad = reads_with(ad)
    parsed = parse(text)
    found, t64 = calls(myers.best_batch_dev, myers.find_all_batch_dev, [myers.Myers(ad)], 3, parsed)
    found_l, tl = calls(myers.long_best_batch_dev, myers.long_find_all_batch_dev, [myers.MyersLong(ad)], 3, parsed)
    assert found == found_l
    say("m = %d, max_dist 3: %d of %d reads have a hit (%d carry the adapter)" % (m, found, N, n_ad))
    if m == 33:
        base = {kind: t64[kind][0] for kind in KINDS}
    for kind in KINDS:
        report("m=%d u64  %s" % (m, NAMES[kind]), BYTES[kind], t64[kind], 1, base[kind])
        report("m=%d long %s" % (m, NAMES[kind]), BYTES[kind], tl[kind], 1, base[kind])
    del parsed
for m in (66, 130, 300):
    ad = adapter(m)
    text, n_ad = reads_with(ad)
    parsed = parse(text)
    for k in (3, m // 10):
        found, t = calls(myers.long_best_batch_dev, myers.long_find_all_batch_dev, [myers.MyersLong(ad)], k, parsed)
        say("m = %d (%d blocks), max_dist %d: %d of %d reads have a hit (%d carry the adapter)" % (m, (m + 63) // 64, k, found, N, n_ad))
        for kind in KINDS:
            report("m=%d k=%d long %s" % (m, k, NAMES[kind]), BYTES[kind], t[kind], (m + 63) // 64, base[kind])
    del parsed
if len(sys.argv) > 2:
    open(sys.argv[2], "w").write("tools/exp/myers_long_timing.py %d on one MI355X, device-resident, median of 10 calls after 3 warm-up calls "
                                 "(device events around the call; outputs allocated beforehand)\n" % N + "\n".join(lines) + "\n")
