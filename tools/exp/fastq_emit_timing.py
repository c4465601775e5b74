"""Device-resident timing of the FASTQ filter and writer next to the FASTQ ingest and the trim, in one process
(python tools/exp/fastq_emit_timing.py [READS] [OUT]; through tools/exp/run.sh: py:tools/exp/fastq_emit_timing.py:1000000,OUT):
  * READS (default 1 M) reads of 150 bp generated as bench.py's FASTQ leg generates them (synth.fastq_text), 30 % of them
    carrying a 3' copy of a 33-symbol adapter with 0 to 2 edits (tools/exp/myers_timing.py's reads), parsed on the device;
  * bg_fastq_parse_dev and bg_fastq_trim_dev (3', one pattern, without totals) as the yardsticks;
  * bg_fastq_filter_dev with min_len only and with max_n (without totals), on the parsed and on the trimmed records;
  * bg_fastq_emit_dev with step 1, and with step 2 twice (an R1 and an R2 text), into buffers allocated beforehand, under each
    flavour of the text pass (fq_emit_mode 1, 2) — the call includes its length pass, its scan and the one read-back;
  * the chain parse -> best -> trim -> filter (PAIRED, min_len 20) -> emit twice.
Per call: 3 warm-up calls, then the median and spread of 10 timed with device events.  Algorithmic bytes of the filter: records
read and written, offsets read and written, the kept sequences and qualities read and written (the sequences once more with
max_n); of the writer: 56 bytes of record and 8 of offset per line, and every byte of text once read and once written.
Fractions are of the 6.29 TB/s copy bandwidth measured on this part."""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from rust_bio_amd import _lib, fastq, myers, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
L, K, COPY_GBS = 150, 3, 6290.0
ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
rng = np.random.default_rng(9)


def reads_text():
    """synth.fastq_text with the tail of 30 % of the reads overwritten by the adapter with 0 - 2 substitutions"""
    text = synth.fastq_text(N, L, seed=6).copy()
    rec = len(text) // N
    rows = text.reshape(N, rec)
    o = int(np.nonzero(rows[0] == 10)[0][0]) + 1
    ad = np.frombuffer(ADAPTER, np.uint8)
    with_ad = np.nonzero(rng.random(N) < 0.3)[0]
    keep = rng.integers(10, L - len(ad) + 1, size=len(with_ad))
    for r, ins in zip(with_ad, keep):
        a = ad.copy()
        for _ in range(int(rng.integers(0, 3))):
            a[int(rng.integers(0, len(a)))] = ord("ACGT"[int(rng.integers(0, 4))])
        rows[r, o + ins:o + ins + len(a)] = a
    return text


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


def say(s):
    lines.append(s)
    print(s, flush=True)


def report(name, nbytes, t, base=None):
    med, lo, hi = t
    gbs = nbytes / med / 1e6
    s = "%-58s median %8.3f ms (min %.3f max %.3f)  %6.1f M reads/s  %7.1f MB algorithmic, %6.1f GB/s = %.3f of copy" % (
        name, med, lo, hi, N / med / 1e3, nbytes / 1e6, gbs, gbs / COPY_GBS)
    if base:
        s += "  %.2f x the parse" % (med / base)
    say(s)
    return med


ctx = _lib.default_context()
stream = torch.cuda.current_stream().cuda_stream
d_fq = torch.from_numpy(reads_text()).cuda()
bufs = fastq.alloc_dev(d_fq.numel(), d_fq.device)
n, status, _, d_recs, d_seq, d_so, d_qual, d_qo = fastq.parse_dev(d_fq, bufs=bufs, stream=stream)
assert (n, status) == (N, "ok")
parse_ms = report("bg_fastq_parse_dev (yardstick)", d_fq.numel(), timed(lambda: fastq.parse_dev(d_fq, bufs=bufs, stream=stream)))
pats = [myers.Myers(ADAPTER)]
d_hits, _ = myers.best_batch_dev(pats, d_seq, d_so, K, stream=stream)
best_ms = report("bg_myers_best_batch_dev, 1 pattern, coordinates only", N * L + 8 * N + 64 * N,
                 timed(lambda: myers.best_batch_dev(pats, d_seq, d_so, K, stream=stream, out=(d_hits, None))), parse_ms)
trim = myers.trim_dev(myers.TRIM_3P, d_hits, 1, N, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream)
t_recs, t_seq, t_so, t_qual, t_qo, (t_sb, t_qb) = trim
trim_bytes = 64 * N + 2 * 56 * N + 4 * 8 * N + 2 * (N * L + t_sb)
trim_ms = report("bg_fastq_trim_dev 3' (yardstick; no totals)", trim_bytes,
                 timed(lambda: myers.trim_dev(myers.TRIM_3P, d_hits, 1, N, d_recs, d_seq, d_so, d_qual, d_qo, stream=stream, want_totals=False,
                                              out=trim)), parse_ms)
say("the trim keeps %d of %d bases; its copy moves %.1f MB of sequences and qualities: %.1f GB/s of them" % (
    t_sb, N * L, 2 * (t_sb + t_qb) / 1e6, 2 * (t_sb + t_qb) / trim_ms / 1e6))

for tag, cols in (("parsed: ", (d_recs, d_seq, d_so, d_qual, d_qo)), ("trimmed: ", (t_recs, t_seq, t_so, t_qual, t_qo))):
    for name, kw in (("min_len 20", dict(min_len=20)), ("min_len 20, max_n 2", dict(min_len=20, max_n=2)),
                     ("PAIRED, min_len 20", dict(flags=fastq.FQF_PAIRED, min_len=20))):
        res = fastq.filter_dev(N, *cols, stream=stream, **kw)
        k, sb, qb = res[6]
        out = fastq.filter_dev(N, *cols, stream=stream, want_totals=False, **kw)
        nbytes = 56 * (N + k) + 2 * 8 * (N + k) + 2 * (sb + qb) + (sb if "max_n" in kw else 0)
        report(tag + "bg_fastq_filter_dev %s (keeps %d; no totals)" % (name, k), nbytes,
               timed(lambda: fastq.filter_dev(N, *cols, stream=stream, want_totals=False, out=out, **kw)), parse_ms)
        del res, out

MODE = {1: "byte stores", 2: "staged in LDS, 16-byte stores"}
for tag, (recs, seq, qual) in (("parsed: ", (d_recs, d_seq, d_qual)), ("trimmed: ", (t_recs, t_seq, t_qual))):
    for mode in (1, 2):
        ctx.set_option("fq_emit_mode", mode)
        d_out, d_off, total = fastq.emit_dev(N, d_fq, recs, seq, qual, stream=stream)
        report(tag + "bg_fastq_emit_dev step 1 (%s)" % MODE[mode], 2 * total + 64 * N,
               timed(lambda: fastq.emit_dev(N, d_fq, recs, seq, qual, stream=stream, out=(d_out, d_off))), parse_ms)
        o1 = fastq.emit_dev(N, d_fq, recs, seq, qual, 0, 2, stream=stream)
        o2 = fastq.emit_dev(N, d_fq, recs, seq, qual, 1, 2, stream=stream)

        def twice():
            fastq.emit_dev(N, d_fq, recs, seq, qual, 0, 2, stream=stream, out=o1[:2])
            fastq.emit_dev(N, d_fq, recs, seq, qual, 1, 2, stream=stream, out=o2[:2])

        report(tag + "bg_fastq_emit_dev step 2, twice (%s)" % MODE[mode], 2 * (o1[2] + o2[2]) + 64 * N, timed(twice), parse_ms)
        del d_out, d_off, o1, o2
    ctx.set_option("fq_emit_mode", 0)
d_out, d_off, total = fastq.emit_dev(N, d_fq, d_recs, d_seq, d_qual, stream=stream)
say("the text pass alone moves %.1f MB read + %.1f MB written per step-1 call of the parsed records" % (total / 1e6, total / 1e6))
del d_out, d_off


def chain():
    k, st, _, recs, seq, so, qual, qo = fastq.parse_dev(d_fq, bufs=bufs, stream=stream)
    myers.best_batch_dev(pats, seq, so, K, stream=stream, out=(d_hits, None))
    t = myers.trim_dev(myers.TRIM_3P, d_hits, 1, k, recs, seq, so, qual, qo, stream=stream, want_totals=False, out=trim)
    f = fastq.filter_dev(k, *t[:5], flags=fastq.FQF_PAIRED, min_len=20, stream=stream)
    kept = f[6][0]
    a = fastq.emit_dev(kept, d_fq, f[0], f[1], f[3], 0, 2, stream=stream)
    b = fastq.emit_dev(kept, d_fq, f[0], f[1], f[3], 1, 2, stream=stream)
    return kept, a[2], b[2]


kept, b1, b2 = chain()
report("chain parse -> best -> trim -> filter -> emit x 2 (allocating)", d_fq.numel() + b1 + b2, timed(lambda: chain()), parse_ms)
say("the chain keeps %d of %d reads and writes %.1f + %.1f MB of FASTQ" % (kept, N, b1 / 1e6, b2 / 1e6))
if len(sys.argv) > 2:
    open(sys.argv[2], "w").write("tools/exp/fastq_emit_timing.py %d on one MI355X, device-resident, median of 10 calls after 3 warm-up calls "
                                 "(device events around the call)\n" % N + "\n".join(lines) + "\n")
