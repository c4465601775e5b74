"""Device-resident timing of the FASTA ingest next to the FASTQ ingest, in one process (python tools/exp/time_fasta.py [GB] [OUT]):
  * bg_fasta_parse_dev and bg_fasta_reference_dev (forward text, and FMD | UPPER) on GB (default 1) gigabytes of 60-column FASTA
    with 24 records, and on as much transcriptome-like FASTA (records of 0.3 - 3 kbp);
  * bg_fastq_parse_dev on as much FASTQ (150 bp reads), the project's established single-pass ingest, as the yardstick.
Per call: 3 warm-up calls, then the median and spread of 10 timed with device events around the call (the parse calls end with
a host synchronisation, so the events bracket the whole call).  Prints GB/s of input text and the FASTA / FASTQ ratios; with OUT
also writes them there."""
import ctypes as C
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from rust_bio_amd import _lib, fasta, fastq, synth  # noqa: E402

GB = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
TARGET = int(GB * 1e9)
rng = np.random.default_rng(5)


def lines60(n_bases):
    rows = n_bases // 60
    a = np.empty((rows, 61), dtype=np.uint8)
    a[:, :60] = rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), size=(rows, 60), p=[.2, .2, .2, .2, .05, .05, .05, .05])
    a[:, 60] = 10
    return a.tobytes()


def genome_text():
    block = lines60(TARGET // 24 // 61 * 60)
    return b"".join(b">chr%d assembled-molecule\n" % (k + 1) + block for k in range(24))


def transcriptome_text():
    unit = b"".join(b">ENST%08d.%d gene=G%d len=%d\n" % (k, k % 9, k // 3, n) + lines60(n) + b"ACGTTGCA\n"
                    for k, n in enumerate(rng.integers(300, 3000, size=4000)))
    return unit * max(1, TARGET // len(unit))


def fastq_text():
    unit = synth.fastq_text(20000, 150, seed=3).tobytes()
    return unit * max(1, TARGET // len(unit))


def timed(f, n=10, warm=3):
    for _ in range(warm):
        f()
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


out = []


def report(name, nbytes, t):
    med, lo, hi = t
    out.append((name, nbytes / med / 1e6))
    print("%-34s %8.1f MB  median %8.3f ms (min %.3f max %.3f)  %7.1f GB/s" % (name, nbytes / 1e6, med, lo, hi, nbytes / med / 1e6), flush=True)


stream = torch.cuda.current_stream().cuda_stream
for label, make in (("fasta genome (24 records, 60 col)", genome_text), ("fasta transcriptome (0.3-3 kbp)", transcriptome_text)):
    host = make()
    n_hdr = host.count(b"\n>") + 1
    d_text = torch.from_numpy(np.frombuffer(host, np.uint8).copy()).cuda()
    del host
    bufs = fasta.alloc_dev(d_text.numel(), d_text.device, n_hdr)
    n, status, _, d_recs, d_seq, _ = fasta.parse_dev(d_text, bufs=bufs, rec_cap=n_hdr, stream=stream)
    assert (n, status) == (n_hdr, "ok")
    report(label + ": parse", d_text.numel(), timed(lambda: fasta.parse_dev(d_text, bufs=bufs, rec_cap=n_hdr, stream=stream)))
    for fl, nm in ((0, "reference"), (fasta.REF_FMD | fasta.REF_UPPER, "reference FMD|UPPER")):
        d_ref, d_contigs, d_names, _ = fasta.reference_dev(n, d_recs, d_text, d_seq, fl, stream=stream)
        nt, nb, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

        def build():
            _lib.check(_lib.lib().bg_fasta_reference_dev(_lib.default_context().h, n, d_recs.data_ptr(), d_text.data_ptr(), d_seq.data_ptr(), fl,
                                                         d_ref.data_ptr(), d_ref.numel(), d_contigs.data_ptr(), d_names.data_ptr(), d_names.numel(),
                                                         C.byref(nt), C.byref(nb), C.byref(bad), stream))
        report(label + ": " + nm, d_ref.numel(), timed(build))
        del d_ref
    del d_text, bufs, d_recs, d_seq
    torch.cuda.empty_cache()
host = fastq_text()
d_text = torch.from_numpy(np.frombuffer(host, np.uint8).copy()).cuda()
del host
bufs = fastq.alloc_dev(d_text.numel(), d_text.device)
report("fastq 150 bp: parse", d_text.numel(), timed(lambda: fastq.parse_dev(d_text, bufs=bufs, stream=stream)))
fq = out[-1][1]
lines = ["%s: %.1f GB/s (%.2f x the FASTQ parse)" % (nm, v, v / fq) for nm, v in out]
print("\n".join(lines))
if len(sys.argv) > 2:
    open(sys.argv[2], "w").write("tools/exp/time_fasta.py %g on one MI355X, device-resident, median of 10 calls after 3 warm-up calls; GB/s of the call's input "
                                 "text (parse) or output text (reference)\n" % GB + "\n".join(lines) + "\n")
