"""Quality preprocessing end to end, nothing but totals and the split's group offsets crossing to the host in between:
interleaved paired FASTQ text -> bg_fastq_parse_dev -> bg_myers_best_batch_dev (one adapter, k = 2) -> bg_fastq_trim_dev at the
3' end -> bg_fastq_qual_cut_dev (running sum at both ends) -> bg_fastq_trim_dev at the 3' and then at the 5' end with the cut
records -> bg_fastq_filter_dev (min_len 1, pairs together) -> bg_fastq_qual_select_dev (mean quality, share of low symbols,
expected errors; pairs together) -> bg_fastq_demux_split_dev with one bin -> bg_fastq_emit_dev twice (R1 and R2), ONE call each
for the passed and the failed records.  The four texts are compared with what the Python restatements write: the quality rules
(tests/fastq_qual_oracle.py), the trim rule (tests/myers_oracle.py) and `Writer::write` (tests/fastq_write_oracle.py); the
per-cycle tables before and after trimming with the restatement's.  The Myers records the chain starts from are the device's,
downloaded after the last call (that call has its own tests)."""
import random

import numpy as np
import pytest
import torch

import fastq_qual_oracle as qo
import fastq_write_oracle as fw
import myers_oracle as mo
from fastq_qual_cases import CUTOFF, PHRED, qual_string
from fastq_write_cases import Batch
from myers_cases import dna
from rust_bio_amd import fastq, myers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, K = 2000, 2
ADAPTER = b"AGATCGGAAGAGCACACG"


def make_reads(seed=41):
    """N interleaved mates of 30 .. 150 bases; a third run into the adapter; the qualities of a mate are mostly
    good with a bad tail, mixed, or bad throughout"""
    rng = random.Random(seed)
    out = []
    for q in range(N // 2):
        for mate in (1, 2):
            s = dna(rng, rng.randint(30, 150))
            if rng.random() < 0.33:
                s = s[:rng.randint(1, len(s))] + ADAPTER + dna(rng, rng.randint(0, 5))
            kind = rng.random()
            if kind < 0.7:
                tail = rng.randint(0, 25)
                qual = qual_string(rng, len(s) - min(tail, len(s)), 0.03) + qual_string(rng, min(tail, len(s)), 0.97)
            else:
                qual = qual_string(rng, len(s), 0.4 if kind < 0.92 else 0.97)
            out.append((b"pair%d" % q, b"%d:N:0" % mate, s, qual))
    return out


def test_trim_cut_filter_select_and_write_paired_reads():
    reads = make_reads()
    fq = b"".join(fw.write(*r) for r in reads)
    st = torch.cuda.current_stream().cuda_stream
    cp = dict(method_5p=fastq.QCUT_RUNSUM, method_3p=fastq.QCUT_RUNSUM, cutoff_5p=CUTOFF, cutoff_3p=CUTOFF, phred_offset=PHRED)
    sp = dict(flags=fastq.QSEL_PAIRED, min_mean_q=25, low_q=15, max_low_pct=20, phred_offset=PHRED)
    max_ee = 2.0
    d_fq = torch.frombuffer(bytearray(fq), dtype=torch.uint8).to(DEV)
    n, status, _, d_recs, d_seq, d_so, d_qual, d_qo = fastq.parse_dev(d_fq, stream=st)
    assert (n, status) == (N, "ok")
    tab_before = fastq.qc_tables_dev(n, d_seq, d_so, d_qual, d_qo, 150, 0, 2, PHRED, stream=st)
    d_hits, _ = myers.best_batch_dev([myers.Myers(ADAPTER)], d_seq, d_so, K, stream=st)
    a = myers.trim_dev(myers.TRIM_3P, d_hits, 1, n, d_recs, d_seq, d_so, d_qual, d_qo, stream=st, want_totals=False)
    d_cut, cut_tot = fastq.qual_cut_dev(n, a[3], a[4], stream=st, want_totals=True, **cp)
    t3 = myers.trim_dev(myers.TRIM_3P, d_cut, 1, n, *a[:5], stream=st, want_totals=False)
    t5 = myers.trim_dev(myers.TRIM_5P, d_cut, 1, n, *t3[:5], stream=st, want_totals=False)
    tab_after = [fastq.qc_tables_dev(n, t5[1], t5[2], t5[3], t5[4], 100, first, 2, PHRED, stream=st) for first in (0, 1)]
    f = fastq.filter_dev(n, *t5[:5], flags=fastq.FQF_PAIRED, min_len=1, stream=st)
    k = f[6][0]
    _, d_bin, passed = fastq.qual_select_dev(k, f[3], f[4], max_ee=max_ee, stream=st, want_stats=False, want_totals=True, **sp)
    s = fastq.demux_split_dev(k, d_bin, 1, *f[:5], stream=st)
    bin_off = s[8]
    texts = []
    for first in (0, 1):
        d_out, d_off, _ = fastq.emit_dev(k, d_fq, s[0], s[1], s[3], first, 2, stream=st)
        texts.append([t.cpu().numpy().tobytes() for t in fastq.demux_texts(d_out, d_off, bin_off, 1, first, 2)])
    torch.cuda.synchronize()

    # the same on the restatements, from the device's Myers records
    hits = myers.records(d_hits)
    clipped = []
    for r, (id_, desc, sq, ql) in enumerate(reads):
        (lo, hi), (qlo, qhi) = mo.trim_range(mo.TRIM_3P, [(int(hits[r]["score"]), int(hits[r]["ystart"]), int(hits[r]["yend"]))], len(sq), len(ql))
        clipped.append((id_, desc, sq[lo:hi], ql[qlo:qhi]))
    assert 400 < sum(len(c[2]) < len(r[2]) for c, r in zip(clipped, reads)) < 1000
    cb = Batch(clipped)
    seen = {}
    w_cut, w_cut_tot, points = qo.cut(cb.qual, cb.qual_off, PHRED, events=seen, method_5p=qo.RUNSUM, method_3p=qo.RUNSUM, cutoff_5p=CUTOFF,
                                      cutoff_3p=CUTOFF)
    assert d_cut.cpu().numpy().tobytes() == w_cut.tobytes() and cut_tot == w_cut_tot
    assert min(seen.get(key, 0) for key in ("no-hit", "3p", "5p", "both", "nothing left")) >= 20, seen
    trimmed = qo.trimmed(clipped, w_cut)
    assert trimmed == [(i, d, sq[b:e], ql[b:e]) for (i, d, sq, ql), (b, e) in zip(clipped, points)]
    kept = [r for r in range(N) if len(trimmed[r][2]) >= 1 and len(trimmed[r ^ 1][2]) >= 1]
    assert k == len(kept) and 40 <= N - k < N // 2 and k % 2 == 0
    kb = Batch([trimmed[r] for r in kept])
    _, w_bin, w_pass = qo.select(kb.qual, kb.qual_off, flags=qo.PAIRED, phred_offset=PHRED, min_mean_q=25, low_q=15, max_low_pct=20,
                                 max_weight=int(round(max_ee * 2 ** 20)), weight=qo.ee_weights(PHRED))
    assert (d_bin.cpu().numpy().view(np.uint32) == w_bin).all() and passed == w_pass and k // 5 < w_pass < k - k // 5
    assert (w_bin[0::2] == w_bin[1::2]).all() and list(bin_off) == [0, w_pass, k, k]
    groups = [[kb.records[r] for r in range(k) if w_bin[r] == g] for g in (0, 1)]
    for g in (0, 1):
        for first in (0, 1):
            assert texts[first][g] == b"".join(fw.write(*w) for w in groups[g][first::2]), (g, first)
    assert texts[0][2] == b"" and texts[1][2] == b""
    # the passed text parses back: what the next tool would read
    for first in (0, 1):
        p = fastq.parse_arrays(texts[first][0])
        assert p.status == "ok" and len(p) == w_pass // 2
        got = [p.record(i) for i in range(len(p))]
        assert [(x._id, x._desc, x._seq, x._qual) for x in got] == groups[0][first::2]

    # the tables: mate 1 of the parsed reads, both mates of the trimmed ones
    def same_tables(got, cols, max_cycles, first):
        want, t = qo.tables(cols.seq, cols.seq_off, cols.qual, cols.qual_off, max_cycles, first, 2, PHRED)
        for key in ("base", "qhist", "len_hist", "meanq_hist", "n_reads"):
            g = getattr(got, key).cpu().numpy().view(np.uint64).reshape(t[key].shape)
            assert (g == t[key]).all(), (key, np.argwhere(g != t[key])[:6].tolist(), g[g != t[key]][:6], t[key][g != t[key]][:6])
        assert (got.buf.cpu().numpy().view(np.uint64) == want).all()
        return t

    same_tables(tab_before, Batch(reads), 150, 0)
    for first in (0, 1):
        t = same_tables(tab_after[first], Batch(trimmed), 100, first)
        assert int(t["n_reads"][0]) == N // 2 and t["len_hist"][0] > 0 and t["base"][100].sum() > 0
