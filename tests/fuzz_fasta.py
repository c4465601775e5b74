"""Differential fuzz of the FASTA ingest (run by hand on a GPU box: python tests/fuzz_fasta.py SEED SECONDS [SUMMARY_FILE]): random
texts through bg_fasta_parse (host buffers) and bg_fasta_parse_dev (device buffers, base pointer off alignment) against the Python
restatement (tests/fasta_oracle.py): status, error position, every record's id / description / sequence / Record::check, offsets;
every fourth clean round also bg_fasta_reference[_dev] in a random layout against the numpy statement.
Texts: records whose lengths come from one of several regimes (empty, a few bases, a few lines, one to three tiles), line widths
from 1 to a whole record, LF or CRLF, headers with and without descriptions, with blanks, tabs and multi-byte white space, trailing
and interior white space in sequence lines, a prefix of random length (every tile phase) — and, in a third of the rounds, one
defect: a byte >= 0x80, a multi-byte character at a random place, a blank header, a blank line, '>' in the middle of a line, a
truncated tail, no newline at the end, a long run of white space."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import fasta_oracle as fo  # noqa: E402
from rust_bio_amd import _lib, fasta  # noqa: E402

rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 1)
budget = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
B = fasta.B
ALPHA = np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)
ODD = np.frombuffer(b"ACGTN-.*RYKM#5 $", dtype=np.uint8)
WS = [b" ", b"\t", b"\r", b"\x0b", b"\xc2\x85", b"\xc2\xa0", b"\xe2\x80\x83", b"\xe3\x80\x80", b"\xe1\x9a\x80"]
t0 = time.time()
rounds = n_rec = n_bytes = n_fail = n_ref = 0
by_status = {"ok": 0, "MissingGt": 0, "Io": 0}


def record(k, ln, nl, odd):
    alpha = ODD if odd and rng.random() < 0.3 else ALPHA
    s = alpha[rng.integers(0, len(alpha), size=ln)].tobytes()
    hdr = b">" + (b"" if odd and rng.random() < 0.05 else b"s%d" % k)
    u = rng.random()
    if u < 0.4:
        hdr += b" " + bytes(rng.integers(97, 123, size=int(rng.integers(0, 30))).astype(np.uint8))
    elif u < 0.5:
        hdr += WS[int(rng.integers(0, len(WS)))] + b" two  words" + WS[int(rng.integers(0, len(WS)))]
    width = int(rng.choice([1, 7, 60, 70, 80, 1000, max(1, ln)]))
    out = hdr + nl
    for a in range(0, ln, width):
        out += s[a:a + width]
        if odd and rng.random() < 0.1:
            out += b"".join(WS[int(i)] for i in rng.integers(0, len(WS), size=int(rng.integers(1, 4))))
        out += nl
    return out


def compare(text, got, want):
    wrecs, wst, wpos = want
    if (got.status, got.err_pos, len(got)) != (wst, wpos, len(wrecs)):
        return "status %s at %d with %d records, want %s at %d with %d" % (got.status, got.err_pos, len(got), wst, wpos, len(wrecs))
    for k, w in enumerate(wrecs):
        r = got.record(k)
        if (r._id, r._desc, r._seq, fasta.CHECK[r._check]) != (w["id"], w["desc"], w["seq"], w["check"]):
            return "record %d: %r %r len %d %s, want %r %r len %d %s" % (k, r._id, r._desc, len(r._seq), fasta.CHECK[r._check], w["id"], w["desc"],
                                                                       len(w["seq"]), w["check"])
        if (int(got.recs["seq_off"][k]), int(got.recs["seq_len"][k])) != (int(got.seq_off[k]), len(w["seq"])):
            return "record %d: offsets" % k
    return None


def dev_parse(text, shift):
    t = np.frombuffer(text, dtype=np.uint8)
    buf = torch.zeros(len(t) + shift + 16, dtype=torch.uint8, device="cuda")
    d_text = buf[shift:shift + len(t)]
    d_text.copy_(torch.from_numpy(t.copy()))
    n, status, err_pos, d_recs, d_seq, d_so = fasta.parse_dev(d_text)
    so = d_so.cpu().numpy().view(np.uint64)
    return (fasta.Parsed(t, d_recs.cpu().numpy().view(_lib.FAREC_DTYPE), d_seq.cpu().numpy()[:int(so[n])], so, fasta.STATUS.index(status), err_pos),
            (n, d_recs, d_text, d_seq))


while time.time() - t0 < budget and n_fail == 0:
    rounds += 1
    regime = int(rng.integers(0, 5))
    lo, hi, cnt = [(0, 3, 400), (1, 200, 300), (200, 3000, 40), (B - 70, B + 70, 6), (B, 3 * B, 4)][regime]
    n = int(rng.integers(1, cnt + 1))
    nl = b"\r\n" if rng.random() < 0.2 else b"\n"
    odd = rng.random() < 0.4
    parts = [record(k, int(rng.integers(lo, hi + 1)), nl, odd) for k in range(n)]
    pre = int(rng.integers(0, B + 100))
    text = (b">p\n" + b"A" * pre + nl if rng.random() < 0.7 else b"") + b"".join(parts)
    if rng.random() < 0.33 and len(text) > 20:
        kind = int(rng.integers(0, 8))
        at = int(rng.integers(0, len(text)))
        if kind == 0:
            text = text[:at] + bytes([int(rng.integers(128, 256))]) + text[at + 1:]
        elif kind == 1:
            text = text[:at] + [b"\xe2\x98\xb9", b"\xc3\xa9", b"\xf0\x9f\x98\x80", b"\xe2\x80\x83", b"\xc2\xa0"][int(rng.integers(0, 5))] + text[at:]
        elif kind == 2:
            nlp = text.find(b"\n>", at)
            if nlp >= 0:
                text = text[:nlp + 2] + [b"\n", b"  \n \n", b"\n\n"][int(rng.integers(0, 3))] + text[nlp + 2:]
        elif kind == 3:
            nlp = text.find(b"\n", at)
            if nlp >= 0:
                text = text[:nlp + 1] + nl + text[nlp + 1:]
        elif kind == 4:
            text = text[:at] + b">" + text[at:]
        elif kind == 5:
            text = text[:at]
        elif kind == 6:
            text = text.rstrip(b"\r\n")
        else:
            text = text[:at] + b" " * int(rng.integers(1, 2 * B + 50)) + text[at:]
    want = fo.parse(text)
    host = fasta.parse_arrays(text)
    dev, handles = dev_parse(text, int(rng.integers(0, 16)))
    err = compare(text, host, want) or compare(text, dev, want)
    if err is None and not (host.recs == dev.recs).all():
        err = "host and device records differ"
    if err is None and rounds % 4 == 0 and want[0] and all(r["check"] == "ok" for r in want[0]):
        flags = int(rng.integers(0, 4))
        wtext, wcontigs = fo.reference(want[0], fmd=bool(flags & fasta.REF_FMD), upper=bool(flags & fasta.REF_UPPER))
        htext, hc = fasta.reference_arrays(host, flags)
        d_text, _, _, dc = fasta.reference_dev(handles[0], handles[1], handles[2], handles[3], flags)
        n_ref += 1
        if not (htext.tobytes() == wtext.tobytes() == d_text.cpu().numpy().tobytes() and hc.table.tobytes() == dc.table.tobytes()
                and hc.names.tobytes() == dc.names.tobytes()
                and [(hc.name(c), int(hc.table["start"][c]), int(hc.table["len"][c])) for c in range(len(hc))] == wcontigs):
            err = "reference text or contigs differ (flags %d)" % flags
    if err:
        n_fail += 1
        fn = "/tmp/fuzz_fasta_fail_%d.fa" % rounds
        open(fn, "wb").write(text)
        print("MISMATCH round", rounds, "regime", regime, "bytes", len(text), err, "->", fn, flush=True)
    by_status[want[1]] += 1
    n_rec += len(want[0])
    n_bytes += len(text)
line = "rounds %d records %d bytes %d reference builds %d statuses %s failures %d" % (rounds, n_rec, n_bytes, n_ref, by_status, n_fail)
print(line, flush=True)
if len(sys.argv) > 3:
    open(sys.argv[3], "w").write("tests/fuzz_fasta.py seed %s, %.0f s on one MI355X: host and device flavours of bg_fasta_parse and "
                                 "bg_fasta_reference against tests/fasta_oracle.py\n%s\n" % (sys.argv[1], budget, line))
sys.exit(1 if n_fail else 0)
