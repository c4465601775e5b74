"""The per-record bodies of the FASTQ filter and writer kernels (csrc/fastq_emit_rule.h: fq_line_write, fq_line_flush,
fq_count_n, fq_passes, fq_keeps, fq_copy_record, `__host__ __device__`) run on the CPU by a stand-alone program
(tests/fastq_emit_host_bodies.cpp) built with AddressSanitizer and UBSan, on seeded random batches against the restatement
(tests/fastq_write_oracle.py), byte for byte.  Every source and destination buffer has exactly its size; the four runs of a
line start at every alignment 0 to 15 and are 0 to 40 bytes long; a byte loaded outside a run's buffer, a byte stored outside
the output, or a 16-byte store that is not aligned stops the program."""
import os
import random
import subprocess

import numpy as np

import fastq_write_oracle as fw
from rust_bio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = b"ACGTNnacgt"


def random_batch(rng, n, a_text, a_seq, a_qual):
    """records whose four runs are 0 .. 40 bytes, behind prefixes of a_* bytes: (recs, text, seq, qual, seq_off, qual_off)"""
    recs = np.zeros(n, dtype=_lib.FQREC_DTYPE)
    text, seq, qual = bytearray(b"#" * a_text), bytearray(b"#" * a_seq), bytearray(b"#" * a_qual)
    so, qo = [a_seq], [a_qual]
    for r in range(n):
        c = recs[r]
        id_ = bytes(rng.randint(48, 122) for _ in range(rng.randint(0, 40)))
        c["id_off"], c["id_len"] = len(text), len(id_)
        text += id_ + b" "
        if rng.random() < 0.6:
            d = bytes(rng.randint(48, 122) for _ in range(rng.randint(0, 40)))
            c["has_desc"], c["desc_off"], c["desc_len"] = 1, len(text), len(d)
            text += d
        text += b"\n"
        s = bytes(rng.choice(ALPHA) for _ in range(rng.randint(0, 40)))
        q = bytes(rng.randint(33, 73) for _ in range(len(s) if rng.random() < 0.8 else rng.randint(0, 40)))
        c["seq_off"], c["seq_len"], c["qual_off"], c["qual_len"] = len(seq), len(s), len(qual), len(q)
        c["check"] = rng.choice([0, 0, 0, 1, 3, 5])
        seq += s
        qual += q
        so.append(len(seq))
        qo.append(len(qual))
    # the text ends with its last run: nothing behind it may be read
    last = recs[n - 1]
    end = int(last["desc_off"] + last["desc_len"]) if last["has_desc"] else int(last["id_off"] + last["id_len"])
    return recs, bytes(text[:end]) if n else bytes(text), bytes(seq), bytes(qual), np.array(so, np.uint64), np.array(qo, np.uint64)


def test_record_bodies_on_the_host_under_sanitizers(tmp_path):
    exe, inp, outp = str(tmp_path / "bodies"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + _lib.CSRC, "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "fastq_emit_host_bodies.cpp"), "-o", exe])
    rng = random.Random(3)
    lines = 0
    for rnd in range(48):
        a_text, a_seq, a_qual, a_out = rnd % 16, (rnd * 7 + 3) % 16, (rnd * 5 + 1) % 16, (rnd * 11 + 2) % 16  # each takes all 16 values
        n = 2 * rng.randint(1, 20)
        G = rng.choice([16, 32])
        first, step = rng.choice([(0, 1), (0, 2), (1, 2), (n, 1), (3, 5)])
        recs, text, seq, qual, so, qo = random_batch(rng, n, a_text, a_seq, a_qual)
        n_pat = rng.choice([1, 3])
        hits = np.zeros(n * n_pat, dtype=_lib.ALN_DTYPE)
        hits["score"] = [fw.MIN_SCORE if rng.random() < 0.7 else rng.randint(0, 3) for _ in range(n * n_pat)]
        flags = rng.choice([0, fw.PAIRED, fw.PAIRED | fw.PAIR_BOTH]) | rng.choice([0, 0, fw.DISCARD_TRIMMED, fw.DISCARD_UNTRIMMED]) | \
            rng.choice([0, fw.CHECK_OK])
        flt = dict(flags=flags, min_len=rng.choice([0, 1, 10]), max_len=rng.choice([fw.NO_BOUND, 30, 40]), max_n=rng.choice([fw.NO_BOUND, 0, 2, 5]))
        with open(inp, "wb") as f:
            f.write(np.array([n, G, a_text, a_seq, a_qual, a_out, len(text) - a_text, len(seq) - a_seq, len(qual) - a_qual, first, step,
                              flt["flags"], flt["min_len"], flt["max_len"], flt["max_n"], n_pat, 1, 0], dtype=np.uint32).tobytes())
            f.write(recs.tobytes() + text + seq + qual + so.tobytes() + qo.tobytes() + hits.tobytes())
        subprocess.check_call([exe, inp, outp])
        raw = open(outp, "rb").read()
        want_text, want_off = fw.emit(text, recs, seq, qual, first, step)
        assert np.frombuffer(raw, np.int32, 1, 0)[0] == 1, (rnd, "the bytes in front of the output were written")
        total = int(np.frombuffer(raw, np.uint64, 1, 4)[0])
        assert total == len(want_text), rnd
        o = 12
        assert raw[o:o + total] == want_text, (rnd, "staged")
        assert raw[o + total:o + 2 * total] == want_text, (rnd, "direct")
        o += 2 * total
        m = len(want_off) - 1
        assert (np.frombuffer(raw, np.uint64, m + 1, o) == want_off).all(), rnd
        o += 8 * (m + 1)
        w_recs, w_seq, w_so, w_qual, w_qo, w_keep = fw.filter_columns(recs, seq, so, qual, qo, hits=hits, n_pat=n_pat, **flt)
        assert raw[o:o + n] == w_keep.tobytes(), (rnd, flt)
        o += n
        nk = int(np.frombuffer(raw, np.uint64, 1, o)[0])
        o += 8
        assert nk == len(w_recs), rnd
        assert raw[o:o + 56 * nk] == w_recs.tobytes(), rnd
        o += 56 * nk
        assert (np.frombuffer(raw, np.uint64, nk + 1, o) == w_so).all() and (np.frombuffer(raw, np.uint64, nk + 1, o + 8 * (nk + 1)) == w_qo).all()
        o += 16 * (nk + 1)
        assert raw[o:o + len(w_seq)] == w_seq and raw[o + len(w_seq):] == w_qual, rnd
        lines += m
    assert lines > 300
