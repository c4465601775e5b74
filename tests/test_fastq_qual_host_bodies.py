"""The lane-group bodies of the quality kernels (csrc/fastq_qual_rule.h: the steps of the running-sum and sliding-window cuts —
a scan, a first-negative minimum, a first-maximum key, the carried state — the shares and the merge of the per-read statistics,
the verdict and the pair rule; `__host__ __device__`) run on the CPU by a stand-alone program (tests/fastq_qual_host_bodies.cpp)
built with AddressSanitizer and UBSan, on seeded random batches against the restatement (tests/fastq_qual_oracle.py), byte for
byte.  Every buffer has exactly its size: a byte loaded or stored outside one stops the program.  Group widths 1 and 16; read
lengths 0, 1, 15, 16, 17, 31, 32, 33 and random up to 300; windows 1, 2, 4, 5 and 40 (longer than many reads); every method pair
and every pair flag.  Nothing is loaded into Python."""
import os
import random
import subprocess

import numpy as np

import fastq_qual_oracle as qo
from fastq_qual_cases import METHOD_PAIRS, PHRED, SELECT_FLAGS, cut_params, random_records, select_params
from fastq_write_cases import Batch
from rust_bio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVENTS = ("no-hit", "3p", "5p", "both", "nothing left", "stopped", "window", "pass", "fail", "overruled")


def test_qual_bodies_on_the_host_under_sanitizers(tmp_path):
    exe, inp, outp = str(tmp_path / "bodies"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + _lib.CSRC, "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "fastq_qual_host_bodies.cpp"), "-o", exe])
    rng = random.Random(29)
    seen = {}
    rounds = [(m5, m3, flags, G) for (m5, m3) in METHOD_PAIRS for flags in SELECT_FLAGS for G in (1, 16)]
    for rnd, (m5, m3, flags, G) in enumerate(rounds):
        n = 2 * rng.randint(45, 75)
        a_qual = (rnd * 5 + 1) % 16
        b = Batch(random_records(rng, n), a_qual=a_qual)
        cp = cut_params(rng, m5, m3, window=(1, 2, 4, 5, 40)[rnd % 5])
        sp = select_params(rng, flags)
        weight = qo.ee_weights(PHRED) if rnd % 3 else None
        if weight is not None:  # a bound that some read's sum meets exactly
            sums = sorted(qo.stats_of(r[3], PHRED, 0, weight)["weight_sum"] for r in b.records)
            sp["max_weight"] = sums[len(sums) // 2]
        with open(inp, "wb") as f:
            f.write(np.array([n, G, a_qual, len(b.qual) - a_qual], dtype=np.uint32).tobytes())
            c = np.zeros(1, dtype=_lib.QUAL_CUT_DTYPE)
            s = np.zeros(1, dtype=_lib.QUAL_SELECT_DTYPE)
            c["phred_offset"] = s["phred_offset"] = PHRED
            for k, v in cp.items():
                c[k] = v
            for k, v in sp.items():
                s[k] = v
            f.write(c.tobytes() + s.tobytes() + np.array([weight is not None], dtype=np.uint32).tobytes())
            f.write((weight if weight is not None else np.zeros(256, dtype=np.uint32)).tobytes() + b.qual + b.qual_off.tobytes())
        subprocess.check_call([exe, inp, outp])
        raw = open(outp, "rb").read()
        w_cut, w_tot, _ = qo.cut(b.qual, b.qual_off, PHRED, events=seen, **cp)
        w_stats, w_bin, w_pass = qo.select(b.qual, b.qual_off, phred_offset=PHRED, weight=weight, events=seen, **sp)
        want = w_cut.tobytes() + w_stats.tobytes() + w_bin.tobytes() + np.array([*w_tot, w_pass], dtype=np.uint64).tobytes()
        assert len(raw) == len(want), rnd
        assert raw[:64 * n] == w_cut.tobytes(), (rnd, "cut", cp)
        assert raw[64 * n:96 * n] == w_stats.tobytes(), (rnd, "stats")
        assert raw == want, (rnd, "bin or totals", sp)
    assert all(seen.get(k, 0) >= 50 for k in EVENTS), seen
