"""The per-job bodies of the Myers kernels (csrc/myers.hip: my_best_job, my_find_all_job, `__host__ __device__`) run on the
CPU by a stand-alone program (tests/myers_host_bodies.cpp) built with AddressSanitizer and UBSan, on seeded random batches
against the restatement: records, operations, counts and the overflow flag byte for byte, with the text off alignment and, in
a third of the rounds, operation slots that are too small.  An out-of-bounds read or write of the scratch columns, the text or
an operation slot stops the program."""
import os
import random
import subprocess

import numpy as np

import myers_cases as mc
import myers_oracle as mo
from rust_bio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_job_bodies_on_the_host_under_sanitizers(tmp_path):
    exe, inp, outp = str(tmp_path / "bodies"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + _lib.CSRC, "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "myers_host_bodies.cpp"), "-o", exe])
    PD = _lib.MYERS_PATTERN_DTYPE
    rng = random.Random(1)
    tot = 0
    for rnd in range(40):
        ms = [rng.choice([1, 2, 5, 13, 31, 32, 33, 63, 64]) for _ in range(rng.randint(1, 3))]
        alpha = bytes(rng.sample(range(33, 120), rng.randint(2, 20)))
        pats, texts = [], []
        for m in ms:
            p, _ = mc.random_case(rng, m, alpha)
            pats.append(mo.Myers(p, wildcards=[alpha[0]] if rng.random() < 0.2 else None))
        for _ in range(rng.randint(1, 30)):
            m = rng.choice(ms)
            _, t = mc.random_case(rng, m, alpha, max_text=rng.choice([3, 17, 100, 150]))
            texts.append(t)
        k = rng.choice([0, 1, 2, 3, 8, 31, 64, 255]); mh = rng.choice([1, 4, 64]); stride = rng.choice([128, 128, 6])
        pa = np.zeros(len(pats), dtype=PD)
        for i, p in enumerate(pats):
            pa["peq"][i] = np.array(p.peq, dtype=np.uint64)
            pa["m"][i] = p.m
        off = np.zeros(len(texts) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(t) for t in texts])
        tb = b"".join(texts)
        with open(inp, "wb") as f:
            f.write(np.array([len(pats), k, mh, len(texts), len(tb), stride], dtype=np.uint32).tobytes())
            f.write(pa.tobytes()); f.write(off.tobytes()); f.write(tb)
        subprocess.check_call([exe, inp, outp], stdout=subprocess.DEVNULL)
        raw = open(outp, "rb").read()
        nj = len(texts) * len(pats); o = 0
        best = np.frombuffer(raw, dtype=mo.ALN_DTYPE, count=nj, offset=o); o += nj * 64
        ops = np.frombuffer(raw, dtype=np.uint8, count=nj * stride, offset=o); o += nj * stride
        fa = np.frombuffer(raw, dtype=mo.ALN_DTYPE, count=nj * mh, offset=o); o += nj * mh * 64
        cnt = np.frombuffer(raw, dtype=np.uint32, count=nj, offset=o); o += nj * 4
        fe = np.frombuffer(raw, dtype=mo.ALN_DTYPE, count=nj * mh, offset=o); o += nj * mh * 64
        cnte = np.frombuffer(raw, dtype=np.uint32, count=nj, offset=o); o += nj * 4
        wrec, wops = mo.best_records(pats, texts, k, 128)
        if stride == 128:
            assert best.tobytes() == wrec.tobytes(), (rnd, "best")
            for j in range(nj):
                a, n = int(wrec["ops_off"][j]), int(wrec["n_ops"][j])
                assert ops[a:a + n].tobytes() == wops[a:a + n].tobytes(), (rnd, j)
        else:
            for j in range(nj):
                w = wrec[j].copy(); n = int(w["n_ops"])
                if w["score"] != mo.MIN_SCORE:
                    if n > stride:
                        w["status"] = -9; w["ops_off"] = j * stride
                    else:
                        w["ops_off"] = (j + 1) * stride - n
                        assert ops[(j + 1) * stride - n:(j + 1) * stride].tobytes() == wops[(j + 1) * 128 - n:(j + 1) * 128].tobytes()
                assert best[j].tobytes() == w.tobytes(), (rnd, j, best[j], w)
        w, wc = mo.find_all_records(pats, texts, k, mh, False)
        assert fa.tobytes() == w.tobytes() and (cnt == wc).all(), (rnd, "find_all")
        w, wc = mo.find_all_records(pats, texts, k, mh, True)
        assert fe.tobytes() == w.tobytes() and (cnte == wc).all(), (rnd, "ends")
        tot += nj
    assert tot > 500
