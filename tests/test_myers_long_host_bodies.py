"""The per-job bodies of the block-based Myers kernels (csrc/myers_long.hip: ml_best_job, ml_find_all_job,
`__host__ __device__`) run on the CPU by a stand-alone program (tests/myers_long_host_bodies.cpp) built with AddressSanitizer
and UBSan, on seeded random batches against the restatement at w = 64: records, operations, counts and the overflow flag byte
for byte, with the text off alignment and, in some rounds, operation slots that are too small.  The program gives every job
scratch columns of exactly the size the library reserves, so an out-of-bounds read or write of them, of the text or of an
operation slot stops it."""
import os
import random
import subprocess

import numpy as np

import myers_cases as mc
import myers_long_oracle as ml
from rust_bio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = [1, 63, 64, 65, 127, 128, 129, 193, 300]


def test_job_bodies_on_the_host_under_sanitizers(tmp_path):
    exe, inp, outp = str(tmp_path / "bodies"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + _lib.CSRC, "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "myers_long_host_bodies.cpp"), "-o", exe])
    rng = random.Random(7)
    tot, seen_m, overflowed = 0, set(), 0
    for rnd in range(18):
        ms = [MS[(2 * rnd + i) % len(MS)] for i in range(rng.randint(1, 3))]  # every m in some round
        seen_m.update(ms)
        alpha = bytes(rng.sample(range(33, 120), rng.randint(2, 20)))
        pats, texts = [], []
        for m in ms:
            p, _ = mc.random_case(rng, m, alpha)
            pats.append(ml.MyersLong(p, wildcards=[alpha[0]] if rng.random() < 0.2 else None))
        for _ in range(rng.randint(2, 7)):
            m = rng.choice(ms)
            _, t = mc.random_case(rng, m, alpha, max_text=rng.choice([3, m // 2 + 1, m + 20, m + 60]))
            texts.append(t)
        m_max = max(ms)
        k = rng.choice([0, 1, 3, 8, 63, 64, 65, m_max // 10, m_max, 10 ** 6])
        mh = rng.choice([1, 4, 64])
        stride = rng.choice([2 * m_max, 2 * m_max, 6])
        peq = np.array([blk.peq for p in pats for blk in p.peq], dtype=np.uint64)
        off = np.zeros(len(texts) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(t) for t in texts])
        tb = b"".join(texts)
        with open(inp, "wb") as f:
            f.write(np.array([len(pats), k, mh, len(texts), len(tb), stride, len(peq)], dtype=np.uint32).tobytes())
            f.write(np.array(ms, dtype=np.uint32).tobytes())
            f.write(peq.tobytes())
            f.write(off.tobytes())
            f.write(tb)
        subprocess.check_call([exe, inp, outp], stdout=subprocess.DEVNULL)
        raw = open(outp, "rb").read()
        nj = len(texts) * len(pats)
        o = 0
        best = np.frombuffer(raw, dtype=ml.ALN_DTYPE, count=nj, offset=o); o += nj * 64
        ops = np.frombuffer(raw, dtype=np.uint8, count=nj * stride, offset=o); o += nj * stride
        fa = np.frombuffer(raw, dtype=ml.ALN_DTYPE, count=nj * mh, offset=o); o += nj * mh * 64
        cnt = np.frombuffer(raw, dtype=np.uint32, count=nj, offset=o); o += nj * 4
        fe = np.frombuffer(raw, dtype=ml.ALN_DTYPE, count=nj * mh, offset=o); o += nj * mh * 64
        cnte = np.frombuffer(raw, dtype=np.uint32, count=nj, offset=o); o += nj * 4
        flag = int(np.frombuffer(raw, dtype=np.int32, count=1, offset=o)[0])
        full = 2 * m_max
        wrec, wops = ml.best_records(pats, texts, k, full)
        if stride == full:
            assert best.tobytes() == wrec.tobytes(), (rnd, "best")
            assert flag == 0
            for j in range(nj):
                a, n = int(wrec["ops_off"][j]), int(wrec["n_ops"][j])
                assert ops[a:a + n].tobytes() == wops[a:a + n].tobytes(), (rnd, j)
        else:
            over = False
            for j in range(nj):
                w = wrec[j].copy()
                n = int(w["n_ops"])
                if w["score"] != ml.MIN_SCORE:
                    if n > stride:
                        w["status"] = -9
                        w["ops_off"] = j * stride
                        over = True
                    else:
                        w["ops_off"] = (j + 1) * stride - n
                        assert ops[(j + 1) * stride - n:(j + 1) * stride].tobytes() == wops[(j + 1) * full - n:(j + 1) * full].tobytes()
                assert best[j].tobytes() == w.tobytes(), (rnd, j, best[j], w)
            assert flag == int(over)
            overflowed += over
        w, wc = ml.find_all_records(pats, texts, k, mh, False)
        assert fa.tobytes() == w.tobytes() and (cnt == wc).all(), (rnd, "find_all")
        w, wc = ml.find_all_records(pats, texts, k, mh, True)
        assert fe.tobytes() == w.tobytes() and (cnte == wc).all(), (rnd, "ends")
        tot += nj
    assert seen_m == set(MS) and tot > 60 and overflowed
