"""Differential fuzz of the block-based Myers calls (run by hand on a GPU box: python tests/fuzz_myers_long.py SEED SECONDS
[SUMMARY_FILE]): random batches through bg_myers_long_best_batch[_dev] and bg_myers_long_find_all_batch[_dev] (with starts and
ENDS_ONLY) against the Python restatement at w = 64 (tests/myers_long_oracle.py), records, operations and counts byte for byte.
A round: 1 to 4 patterns of random lengths 1 .. 330 (often next to a multiple of 64, now and then 1000 .. 1024) over an alphabet
of 2 to 20 symbols (sometimes with an ambiguity code or a text wildcard), 1 to 20 texts of 0 to 300 bytes with planted, mutated
copies of the patterns, a random bound k, max_hits and operation stride (sometimes too small), the device text at a random byte
offset, and now and then a ctx with small launches and a small table budget."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import myers_long_oracle as mo  # noqa: E402
from rust_bio_amd import _lib, myers  # noqa: E402

seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
rng = np.random.default_rng(seed)
budget = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
t0 = time.time()
rounds = n_jobs = n_hits = n_cap = n_fail = 0
small = _lib.Context(0)
small.set_option("myers_chunk_jobs", 256)
small.set_option("myers_lds_bytes", 4096)


def rand_bytes(alphabet, n):
    return alphabet[rng.integers(0, len(alphabet), size=n)].tobytes()


def mutate(s, alphabet, rate):
    out = bytearray()
    for c in s:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < rate:
            out += rand_bytes(alphabet, 1)
            if u < 2 * rate / 3:
                continue
        out.append(c)
    return bytes(out)


while time.time() - t0 < budget and n_fail == 0:
    rounds += 1
    alphabet = rng.permutation(np.arange(33, 127, dtype=np.uint8))[:int(rng.integers(2, 21))]
    pats, wants, plain = [], [], []
    for _ in range(int(rng.integers(1, 5))):
        u = rng.random()
        m = int(rng.choice([1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257])) if u < 0.4 else int(rng.integers(1, 331))
        if u > 0.97:
            m = int(rng.integers(1000, 1025))
        p = rand_bytes(alphabet, m)
        ambigs = {int(alphabet[0]): [int(c) for c in alphabet[1:3]]} if rng.random() < 0.2 else None
        wild = [int(alphabet[-1])] if rng.random() < 0.2 else None
        b = myers.MyersBuilder()
        for sym, eq in (ambigs or {}).items():
            b.ambig(sym, eq)
        for w in wild or ():
            b.text_wildcard(w)
        pats.append(b.build_long_64(p))
        wants.append(mo.MyersLong(p, ambigs, wild))
        plain.append(p)
    texts = []
    for _ in range(int(rng.integers(1, 21))):
        t = rand_bytes(alphabet, int(rng.integers(0, 301)))
        if rng.random() < 0.7:
            copy = mutate(plain[int(rng.integers(0, len(plain)))], alphabet, float(rng.choice([0, 0.05, 0.15, 0.3])))
            at = int(rng.integers(0, len(t) + 1))
            t = (t[:at] + copy + t[at:])[:300]
        texts.append(t)
    k = int(rng.choice([0, 1, 2, 3, 5, 8, 16, 32, 63, 64, 65, 128, 255, 1024, 10 ** 6]))
    max_hits = int(rng.choice([1, 2, 4, 64]))
    full = 2 * max(w.m for w in wants)
    stride = int(rng.choice([full, full, full, max(w.m for w in wants) + 1]))
    ctx = small if rounds % 5 == 0 else None
    buf, off = _lib.concat(texts)
    shift = int(rng.integers(0, 16))
    d_buf = torch.zeros(len(buf) + shift + 16, dtype=torch.uint8, device="cuda")
    d_text = d_buf[shift:shift + max(1, len(buf))]
    d_text[:len(buf)].copy_(torch.from_numpy(buf.copy()))
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    err = None
    # the best call
    wide, wops = mo.best_records(wants, texts, k, full)
    host = myers.long_best_batch(pats, buf, off, k, ops_stride=stride, ctx=ctx, allow_ops_cap=True)
    d_aln, d_ops = myers.long_best_batch_dev(pats, d_text, d_off, k, ops_stride=stride, ctx=ctx, allow_ops_cap=True)
    torch.cuda.synchronize()
    for name, (rec, ops) in (("host", host), ("dev", (myers.records(d_aln), d_ops.cpu().numpy()))):
        for j in range(len(wide)):
            w = wide[j].copy()
            n = int(w["n_ops"])
            if w["score"] != mo.MIN_SCORE:
                if n > stride:
                    w["status"], w["ops_off"] = -9, j * stride
                    n_cap += name == "dev"
                else:
                    w["ops_off"] = (j + 1) * stride - n
                    if ops[(j + 1) * stride - n:(j + 1) * stride].tobytes() != wops[(j + 1) * full - n:(j + 1) * full].tobytes():
                        err = err or "best %s: operations of job %d" % (name, j)
            if rec[j].tobytes() != w.tobytes():
                err = err or "best %s: record of job %d: %s, want %s" % (name, j, rec[j], w)
    # find-all, with starts and ends only
    for ends_only in (False, True):
        wrec, wcount = mo.find_all_records(wants, texts, k, max_hits, ends_only)
        rec, count = myers.long_find_all_batch(pats, buf, off, k, max_hits, ends_only, ctx=ctx)
        d_aln, d_count = myers.long_find_all_batch_dev(pats, d_text, d_off, k, max_hits, ends_only, ctx=ctx)
        torch.cuda.synchronize()
        for name, r, c in (("host", rec, count), ("dev", myers.records(d_aln), d_count.cpu().numpy().astype(np.uint32))):
            if not (c == wcount).all() or r.tobytes() != wrec.tobytes():
                err = err or "find_all %s ends_only=%s" % (name, ends_only)
        if not ends_only:
            n_hits += int(wcount.sum())
    n_jobs += len(wide)
    if err:
        n_fail += 1
        print("MISMATCH round", rounds, "seed", seed, "k", k, "max_hits", max_hits, "stride", stride, "patterns", plain, err, flush=True)
line = "rounds %d jobs %d hits traced %d paths over their slot %d failures %d" % (rounds, n_jobs, n_hits, n_cap, n_fail)
print(line, flush=True)
if len(sys.argv) > 3:
    open(sys.argv[3], "w").write("tests/fuzz_myers_long.py seed %s, %.0f s on one MI355X: host and device flavours of bg_myers_long_best_batch and "
                                 "bg_myers_long_find_all_batch (with starts, ENDS_ONLY) against tests/myers_long_oracle.py at w = 64\n%s\n" % (sys.argv[1], budget, line))
sys.exit(1 if n_fail else 0)
