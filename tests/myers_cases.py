"""The reference's known answers (tests/golden/myers_kats.json) as objects, and what each of them asserts of an
implementation with the restatement's interface (tests/myers_oracle.py) — shared by the CPU rule test and the GPU tests."""
import json
import os

import numpy as np

import myers_oracle as mo

KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "myers_kats.json")))["cases"]
OPS = {"M": mo.MATCH, "S": mo.SUBST, "D": mo.DEL, "I": mo.INS}


def pattern_args(case):
    ambigs = {}
    for sym, eq in case.get("ambigs", ()):
        ambigs.setdefault(ord(sym), []).extend(eq.encode())
    return case["pattern"].encode(), ambigs, list(case.get("wildcards", "").encode())


def restatement(case):
    return mo.Myers(*pattern_args(case))


def k_of(case):
    """the max_dist a case searches with (distance / best_end cases: unbounded)"""
    return case.get("k", 255)


def check_case(case, distance, find_all_end, find_all, paths, best):
    """distance: int or None (empty text); find_all_end: [(end, dist)]; find_all: [(start, end + 1, dist)];
    paths: hit index -> op codes in pattern order, for the hits whose path the implementation can give (the restatement:
    all; the device: those the best call reaches, see best_of_prefix); best: (start, end + 1, dist, ops) of
    find_all(text, k).min_by_key(dist), or None"""
    if "distance" in case:
        assert distance == case["distance"]
    if "best_end" in case:
        assert list(min(find_all_end, key=lambda h: h[1])) == case["best_end"]
    if "find_all_end" in case:
        assert [list(h) for h in find_all_end] == case["find_all_end"]
    if "find_all" in case:
        assert [list(h) for h in find_all] == case["find_all"]
    if "starts" in case:
        assert [h[0] for h in find_all] == case["starts"]
        assert [(h[1] - 1, h[2]) for h in find_all] == [tuple(h) for h in find_all_end]
    if "find_all_first" in case:
        assert list(find_all[0]) == case["find_all_first"]
    if "find_all_prefix" in case:  # the first hits (the reference's example prints them and truncates)
        assert [list(h) for h in find_all[:len(case["find_all_prefix"])]] == case["find_all_prefix"]
    if "max_dist_seen" in case:
        assert max(h[1] for h in find_all_end) == case["max_dist_seen"]
        assert max(h[2] for h in find_all) == case["max_dist_seen"]
    for p in case.get("paths", ()):
        assert list(find_all[p["hit"]]) == p["tuple"]
        if p["hit"] in paths:
            assert list(paths[p["hit"]]) == [OPS[c] for c in p["ops"]]
    if "best" in case:
        assert list(best[:3]) == case["best"]["tuple"] and list(best[3]) == [OPS[c] for c in case["best"]["ops"]]
    if "alignment" in case:
        a = case["alignment"]
        s, e, d = find_all[a["hit"]]
        assert (d, 0, len(case["pattern"]), len(case["pattern"]), s, e, len(case["text"])) == (
            a["score"], a["xstart"], a["xend"], a["xlen"], a["ystart"], a["yend"], a["ylen"])
        assert list(paths[a["hit"]]) == [OPS[c] for c in a["ops"]]


def best_of_prefix(case, hit):
    """True where the hit find_all(text, k)[hit] = (s, e, d) is what the best call returns for text[:e] with bound d — the way
    the device gives the path of a hit that is not the whole text's best (the find-all call writes no operations)"""
    my, text = restatement(case), case["text"].encode()
    s, e, d, ops = my.find_all(text, k_of(case))[hit]
    return mo.best_hit(my, text[:e], d) == (s, e, d, ops)


def named_hits(case):
    """indexes of the find_all hits whose path a case pins"""
    return sorted({p["hit"] for p in case.get("paths", ())} | ({case["alignment"]["hit"]} if "alignment" in case else set()))


# ---- random inputs ----------------------------------------------------------------------------------------------------
def dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def mutated(rng, s, alphabet, rate):
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(rng.choice(alphabet))
            continue
        if r < rate:
            out.append(rng.choice(alphabet))
        out.append(c)
    return bytes(out)


def random_case(rng, m, alphabet=b"ACGT", max_text=100):
    pattern = bytes(rng.choice(alphabet) for _ in range(m))
    n = rng.randint(0, max_text)
    text = bytearray(rng.choice(alphabet) for _ in range(n))
    if n and rng.random() < 0.8:  # a planted, mutated copy
        copy = mutated(rng, pattern, alphabet, rng.choice([0.0, 0.05, 0.15, 0.3]))
        at = rng.randint(0, n)
        text[at:at + len(copy)] = copy
        text = text[:max_text]
    return pattern, bytes(text)


# ---- the calls of both flavours (GPU tests; torch and the package are imported where they are used) -----------------
DEV = "cuda:0"


def mirror(case):
    from rust_bio_amd import myers
    pattern, ambigs, wildcards = pattern_args(case)
    b = myers.MyersBuilder()
    for sym, eq in ambigs.items():
        b.ambig(sym, eq)
    for w in wildcards:
        b.text_wildcard(w)
    return b.build_64(pattern)


def dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy() if dtype is None else np.ascontiguousarray(a).astype(dtype))
    return t.to(DEV)


def both_best(pats, texts, k, stride):
    """the best call of both flavours: [(records, ops)]"""
    import torch
    from rust_bio_amd import _lib, myers
    buf, off = _lib.concat(texts)
    host = myers.best_batch(pats, buf, off, k, ops_stride=stride)
    d_aln, d_ops = myers.best_batch_dev(pats, dev(buf) if len(buf) else torch.zeros(1, dtype=torch.uint8, device=DEV), dev(off, np.int64), k,
                                        ops_stride=stride, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [host, (myers.records(d_aln), d_ops.cpu().numpy() if d_ops is not None else None)]


def both_find_all(pats, texts, k, max_hits, ends_only):
    import torch
    from rust_bio_amd import _lib, myers
    buf, off = _lib.concat(texts)
    host = myers.find_all_batch(pats, buf, off, k, max_hits, ends_only)
    d_aln, d_count = myers.find_all_batch_dev(pats, dev(buf) if len(buf) else torch.zeros(1, dtype=torch.uint8, device=DEV),
                                              dev(off, np.int64), k, max_hits, ends_only, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [host, (myers.records(d_aln), d_count.cpu().numpy().astype(np.uint32))]


def same_best(got, want, stride):
    """records byte for byte; the operations of every hit (the rest of a slot is the caller's)"""
    (rec, ops), (wrec, wops) = got, want
    assert rec.tobytes() == wrec.tobytes()
    if stride:
        for j in np.nonzero(wrec["n_ops"])[0]:
            a, n = int(wrec["ops_off"][j]), int(wrec["n_ops"][j])
            assert ops[a:a + n].tobytes() == wops[a:a + n].tobytes(), j
