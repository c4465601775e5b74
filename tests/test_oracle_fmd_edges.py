"""The corpus of tests/fmd_cases.py under the CPU oracle (oracle_py.FMDIndex, fmindex.rs:363-501): every case shows what it claims
to hit, and the corpus as a whole holds each property the GPU tests (tests/test_gpu_fmd_edges.py) lean on.  No GPU needed."""
import functools

import numpy as np
import pytest

import fmd_cases as fc
import oracle_py as orc

CASES = fc.cases()


@functools.lru_cache(maxsize=None)
def index_of(fwd, alphabet):
    text = fc.full_text(fwd)
    sa = orc.suffix_array(text)
    b = orc.bwt(text, sa)
    ls = orc.less(b, alphabet)
    return b, ls, orc.FMDIndex(b, ls, orc.Occ(b, 3, alphabet))


def raises(f, *a):
    try:
        f(*a)
    except IndexError:
        return True
    return False


def trace(ofmd, read, i):
    """smems(read, i, 0) step by step on the oracle's single extensions (fmindex.rs:363-434) -> (steps of the forward pass at
    which the interval's size changes, list entries dropped as duplicates of their neighbour's size)"""
    iv = ofmd.init_interval_with(read[i])
    ml = 1 if iv[2] else 0
    curr, changes = [], 0
    for p in range(i + 1, len(read)):
        f = ofmd.forward_ext(iv, read[p])
        if f[2] != iv[2]:
            curr.append((iv, ml))
            changes += 1
        if f[2] == 0:
            break
        iv, ml = f, ml + 1
    curr.append((iv, ml))
    prev, dropped = curr[::-1], 0
    for k in range(i - 1, -2, -1):
        a = ord("$") if k == -1 else read[k]
        curr, last = [], -1
        for e, m in prev:
            f = ofmd.backward_ext(e, a)
            if f[2] != 0 and f[2] == last:
                dropped += 1
            if f[2] != 0 and f[2] != last:
                last = f[2]
                curr.append((f, m + 1))
        if not curr:
            break
        prev = curr
    return changes, dropped


def facts(case):
    """the names of fc.CLAIMS this case shows under the oracle"""
    b, ls, ofmd = index_of(case["text"], case["alphabet"])
    reads, pos, ml = case["reads"], case["positions"], case["min_len"]
    buf, off = fc.concat(reads)
    counts, flat = fc.oracle_batch(orc, ofmd, buf, off, pos, ml)
    seen = set()
    if (flat[:, 2] == 0).any():
        seen.add("size0")
    if (flat[:, 0] == flat[:, 1]).any():
        seen.add("palindrome")
    if ((counts != fc.PANIC) & (counts >= 20)).any():
        seen.add("many_records")
    for r in flat[flat[:, 4] == 0][:50]:
        if r[2] and not raises(ofmd.backward_ext, tuple(int(v) for v in r[:4]), ord("$")) and \
                ofmd.backward_ext(tuple(int(v) for v in r[:4]), ord("$"))[2] != 0:
            seen.add("dollar_step")
            break
    lens = np.diff(off).astype(np.int64)
    for s in range(0, len(reads), 64):
        if (lens[s:s + 64] <= 248).any() and (lens[s:s + 64] > 248).any():
            seen.add("mixed_block")
    less_len = len(ls)
    for q, r in enumerate(reads):
        i = 0 if pos is None else pos[q]
        panicked = counts[q] == fc.PANIC
        if pos is not None and len(r) == 0 and panicked:
            seen.add("panic_empty")
        if pos is None and len(r) == 0 and counts[q] == 0:
            seen.add("empty_all")
        if pos is not None and len(r) and i >= len(r) and panicked:
            seen.add("panic_i")
        if panicked and len(r) and i < len(r):
            # why: a byte beyond `less` (the read is fine with A in its place); else a first byte below '$', whose empty interval
            # starts at row 0 (lower + size == 0); else a symbol of the extension order outside the index's alphabet
            high = bytes(c for c in set(r) if c + 1 >= less_len)
            if high:
                fixed = r.translate(bytes.maketrans(high, b"A" * len(high)))
                if not raises(ofmd._smems, fixed, i, ml, 1 if pos is None else 0):
                    seen.add("panic_less")
            elif min(r) < ord("$"):
                seen.add("panic_underflow")
            else:
                seen.add("panic_class")
        if not panicked and b"X" in r:
            seen.add("x_no_panic")
    if "long_forward" in case["claims"] or "dedup" in case["claims"]:
        for q, r in enumerate(reads):
            i = 0 if pos is None else pos[q]
            if counts[q] == fc.PANIC or not 2 <= len(r) <= 400 or i >= len(r):
                continue
            changes, dropped = trace(ofmd, r, i)
            if changes >= 100:
                seen.add("long_forward")
            if dropped:
                seen.add("dedup")
    return seen, counts


@functools.lru_cache(maxsize=None)
def all_facts():
    return {c["name"]: facts(c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_hits_what_it_claims(case):
    assert case["claims"] <= set(fc.CLAIMS)
    assert len(fc.full_text(case["text"])) <= 2 * 66_001
    seen, counts = all_facts()[case["name"]]
    assert case["claims"] <= seen, (case["name"], sorted(case["claims"] - seen))
    assert len(counts) == len(case["reads"]) and (case["positions"] is None or len(case["positions"]) == len(case["reads"]))


@pytest.mark.parametrize("claim", sorted(fc.CLAIMS))
def test_corpus_holds_every_property(claim):
    assert any(claim in seen for seen, _ in all_facts().values()), fc.CLAIMS[claim]


def test_the_oracle_facts_the_corpus_is_built_on():
    b, ls, ofmd = index_of(fc.texts()["random"]["text"], fc.ALPHA)
    assert raises(ofmd.smems, b"", 0, 0) and raises(ofmd.smems, b"ACGT", 4, 0)
    assert ofmd.all_smems(b"", 0) == []
    assert ord("X") + 1 < len(ls) <= ord("z")
    r = fc.texts()["random"]["text"][500:560]
    got = ofmd.all_smems(fc.with_byte(r, 20, ord("X")), 0)
    assert got and any(iv[2] == 0 for iv, _, _ in got)
    assert raises(ofmd.all_smems, fc.with_byte(r, 20, 0xFF), 0) and raises(ofmd.all_smems, fc.with_byte(r, 20, ord("z")), 0)


def test_texts_are_what_they_are_named():
    t = fc.texts()
    assert all(len(v["text"]) <= 60_000 for k, v in t.items() if k != "limit") and len(t["limit"]["text"]) == 66_000
    assert fc.full_text(t["two_sequences"]["text"]).count(b"$") == 4 and fc.full_text(t["five_sequences"]["text"]).count(b"$") == 10
    assert t["few_n"]["text"].count(b"N") in range(1, 9) and b"A" * 300 in t["homopolymer"]["text"]
    assert any(c in t["soft_masked"]["text"] for c in b"acgt")
    assert fc.revcomp(t["own_revcomp"]["text"]) == t["own_revcomp"]["text"]
    assert t["dense_n"]["text"].count(b"N") > 1024  # more than the sparse lists hold: rank bit vectors
    for p, n in ((b"AC", 400), (b"ACG", 300), (b"ACGTTGA", 150)):
        assert p * n in t["tandem"]["text"]
    seg = [t["four_copies"]["text"][1_500 * k + 1_000:1_500 * k + 1_500] for k in range(4)]
    assert all(sum(a != b for a, b in zip(seg[0], s)) == 2 for s in seg[1:])
    _, too_long = fc.refused_read()
    assert len(too_long) == 65_535


def test_big_batch_is_what_the_gpu_test_needs():
    """more reads than 256 CUs x 8 blocks x 64 quads, the stated shares of long, panicking and empty reads, and every read
    answered by the oracle — with panics exactly where a byte lies beyond `less`, a read is empty (smems) or i >= len"""
    bb = fc.big_batch()
    n = len(bb["off"]) - 1
    assert n == 300_000 and n > 2 * 131_072
    lens = np.diff(bb["off"]).astype(np.int64)
    short = lens[~bb["long"] & ~bb["empty"]]
    assert short.min() == 12 and short.max() == 40 and lens[bb["long"]].min() >= 249 and lens.max() <= 400
    assert 0.008 < bb["long"].mean() < 0.012 and 0.005 < bb["bad"].mean() < 0.01
    b, ls, ofmd = index_of(bb["text"], bb["alphabet"])
    call, cflat = fc.oracle_batch(orc, ofmd, bb["buf"], bb["off"], None, 10)
    assert ((call == fc.PANIC) == bb["bad"]).all()
    assert 0.005 < (call == fc.PANIC).mean() < 0.01
    cs, sflat = fc.oracle_batch(orc, ofmd, bb["buf"], bb["off"], bb["positions"], 10)
    must = bb["empty"] | (bb["positions"] >= lens)
    assert ((cs == fc.PANIC) >= must).all() and ((cs == fc.PANIC) <= (must | bb["bad"])).all()
    assert bb["empty"].sum() > 500 and (bb["positions"] >= lens)[~bb["empty"]].sum() > 500
    # every third slot of a launch with the most quad slots possible walks a panicking read right before or after a clean one
    slot = np.arange(n) % 131_072
    pan = call == fc.PANIC
    assert (pan[131_072:] & ~pan[:n - 131_072]).sum() > 100 and (~pan[131_072:] & pan[:n - 131_072]).sum() > 100
    assert len(np.unique(slot[bb["long"]])) > 1000 and len(cflat) > n and len(sflat) > n // 2
