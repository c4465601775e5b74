"""The oracle's scores at the extreme scorings the narrow-score kernels are admitted for (tests/test_gpu_score_edges.py
compares the kernels with the oracle there), checked against a plain Gotoh recurrence in int64 that shares nothing with
oracle/: global, semiglobal and local, score only.  No GPU."""
import numpy as np
import pytest

import oracle_py as orc
from rust_bio_amd import _lib

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
NEG_INF = -(1 << 62)


def gotoh_score(x, y, mode, gap_open, gap_extend, match, mismatch):
    """Best score of x (rows) against y (columns); a gap of length k costs gap_open + (k - 1) * gap_extend.  global: both
    whole; semiglobal: x whole, y free at both ends; local: free everywhere, never below 0.  Rows are vectors: the vertical
    gap and the diagonal are elementwise, the horizontal gap of a row is a cumulative max."""
    assert gap_open <= 0 and gap_extend <= 0
    x = np.frombuffer(bytes(x), dtype=np.uint8)
    y = np.frombuffer(bytes(y), dtype=np.uint8)
    m, n = len(x), len(y)
    go, ge = np.int64(gap_open), np.int64(gap_extend)
    j = np.arange(n + 1, dtype=np.int64)
    if mode == "global":
        S = np.where(j == 0, 0, go + ge * (j - 1))
    else:
        S = np.zeros(n + 1, dtype=np.int64)
    I = np.full(n + 1, NEG_INF, dtype=np.int64)
    best = S.max() if mode == "local" else None
    for i in range(1, m + 1):
        I = np.maximum(S + go, I + ge)  # x[i - 1] against a gap
        T = np.empty(n + 1, dtype=np.int64)
        T[0] = 0 if mode == "local" else go + ge * (i - 1)
        sub = np.where(y == x[i - 1], np.int64(match), np.int64(mismatch))
        T[1:] = np.maximum(S[:-1] + sub, I[1:])
        if mode == "local":
            T[1:] = np.maximum(T[1:], 0)
        # y[j - 1] against a gap: D[j] = max(S[j - 1] + go, D[j - 1] + ge) with S = max(T, D) is
        # D[j] = max(T[j - 1] + go, D[j - 1] + e), e = max(go, ge) (a gap may also close and open again), so
        # D[j] = go + e * (j - 1) + max_{k < j} (T[k] - e * k)
        e = max(go, ge)
        run = np.maximum.accumulate(T - e * j)
        D = np.full(n + 1, NEG_INF, dtype=np.int64)
        D[1:] = run[:-1] + go + e * j[:-1]
        S = np.maximum(T, D)
        if mode == "local":
            best = max(best, S.max())
    if mode == "global":
        return int(S[n])
    if mode == "semiglobal":
        return int(S.max())
    return int(best)


def families(rng, m, n):
    """Pairs that reach the ends of a scoring's range: equal sequences (positive end), disjoint letters (every cell a
    mismatch or a gap: negative end), a 1-8 symbol x against y, and related / unrelated pairs of lengths m x n."""
    out = []
    y = ACGT[rng.integers(0, 4, size=n)]
    if m == n:
        out.append((y.tobytes(), y.tobytes()))
    out.append((b"A" * m, b"C" * n))
    for k in sorted({1, 3, 8}):
        if k <= m:
            out.append((b"A" * k, b"C" * n))
            s = int(rng.integers(0, max(1, n - k)))
            out.append((y[s:s + k].tobytes(), y.tobytes()))
    x = np.resize(y[int(rng.integers(0, max(1, n // 4))):], m).copy()
    k = max(1, m // 10)
    x[rng.integers(0, m, size=k)] = ACGT[rng.integers(0, 4, size=k)]
    out.append((x.tobytes(), y.tobytes()))
    out.append((ACGT[rng.integers(0, 4, size=m)].tobytes(), y.tobytes()))
    return out


def magnitude_scorings(mag):
    """Scorings whose largest finite magnitude is mag: everything at -mag / +mag, and mixed ones."""
    return [dict(gap_open=-mag, gap_extend=-mag, match=mag, mismatch=-mag),
           dict(gap_open=-mag, gap_extend=-max(1, mag // 3), match=max(0, mag // 2), mismatch=-mag),
           dict(gap_open=0, gap_extend=-mag, match=mag, mismatch=-mag)]  # (closing and reopening a gap is cheaper)


# every path ties: all zeros; match == mismatch (both 0: MatchParams wants match >= 0 >= mismatch); free gaps
TIE_SCORINGS = [dict(gap_open=0, gap_extend=0, match=0, mismatch=0), dict(gap_open=-3, gap_extend=-1, match=0, mismatch=0),
                dict(gap_open=0, gap_extend=0, match=1, mismatch=-1)]


def oracle_scores(kw, mode, pairs):
    x, xo = _lib.concat([p[0] for p in pairs])
    y, yo = _lib.concat([p[1] for p in pairs])
    out, _, _ = orc.align_batch(orc.make_scoring(**kw), mode, x, xo, y, yo, threads=8, want_ops=False)
    return [int(s) for s in out["score"]]


def test_gotoh_reference_by_hand():
    kw = dict(gap_open=-5, gap_extend=-1, match=1, mismatch=-1)
    assert gotoh_score(b"ACGT", b"ACGT", "global", **kw) == 4
    assert gotoh_score(b"ACGT", b"AGT", "global", **kw) == 3 - 5
    assert gotoh_score(b"A", b"CCCC", "global", **kw) == -1 - 5 - 2
    assert gotoh_score(b"AC", b"AGGGC", "global", gap_open=0, gap_extend=-3, match=1, mismatch=-1) == 2  # re-opening is free
    assert gotoh_score(b"GT", b"AAGTAA", "semiglobal", **kw) == 2
    assert gotoh_score(b"TTACGTTT", b"GGACGGG", "local", **kw) == 3
    assert gotoh_score(b"A" * 5, b"C" * 7, "local", **kw) == 0


# (mag, L) with mag * (L + 2) == 2040 (K1p's bound) and the K1 narrow bound at m + n + 8 = 2008
@pytest.mark.parametrize("mag,m,n", [(1, 8, 2038), (3, 150, 678), (12, 168, 168), (60, 32, 32), (680, 1, 1), (170, 10, 10),
                                     (8355, 1000, 1000), (8356, 300, 1700)])
@pytest.mark.parametrize("mode", ["global", "semiglobal", "local"])
def test_oracle_scores_equal_int64_reference_at_the_bounds(mag, m, n, mode):
    rng = np.random.default_rng(mag * 7 + m)
    pairs = families(rng, m, n)
    if m * n > 300_000:
        pairs = pairs[:4] + pairs[-1:]  # (the int64 reference is a python loop over rows)
    for kw in magnitude_scorings(mag):
        got = oracle_scores(kw, mode, pairs)
        want = [gotoh_score(x, y, mode, **kw) for x, y in pairs]
        assert got == want, (kw, mode, m, n)
        assert all(abs(w) <= mag * (m + n + 2) for w in want)


@pytest.mark.parametrize("mode", ["global", "semiglobal", "local"])
def test_oracle_scores_equal_int64_reference_on_ties(mode):
    rng = np.random.default_rng(3)
    pairs = families(rng, 120, 120) + families(rng, 7, 300) + families(rng, 384, 384)[:3]
    for kw in TIE_SCORINGS:
        assert oracle_scores(kw, mode, pairs) == [gotoh_score(x, y, mode, **kw) for x, y in pairs], (kw, mode)
