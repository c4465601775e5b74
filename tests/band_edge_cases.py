"""Sequence pairs that sit on the hard limits of the device band builder (rust-bio_amd/csrc/band_device.hip, B1-B4):
the match caps, the per-k-mer cap, the join flavours' size limits, the raster tile, the tree placement's batch size.

Generators only: numpy, nothing of the GPU, deterministic by seed.  tests/test_band_edge_cases.py proves with the CPU
oracle that every pair holds what it is for (and that the constants below still equal the ones in the sources);
tests/test_gpu_band_builder_edges.py runs the pairs through both builders.  k = 16, w = 32 (the benchmark's banded
configuration) unless a caller says otherwise."""
import itertools

import numpy as np

K, W = 16, 32

# Copies of the builder's limits.  test_band_edge_cases.py reads the originals out of band_device.h / band_device.hip:
# a cap that moves there breaks that test instead of silently moving these pairs off their edge.
MAX_CHAIN_MATCHES = 4095       # kMaxChainMatches
SMALL_CHAIN_MATCHES = 2047     # kSmallChainMatches
MAX_MATCHES_PER_KMER = 32      # kMaxMatchesPerKmer
CHAIN_GLOBAL_MIN_PAIRS = 1024  # kChainGlobalMinPairs
BAND_TILE = 2048               # kBandTile
STAGE_MAX_BYTES = 40960        # kStageMaxBytes
LDS_JOIN_MAX_BYTES = 150 * 1024  # launch_band_match
LDS_JOIN_TABLE = 8192          # kLdsJoinTable

MATCH_COUNTS = (1, 2047, 2048, 4095, 4096)
PER_KMER_COPIES = (32, 33)
NO_MATCH_M = (1, 15, 16, 17, 31, 33)
NO_MATCH_N = (15, 16, 17, 33)
TILE_N = (2047, 2048, 2049, 4095, 4096, 4097)
LONG_L = (20128, 20129, 20464, 20465)
LONG_FLAVOUR = {20128: "lds", 20129: "staged", 20464: "staged", 20465: "unstaged"}

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_NEXT = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"CGTA"):
    _NEXT[_a] = _b


# ---- launch_band_match's three size formulas, restated
def _up(v, a):
    return (v + a - 1) // a * a


def lds_join_bytes(m, n):
    return _up(m, 16) + _up(n, 16) + 4 * LDS_JOIN_TABLE + 2 * _up(n, 8) * 2 + 64


def stage_bytes(m, n):
    return _up(m, 16) + n + 16


def join_flavour(max_m, max_n, join_global=False):
    """the k-mer join a sub-batch with these longest x / y gets"""
    if max_n < 0xFFFF and lds_join_bytes(max_m, max_n) <= LDS_JOIN_MAX_BYTES and not join_global:
        return "lds"
    return "staged" if stage_bytes(max_m, max_n) <= STAGE_MAX_BYTES else "unstaged"


def handed_over(total, per_x_max):
    """the device builder gives such a pair back to the host builder"""
    return total > MAX_CHAIN_MATCHES or per_x_max > MAX_MATCHES_PER_KMER


def match_stats(find_kmer_matches, x, y, k=K):
    """(matches, most matches of one x position) from a find_kmer_matches(x, y, k) -> [(x, y)]"""
    mm = np.asarray(find_kmer_matches(x, y, k)).reshape(-1, 2)
    if len(mm) == 0:
        return 0, 0
    return len(mm), int(np.bincount(mm[:, 0].astype(np.int64)).max())


# ---- pairs
class Pair:
    """kind: zero (no match), handed (the device gives it back), full (exactly 4095 matches), small, tile, long"""

    def __init__(self, name, kind, x, y):
        self.name, self.kind = name, kind
        self.x, self.y = np.ascontiguousarray(x, dtype=np.uint8).tobytes(), np.ascontiguousarray(y, dtype=np.uint8).tobytes()

    def __repr__(self):
        return f"Pair({self.name}, {self.kind}, m={len(self.x)}, n={len(self.y)})"


def _dna(rng, n, letters=_ACGT):
    return letters[rng.integers(0, len(letters), size=n)]


def match_count_pair(c, seed=0, k=K):
    """x = y = random ACGT of c + k - 1 bases: c matches, one per x position"""
    s = _dna(np.random.default_rng([101, c, seed]), c + k - 1)
    kind = "handed" if c > MAX_CHAIN_MATCHES else "full" if c == MAX_CHAIN_MATCHES else "small"
    return Pair(f"matches{c}.{seed}", kind, s, s)


def per_kmer_pair(r, seed=0, k=K, left=300, right=300):
    """One k-mer of x (drawn from ACG) stands r times in y, the copies separated by a T; around it both reads carry the
    same random flanks, which do not touch the unit with a T."""
    rng = np.random.default_rng([102, r, seed])
    unit = _dna(rng, k, _ACGT[:3])
    lf, rf = _dna(rng, left), _dna(rng, right)
    if lf[-1] == ord("T"):
        lf[-1] = ord("A")
    if rf[0] == ord("T"):
        rf[0] = ord("A")
    x = np.concatenate([lf, unit, rf])
    y = np.concatenate([lf, unit] + [np.concatenate([_ACGT[3:], unit])] * (r - 1) + [rf])
    return Pair(f"copies{r}.{seed}", "handed" if r > MAX_MATCHES_PER_KMER else "small", x, y)


def no_match_pairs():
    """(m, n) around k, a read shorter than k among them — x over AC, y over GT — and two unrelated 300-base reads"""
    out = []
    for i, (m, n) in enumerate(itertools.product(NO_MATCH_M, NO_MATCH_N)):
        rng = np.random.default_rng([103, i])
        out.append(Pair(f"nomatch{m}x{n}", "zero", _dna(rng, m, _ACGT[:2]), _dna(rng, n, _ACGT[2:])))
    for i in range(2):
        rng = np.random.default_rng([104, i])
        out.append(Pair(f"unrelated300.{i}", "zero", _dna(rng, 300), _dna(rng, 300)))
    return out


def tile_pair(n, mutated, seed=0):
    """y of n bases around the raster tile.  Identical reads: one anchor and a run of n - k continuations.  Mutated: x
    is y with a substitution every 20th base, every eighth of them (160 bases) a deleted base instead — many anchors,
    gaps with different row and column counts.  The substitutions' phase leaves y's last k bases alone, so a match ends
    in column n, and (checked by the CPU test) one covers column 2048 and column 4096 where y has it."""
    y = _dna(np.random.default_rng([105, n, seed]), n)
    if not mutated:
        return Pair(f"tile{n}.same", "tile", y, y)
    pos = np.arange(n % 20, n, 20)
    x = y.copy()
    x[pos] = _NEXT[y[pos]]
    x = np.delete(x, pos[3::8])
    return Pair(f"tile{n}.mut", "tile", x, y)


def long_pair(length, period=20, seed=0):
    """x = y of `length` bases with a substitution every `period`-th base"""
    y = _dna(np.random.default_rng([106, length, seed]), length)
    x = y.copy()
    pos = np.arange(period - 1, length, period)
    x[pos] = _NEXT[y[pos]]
    return Pair(f"long{length}", "long", x, y)


def small_pair(m, n, seed=0):
    """a read and a prefix of it (m, n >= 40 bases) with one substitution in the middle of the shorter"""
    rng = np.random.default_rng([107, seed])
    s = _dna(rng, max(m, n))
    t = s[:min(m, n)].copy()
    t[len(t) // 2] = _NEXT[t[len(t) // 2]]
    return Pair(f"small{m}x{n}.{seed}", "small", s if m >= n else t, t if m >= n else s)


N_QUADS = 26
HANDED_RUN = 9


def short_batch():
    """Every family but the long pairs, in a fixed order of 129 pairs (1 mod 4):

      [0, 104)    26 quads (zero, handed, full, small): every four consecutive pairs hold one of each — the four rows of
                  a chain_rows_kernel wavefront finish at very different times.  The handed-over pair alternates between
                  4096 matches and 33 copies of a k-mer.  The small pair's lengths are chosen so that the next quad's
                  zero-match pair starts at residue q mod 16 of the concatenated x and 7 q mod 16 of y: the no-match family
                  takes every residue in both buffers (head / vector / tail paths of stage_bytes).
      [104, 113)  nine handed-over pairs in a row: with chunk_pairs 4 or 5 some sub-batch holds nothing else
      [113, 129)  the twelve raster-tile pairs and the small pairs on the caps (1, 2047, 2048 matches, 32 copies): no
                  handed-over pair, so some sub-batch holds none
    """
    zero = no_match_pairs()
    assert len(zero) == N_QUADS
    pairs, xo, yo = [], 0, 0

    def add(p):
        nonlocal xo, yo
        pairs.append(p)
        xo += len(p.x)
        yo += len(p.y)

    for q in range(N_QUADS):
        assert (xo % 16, yo % 16) == (q % 16, 7 * q % 16)
        add(zero[q])
        add(match_count_pair(4096, seed=q) if q % 2 == 0 else per_kmer_pair(33, seed=q, left=200 + 7 * q, right=250 - 3 * q))
        add(match_count_pair(4095, seed=q))
        m, n = 48 + 5 * q, 48 + 3 * q
        m += (q + 1 - (xo + m)) % 16
        n += (7 * (q + 1) - (yo + n)) % 16
        add(small_pair(m, n, seed=q))
    for i in range(HANDED_RUN):
        add(per_kmer_pair(33, seed=100 + i, left=150 + 11 * i, right=97 + 5 * i) if i % 2 == 0 else match_count_pair(4096, seed=100 + i))
    for n in TILE_N:
        add(tile_pair(n, False))
        add(tile_pair(n, True))
    add(match_count_pair(1))
    add(match_count_pair(2047))
    add(match_count_pair(2048))
    add(per_kmer_pair(32))
    return pairs


def zero_match_starts(pairs):
    """[(x start mod 16, y start mod 16)] of the no-match pairs inside the concatenated buffers of `pairs`"""
    out, xo, yo = [], 0, 0
    for p in pairs:
        if p.kind == "zero":
            out.append((xo % 16, yo % 16))
        xo += len(p.x)
        yo += len(p.y)
    return out


def sub_batches(n_pairs, chunk_pairs):
    """[(first pair, pairs)] of the sub-batches of a call: the remainder goes first (banded_api.hip: band_want)"""
    out, p0 = [], 0
    rem = n_pairs % chunk_pairs if n_pairs > chunk_pairs else 0
    while p0 < n_pairs:
        want = rem if p0 == 0 and rem else min(chunk_pairs, n_pairs - p0)
        out.append((p0, want))
        p0 += want
    return out


def many_small_pairs(count, seed=0):
    """`count` pairs of 60-120 bases, the read a copy of the reference with two substitutions (pair i is the same for
    every count)"""
    out = []
    for i in range(count):
        rng = np.random.default_rng([108, seed, i])
        n = int(rng.integers(60, 121))
        y = _dna(rng, n)
        x = y.copy()
        pos = rng.integers(0, n, size=2)
        x[pos] = _NEXT[y[pos]]
        out.append(Pair(f"tiny{i}", "small", x, y))
    return out
