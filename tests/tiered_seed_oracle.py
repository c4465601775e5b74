"""CPU statement of tiered seed-and-extend (include/biogpu.h, bg_seed_extend_tiered_batch), for the tests.

Tier 1 is the SMEM statement (smem_seed_oracle.candidates) with its seeds replaced: `WindowSeeds` stands where the oracle's
FMDIndex stands there and answers all_smems with the read's fixed windows, each searched with `oracle_py.backward_search` on the
BWT of T$R$.  Tier 2 is smem_seed_oracle.candidates itself on the re-seeded reads.  `better` is the choice between a read's two
tier winners, `tiered` the whole call."""
import numpy as np

import smem_seed_oracle as sso

MIN_SCORE = sso.MIN_SCORE
INT32_MAX = 2**31 - 1
TIER_NONE, TIER_FIRST, TIER_SECOND = 0, 1, 2
OK, OUT_OF_ALPHABET, OPS_CAP = 0, -7, -9
ABSENT = (MIN_SCORE, sso.HIT_NONE, sso.SA_NONE)  # a tier without a hit, as `better` takes it


class WindowSeeds:
    """The windows read[o .. o + seed_len), o = 0, stride, ... while they fit, as all_smems-shaped records ((lower, lower_rev,
    size, match_size), a, len): size = upper - lower of a Complete backward_search, 0 of a Partial or Absent one and of a window
    that reaches a byte outside the alphabet (counted in `panics`: it does not vote, the read's other windows do)."""

    def __init__(self, orc, bwt, less, occ, seed_len, stride):
        self.orc, self.bwt, self.less, self.occ, self.seed_len, self.stride = orc, bwt, less, occ, seed_len, stride
        self.panics = 0

    def all_smems(self, read, _min_len):
        recs = []
        for o in range(0, len(read) - self.seed_len + 1, self.stride):
            tag, lo, hi, _ = self.orc.backward_search(self.bwt, self.less, self.occ, read[o:o + self.seed_len])
            self.panics += tag == "panic"
            size = hi - lo if tag == "complete" else 0
            recs.append(((lo if size else 0, 0, size, self.seed_len), o, self.seed_len))
        return recs


def tier1(orc, index, fwd, sc, reads, off, strands=sso.STRAND_BOTH, seed_len=20, stride=10, max_occ=16, pad=25):
    """index: (bwt of T$R$, less, oracle Occ, suffix array).  Returns (a smem_seed_oracle.candidates result, windows that panicked)."""
    bwt, less, occ, sa = index
    seeds = WindowSeeds(orc, bwt, less, occ, seed_len, stride)
    res = sso.candidates(orc, seeds, sa, fwd, sc, reads, off, strands=strands, min_seed_len=seed_len, max_smems=1 << 30, max_occ=max_occ,
                         pad=pad)
    assert not res["truncated"].any() and not res["panicked"].any()  # tier 1 has neither
    return res, seeds.panics


def better(t1, t2):
    """True when tier 2's winner is the answer; t1, t2: (score, strand, window_start), or ABSENT.  A tier without a hit loses to
    one with a hit; then the higher score, the forward strand, the smaller window_start, tier 1."""
    if t2[1] == sso.HIT_NONE:
        return False
    if t1[1] == sso.HIT_NONE:
        return True
    return (-t2[0], t2[1], t2[2]) < (-t1[0], t1[1], t1[2])


def _key(e):
    return ABSENT if e[1] is None else (e[1]["score"], e[0], e[1]["wlo"])


def tiered(orc, index, ofmd, fwd, sc, reads, off, strands=sso.STRAND_BOTH, window=None, smem=None, reseed_below=MIN_SCORE):
    """window: dict(seed_len, stride, max_occ, pad), smem: dict(min_seed_len, max_smems, max_occ, pad); ofmd: the oracle's FMDIndex
    over T$R$.  Returns a dict: want — per read (strand, candidate or None, n_candidates, n_seed_hits) as smem_seed_oracle.expected
    —, tier, totals (3), status, and first — tier 1's own `expected`."""
    window = dict(dict(seed_len=20, stride=10, max_occ=16, pad=25), **(window or {}))
    smem = dict(dict(min_seed_len=19, max_smems=16, max_occ=16, pad=25), **(smem or {}))
    assert window["pad"] == smem["pad"]
    reads = np.ascontiguousarray(reads, np.uint8)
    n = len(off) - 1
    res1, panics = tier1(orc, index, fwd, sc, reads, off, strands, **window)
    first = sso.expected(res1)
    again = [r for r in range(n) if _key(first[r])[0] < reseed_below]
    want, tier = list(first), np.zeros(n, np.uint8)
    rows, status = res1["rows"], OUT_OF_ALPHABET if panics else OK
    if again:
        pieces = [reads[int(off[r]):int(off[r + 1])] for r in again]
        off2 = np.zeros(len(again) + 1, np.uint64)
        off2[1:] = np.cumsum([len(p) for p in pieces])
        res2 = sso.candidates(orc, ofmd, index[3], fwd, sc, np.concatenate(pieces), off2, strands=strands, **smem)
        second = sso.expected(res2)
        rows += res2["rows"]
        if res2["panicked"].any():
            status = OUT_OF_ALPHABET
        elif res2["truncated"].any() and status == OK:
            status = OPS_CAP
        for j, r in enumerate(again):
            e1, e2 = first[r], second[j]
            win = better(_key(e1), _key(e2))
            tier[r] = TIER_SECOND if win else TIER_FIRST
            want[r] = ((e2 if win else e1)[0], (e2 if win else e1)[1], e1[2] + e2[2], e1[3] + e2[3])
    return {"want": want, "tier": tier, "totals": (rows, sum(w[2] for w in want), len(again)), "status": status, "first": first}
