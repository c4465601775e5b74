"""Inputs of the mate rescue tests and the CPU expectation for them (no GPU needed: tests/rescue_oracle.py on the oracle's calls)."""
import numpy as np

import oracle_py as orc
import pair_oracle as po
import rescue_oracle as ro
from rust_bio_amd import synth
from rust_bio_amd.alphabets import dna
from rust_bio_amd.bwt import bwt, less
from rust_bio_amd.suffix_array import suffix_array

ALPHA = b"ACGTNacgtn$"
SC = (-5, -1, 1, -1)
L = 150
# A placed 150 bp mate with 10 % substitutions scores 150 - 2 * 15 = 120 under SC; a random 150-mer against a window matches a
# quarter of its bases at best a little more (score around -75 ungapped, every gap costs 6).  Half the read length separates the
# two with room on both sides.
MIN_SCORE = L // 2


def genome(n_text=200_000, seed=31):
    """the pairs generator's genome: random, one 400 bp repeat (10 000 and 50 000)"""
    g = synth.random_dna(n_text, seed=seed).copy()
    g[50_000:50_400] = g[10_000:10_400]
    return g, np.append(g, np.uint8(ord("$")))


def flat_of(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return (np.ascontiguousarray(np.concatenate(seqs)) if len(seqs) and off[-1] else np.zeros(0, np.uint8)), off


def other_base(x):
    """a different base for every byte of x"""
    return np.where(x == ord("A"), ord("C"), np.where(x == ord("C"), ord("G"), np.where(x == ord("G"), ord("T"), ord("A")))).astype(np.uint8)


def seed_broken(ref):
    """a substitution every 15 bases from base 7: every 20-base window holds one (no seed of length 20 survives, on either
    strand: the set of positions is its own mirror image in a 150 bp read)"""
    out = ref.copy()
    pos = np.arange(7, len(ref), 15)
    out[pos] = other_base(out[pos])
    return out


def planted_pairs(g, s, frag, swap, light=None, seed=1, break_mate2=True):
    """pairs from fragments g[s .. s + frag): mate 1 its first L bases (two substitutions where `light`), mate 2 the revcomp of its
    last L bases, seed-broken; swapped where `swap` (orientation B).  Returns (list of reads, origin of each read's alignment,
    which read of each pair is the seed-broken one)."""
    rng = np.random.default_rng(seed)
    reads, org, broken = [], [], []
    for k, (a, f) in enumerate(zip(s, frag)):
        a, f = int(a), int(f)
        m1 = g[a:a + L].copy()
        if light is not None and light[k]:
            q = rng.choice(np.arange(40, 110), size=2, replace=False)
            m1[q] = other_base(m1[q])
        ref2 = g[a + f - L:a + f]
        m2 = np.frombuffer(dna.revcomp((seed_broken(ref2) if break_mate2 else ref2).tobytes()), np.uint8)
        pair, o = [m1, m2], [a, a + f - L]
        if swap[k]:
            pair, o = pair[::-1], o[::-1]
        reads += pair
        org += o
        broken.append(0 if swap[k] else 1)
    return reads, np.array(org, np.int64), np.array(broken)


def case_rescue(n_pairs=240):
    """test 1: fragments of 400 bp away from the repeat, half swapped, half with a lightly mutated mate 1, some touching the text's
    first and last bytes"""
    g, text = genome()
    rng = np.random.default_rng(17)
    n = len(g)
    s = rng.integers(60_000, n - 2_000, size=n_pairs)
    s[:6] = [0, 3, 200, n - 400, n - 402, n - 700]
    frag = np.full(n_pairs, 400)
    swap = np.arange(n_pairs) % 2 == 1
    light = (np.arange(n_pairs) // 2) % 2 == 1
    reads, org, broken = planted_pairs(g, s, frag, swap, light, seed=2)
    flat, off = flat_of(reads)
    return g, text, flat, off, org, broken


def index_of(text):
    sa = suffix_array(text)
    b = bwt(text, sa)
    return sa, b, less(b, ALPHA)


def oracle_rescue(b, ls, sa, text, n_text, reads, off, pp, rp, scores=SC, **kw):
    """(expected reads, expected pairs, rescued, rescue alignments run, the paired call's expectation (reads, pairs), candidates,
    seed hits per virtual read)"""
    occ = orc.Occ(b, 64, ALPHA)
    vr, voff = po.virtual_reads(reads, off)
    sc = orc.make_scoring(*scores)
    cands, nh = po.candidates(orc, b, ls, occ, sa, text, n_text, sc, vr, voff, **kw)
    n_pairs = (len(off) - 1) // 2
    er, ep, rescued, n_al = ro.expected(orc, sc, cands, nh, vr, voff, text, n_text, n_pairs, pp.min_span, pp.max_span, pp.pen_unpaired,
                                        rp.max_anchors, rp.min_score)
    plain = po.expected(cands, nh, n_pairs, pp.min_span, pp.max_span, pp.pen_unpaired)
    return er, ep, rescued, n_al, plain, cands, nh
