// The pair rule of bg_seed_extend_pairs_batch[_dev] (include/biogpu.h, "Read pairs") as device functions, shared by the pair
// stage (seed_pairs.hip) and the rescue stages (seed_rescue.hip): one pair per group of 16 lanes, on the pass scratch of
// seed_extend.hip (candidate offsets of the 4 n_pairs virtual reads m1, rc(m1), m2, rc(m2), their alignments, windows).
#ifndef BG_SEED_PAIR_RULE_H
#define BG_SEED_PAIR_RULE_H
#include "fm_kernels.h"

namespace bgpair {

constexpr uint32_t kMaxCand = 1024;  // candidates of one virtual read are below this: a candidate index fits in 10 key bits

struct PairPrm {
    uint64_t min_span, max_span;
    int64_t pen_unpaired;
};

// max of a 64-bit key over the 16 lanes of a group
__device__ __forceinline__ uint64_t max16(uint64_t v) {
#pragma unroll
    for (int o = 8; o; o >>= 1) {
        const uint64_t other = ((uint64_t)(uint32_t)__shfl_xor((int)(v >> 32), o, 16) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, o, 16);
        v = max(v, other);
    }
    return v;
}

// the score of an own-best key (se_best_kernel<2>'s key: score biased to unsigned in the high word, ~candidate in the low one)
__device__ __forceinline__ int32_t key_score(uint64_t key) { return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u); }

// What the rule finds for one pair, the same in every lane of its group.
struct PairRule {
    uint64_t cb[5];   // candidate offsets of the pair's four virtual reads, and their end
    uint64_t own[2];  // each mate's own best over both strands (own-best key; 0: the mate has no candidate)
    uint64_t best;    // key of the best proper combination: score sum biased to unsigned (33 bits), 1 for orientation A, ~i, ~j
    uint32_t n_proper;
};

// Orientation A pairs m1's forward candidates (v = 0) with m2's reverse ones (v = 3), orientation B m2's forward ones (v = 2)
// with m1's reverse ones (v = 1).  The lanes walk each orientation's product, strided over the longer list, with one key per
// combination (10 bits per candidate index: both below kMaxCand), so the max is the rule's best.
__device__ __forceinline__ PairRule pair_rule(uint64_t p, uint32_t l16, const PairPrm& pp, const uint64_t* __restrict__ coff,
                                              const bg_alignment_t* __restrict__ aln, const uint64_t* __restrict__ w_lo) {
    PairRule R;
#pragma unroll
    for (int v = 0; v < 5; v++) R.cb[v] = coff[4 * p + v];
    // each mate's own best over both strands: highest score, forward strand on a tie, smallest start
#pragma unroll
    for (int m = 0; m < 2; m++) {
        const uint64_t c0 = R.cb[2 * m];
        const uint32_t nc = (uint32_t)(R.cb[2 * m + 2] - c0);
        uint64_t best = 0;
        for (uint32_t c = l16; c < nc; c += 16) {
            const uint32_t sc = (uint32_t)aln[c0 + c].score ^ 0x80000000u;
            best = max(best, ((uint64_t)sc << 32) | (uint32_t)~c);
        }
        R.own[m] = max16(best);
    }
    // proper combinations of both orientations
    uint64_t best = 0;
    uint32_t n_proper = 0;
#pragma unroll
    for (int o = 0; o < 2; o++) {
        const uint64_t fa = R.cb[o == 0 ? 0 : 2], fb = R.cb[o == 0 ? 3 : 1];
        const uint32_t na = (uint32_t)(R.cb[o == 0 ? 1 : 3] - fa), nb = (uint32_t)(R.cb[o == 0 ? 4 : 2] - fb);
        const bool lanes_on_a = na > nb;
        const uint32_t n_out = lanes_on_a ? nb : na, n_in = lanes_on_a ? na : nb;
        for (uint32_t u = 0; u < n_out; u++) {
            for (uint32_t w = l16; w < n_in; w += 16) {
                const uint32_t i = lanes_on_a ? w : u, j = lanes_on_a ? u : w;
                const bg_alignment_t& A = aln[fa + i];
                const bg_alignment_t& B = aln[fb + j];
                const uint64_t a_start = w_lo[fa + i] + A.ystart, b_start = w_lo[fb + j] + B.ystart;
                if (a_start > b_start) continue;
                const uint64_t span = max(w_lo[fa + i] + A.yend, w_lo[fb + j] + B.yend) - a_start;
                if (span < pp.min_span || span > pp.max_span) continue;
                n_proper++;
                const uint64_t sum = (uint64_t)((int64_t)A.score + B.score + (1ll << 32));
                best = max(best, sum << 21 | (uint64_t)(o == 0) << 20 | (uint64_t)(kMaxCand - 1 - i) << 10 | (kMaxCand - 1 - j));
            }
        }
    }
    R.best = max16(best);
#pragma unroll
    for (int o = 8; o; o >>= 1) n_proper += (uint32_t)__shfl_xor((int)n_proper, o, 16);
    R.n_proper = n_proper;
    return R;
}

// Mate m of pair p (caller read r0 + 2p + m) reports candidate `pick` of its own (relative to cb[2m]; ignored when the mate
// has none: it is then written like an unmapped read) exactly as se_best_kernel<2> writes a winner: record, window,
// operations right-aligned in the read's slot, strand.
__device__ __forceinline__ void write_mate(uint64_t p, int m, uint32_t l16, uint64_t r0, const PairRule& R, uint64_t pick,
                                           const uint32_t* __restrict__ n_hits, const bg_alignment_t* __restrict__ aln,
                                           const uint8_t* __restrict__ c_ops, const uint64_t* __restrict__ w_lo,
                                           bg_seed_hit_t* __restrict__ hits, uint8_t* __restrict__ ops, uint64_t ops_stride,
                                           uint8_t* __restrict__ strand) {
    const uint64_t r = 2 * p + m;
    const uint64_t c0 = R.cb[2 * m];
    const uint32_t nc = (uint32_t)(R.cb[2 * m + 2] - c0);
    bg_seed_hit_t h;
    memset(&h, 0, sizeof(h));
    h.aln.score = BG_MIN_SCORE;
    h.window_start = h.ref_start = h.ref_end = ~0ull;
    h.n_candidates = nc;
    h.n_seed_hits = n_hits[4 * p + 2 * m] + n_hits[4 * p + 2 * m + 1];
    h.aln.ops_off = (r0 + r + 1) * ops_stride;
    uint8_t won = BG_HIT_NONE;
    if (nc) {
        const uint64_t c = pick;
        won = c >= R.cb[2 * m + 1] - c0 ? BG_HIT_REVERSE : BG_HIT_FORWARD;
        const bg_alignment_t a = aln[c0 + c];
        h.aln = a;
        h.aln.ops_off = (r0 + r + 1) * ops_stride - a.n_ops;
        h.window_start = w_lo[c0 + c];
        h.ref_start = w_lo[c0 + c] + a.ystart;
        h.ref_end = w_lo[c0 + c] + a.yend;
        if (ops && c_ops)
            for (uint32_t k = l16; k < a.n_ops; k += 16) ops[h.aln.ops_off + k] = c_ops[a.ops_off + k];
    }
    if (l16 == 0) {
        hits[r0 + r] = h;
        if (strand) strand[r0 + r] = won;
    }
}

// Rule 4 and the writes of the paired call: the best proper pair, if it gives up at most pen_unpaired against the mates' own
// bests; a mate that is not part of a proper pair reports exactly what se_best_kernel<2> writes for it.
__device__ __forceinline__ void pair_write(uint64_t p, uint32_t l16, uint64_t r0, const PairPrm& pp, const PairRule& R,
                                           const uint32_t* __restrict__ n_hits, const bg_alignment_t* __restrict__ aln,
                                           const uint8_t* __restrict__ c_ops, const uint64_t* __restrict__ w_lo,
                                           bg_seed_hit_t* __restrict__ hits, uint8_t* __restrict__ ops, uint64_t ops_stride,
                                           uint8_t* __restrict__ strand, bg_pair_hit_t* __restrict__ pairs) {
    bool proper = false;
    uint64_t pick[2] = {~(uint32_t)R.own[0], ~(uint32_t)R.own[1]};  // candidate per mate, relative to cb[2m]
    uint64_t span = 0;
    if (R.n_proper) {
        const int64_t pair_sum = (int64_t)(R.best >> 21) - (1ll << 32);
        const int64_t own_sum = (int64_t)key_score(R.own[0]) + key_score(R.own[1]);
        if (pair_sum + pp.pen_unpaired >= own_sum) {
            proper = true;
            const bool orient_a = (R.best >> 20) & 1;
            const uint32_t i = kMaxCand - 1 - (uint32_t)((R.best >> 10) & (kMaxCand - 1));
            const uint32_t j = kMaxCand - 1 - (uint32_t)(R.best & (kMaxCand - 1));
            const uint64_t ca = (orient_a ? R.cb[0] : R.cb[2]) + i, cr = (orient_a ? R.cb[3] : R.cb[1]) + j;  // forward, reverse
            const uint64_t a_start = w_lo[ca] + aln[ca].ystart;
            span = max(w_lo[ca] + aln[ca].yend, w_lo[cr] + aln[cr].yend) - a_start;
            pick[0] = (orient_a ? ca : cr) - R.cb[0];
            pick[1] = (orient_a ? cr : ca) - R.cb[2];
        }
    }
#pragma unroll
    for (int m = 0; m < 2; m++) write_mate(p, m, l16, r0, R, pick[m], n_hits, aln, c_ops, w_lo, hits, ops, ops_stride, strand);
    if (l16 == 0) {
        bg_pair_hit_t ph;
        memset(&ph, 0, sizeof(ph));
        ph.span = span;
        ph.n_proper = R.n_proper;
        ph.proper = proper ? 1 : 0;
        pairs[r0 / 2 + p] = ph;
    }
}

}  // namespace bgpair

#endif
