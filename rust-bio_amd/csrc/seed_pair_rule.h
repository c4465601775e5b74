// The pair rule of bg_seed_extend_pairs_batch[_dev] (include/biogpu.h, "Read pairs") as device functions, shared by the pair
// stages (seed_pairs.hip, seed_pairq.hip) and the rescue stages (seed_rescue.hip, seed_rescueq.hip): one pair per group of 16
// lanes, on the pass view of seed_pass.h (pair p: virtual reads 4p .. 4p + 3 = m1, rc(m1), m2, rc(m2)).
#ifndef BG_SEED_PAIR_RULE_H
#define BG_SEED_PAIR_RULE_H
#include "seed_rule.h"

namespace bgpair {

using namespace bgseed;

struct PairPrm {
    uint64_t min_span, max_span;
    int64_t pen_unpaired;
};
inline PairPrm pair_prm(const bg_pair_params_t* pp) { return PairPrm{pp->min_span, pp->max_span, pp->pen_unpaired}; }

// What the rule finds for one pair, the same in every lane of its group.
struct PairRule {
    uint64_t cb[5];   // candidate offsets of the pair's four virtual reads, and their end
    uint64_t own[2];  // each mate's own best over both strands (own_key; 0: the mate has no candidate)
    uint64_t best;    // key of the best proper combination: score sum biased to unsigned (33 bits), 1 for orientation A, ~i, ~j
    uint32_t n_proper;
};

// A proper combination: candidate i of the forward list `a` with candidate j of the reverse list `b` of orientation o
// (0: A, a is m1's; 1: B, a is m2's), their scores and text intervals.
struct ProperCombo {
    int o;
    uint32_t i, j;
    int32_t a_score, b_score;
    uint64_t a_start, a_end, b_start, b_end;
};

// Orientation A pairs m1's forward candidates (v = 0) with m2's reverse ones (v = 3), orientation B m2's forward ones (v = 2)
// with m1's reverse ones (v = 1).  The lanes of the group walk each orientation's product, strided over the longer list, and
// f sees every proper combination once, in one lane.  `on` false: nothing is walked.
template <typename F>
__device__ __forceinline__ void for_proper(const SeedPass& P, const uint64_t (&cb)[5], bool on, uint32_t l16, const PairPrm& pp, F&& f) {
#pragma unroll
    for (int o = 0; o < 2; o++) {
        const uint64_t fa = cb[o == 0 ? 0 : 2], fb = cb[o == 0 ? 3 : 1];
        const uint32_t na = on ? (uint32_t)(cb[o == 0 ? 1 : 3] - fa) : 0, nb = on ? (uint32_t)(cb[o == 0 ? 4 : 2] - fb) : 0;
        const bool lanes_on_a = na > nb;
        const uint32_t n_out = lanes_on_a ? nb : na, n_in = lanes_on_a ? na : nb;
        for (uint32_t u = 0; u < n_out; u++) {
            for (uint32_t w = l16; w < n_in; w += 16) {
                const uint32_t i = lanes_on_a ? w : u, j = lanes_on_a ? u : w;
                const bg_alignment_t& A = P.aln[fa + i];
                const bg_alignment_t& B = P.aln[fb + j];
                const uint64_t a_start = P.w_lo[fa + i] + A.ystart, b_start = P.w_lo[fb + j] + B.ystart;
                if (a_start > b_start) continue;
                const uint64_t a_end = P.w_lo[fa + i] + A.yend, b_end = P.w_lo[fb + j] + B.yend;
                const uint64_t span = max(a_end, b_end) - a_start;
                if (span < pp.min_span || span > pp.max_span) continue;
                f(ProperCombo{o, i, j, A.score, B.score, a_start, a_end, b_start, b_end});
            }
        }
    }
}

// One key per proper combination (10 bits per candidate index: both below kMaxCand), so the max is the rule's best.
__device__ __forceinline__ PairRule pair_rule(const SeedPass& P, uint64_t p, uint32_t l16, const PairPrm& pp) {
    PairRule R;
#pragma unroll
    for (int v = 0; v < 5; v++) R.cb[v] = P.coff[4 * p + v];
    // each mate's own best over both strands: highest score, forward strand on a tie, smallest start
#pragma unroll
    for (int m = 0; m < 2; m++) {
        const uint64_t c0 = R.cb[2 * m];
        const uint32_t nc = (uint32_t)(R.cb[2 * m + 2] - c0);
        uint64_t best = 0;
        for (uint32_t c = l16; c < nc; c += 16) best = max(best, own_key(P.aln[c0 + c].score, c));
        R.own[m] = max16(best);
    }
    uint64_t best = 0;
    uint32_t n_proper = 0;
    for_proper(P, R.cb, true, l16, pp, [&](const ProperCombo& k) {
        n_proper++;
        const uint64_t sum = (uint64_t)((int64_t)k.a_score + k.b_score + (1ll << 32));
        best = max(best, sum << 21 | (uint64_t)(k.o == 0) << 20 | (uint64_t)(kMaxCand - 1 - k.i) << 10 | (kMaxCand - 1 - k.j));
    });
    R.best = max16(best);
#pragma unroll
    for (int o = 8; o; o >>= 1) n_proper += (uint32_t)__shfl_xor((int)n_proper, o, 16);
    R.n_proper = n_proper;
    return R;
}

// "Paired or not" (rule 4): the best proper combination, if it gives up at most pen_unpaired against the mates' own bests.
struct PairChoice {
    bool proper;
    uint32_t pick[2];  // the candidate each mate reports, relative to cb[2m]: the combination's member, or the mate's own best
    int64_t pair_sum;  // proper: the combination's score sum
    uint64_t span;     // proper: its span
};
__device__ __forceinline__ PairChoice pair_choice(const SeedPass& P, const PairRule& R, const PairPrm& pp) {
    PairChoice ch{false, {key_cand(R.own[0]), key_cand(R.own[1])}, 0, 0};
    if (R.n_proper) {
        const int64_t pair_sum = (int64_t)(R.best >> 21) - (1ll << 32);
        if (pair_sum + pp.pen_unpaired >= (int64_t)key_score(R.own[0]) + key_score(R.own[1])) {
            ch.proper = true;
            ch.pair_sum = pair_sum;
            const bool orient_a = (R.best >> 20) & 1;
            const uint32_t i = kMaxCand - 1 - (uint32_t)((R.best >> 10) & (kMaxCand - 1));
            const uint32_t j = kMaxCand - 1 - (uint32_t)(R.best & (kMaxCand - 1));
            const uint64_t ca = (orient_a ? R.cb[0] : R.cb[2]) + i, cr = (orient_a ? R.cb[3] : R.cb[1]) + j;  // forward, reverse
            ch.span = max(P.w_lo[ca] + P.aln[ca].yend, P.w_lo[cr] + P.aln[cr].yend) - (P.w_lo[ca] + P.aln[ca].ystart);
            ch.pick[0] = (uint32_t)((orient_a ? ca : cr) - R.cb[0]);
            ch.pick[1] = (uint32_t)((orient_a ? cr : ca) - R.cb[2]);
        }
    }
    return ch;
}

// Mate m of pair p (caller read r0 + 2p + m) reports candidate `pick` of its own (relative to cb[2m]; a mate without
// candidates is written like an unmapped read) exactly as se_best_kernel<2> writes a winner.
__device__ __forceinline__ void write_mate(const SeedPass& P, const SeedOut& O, uint64_t p, int m, uint32_t l16, const PairRule& R,
                                           uint32_t pick) {
    const uint64_t c0 = R.cb[2 * m];
    const uint32_t nc = (uint32_t)(R.cb[2 * m + 2] - c0);
    const uint8_t won = !nc ? BG_HIT_NONE : pick >= R.cb[2 * m + 1] - c0 ? BG_HIT_REVERSE : BG_HIT_FORWARD;
    write_cand(P, O, P.r0 + 2 * p + m, l16, c0 + pick, won, nc, P.n_hits[4 * p + 2 * m] + P.n_hits[4 * p + 2 * m + 1]);
}

// The writes of the paired call: a mate that is not part of a proper pair reports exactly what se_best_kernel<2> writes for it.
__device__ __forceinline__ void pair_write(const SeedPass& P, const SeedOut& O, uint64_t p, uint32_t l16, const PairRule& R,
                                           const PairChoice& ch) {
#pragma unroll
    for (int m = 0; m < 2; m++) write_mate(P, O, p, m, l16, R, ch.pick[m]);
    if (l16 == 0) {
        bg_pair_hit_t ph;
        memset(&ph, 0, sizeof(ph));
        ph.span = ch.span;
        ph.n_proper = R.n_proper;
        ph.proper = ch.proper ? 1 : 0;
        O.pairs[P.r0 / 2 + p] = ph;
    }
}

}  // namespace bgpair

#endif
