// The rescue rule's plan entry and its acceptance test (include/biogpu.h, "Mate rescue": accepted, choice) as device code, shared
// by the rescue stages (seed_rescue.hip: R4 picks with it) and the mapping quality of rescued pairs (seed_rescueq.hip: it finds
// the chosen rescue again and every other accepted one), so that there is one statement of both.
#ifndef BG_SEED_RESCUE_RULE_H
#define BG_SEED_RESCUE_RULE_H
#include "seed_pair_rule.h"

namespace bgpair {

constexpr uint32_t kSlots = 2 * BG_RESCUE_MAX_ANCHORS;  // rescue alignments of one pair: up to A per anchoring mate

// one planned rescue alignment; entry k of pair p is plan[kSlots * p + k]
struct RescuePlan {
    uint64_t lo;    // the window's first text offset
    uint32_t len;   // its length, 1 ..= max_span
    uint32_t info;  // anchor candidate relative to cb[0] (bits 0-12) | x's virtual read within the pair << 16 | rank << 18 |
                    // anchor on the forward strand << 20 | anchoring mate << 21
};

struct RescuePrm {
    uint32_t max_anchors;
    int32_t min_score;
    uint64_t n_text;
};

// Planned rescue `slot` of a pair (plan entry e, its alignment q, the pair's first candidate cb0): 0 if it is not accepted,
// otherwise the key whose maximum over the pair's slots is the rule's choice: the score sum biased to unsigned (33 bits), 1 for
// orientation A, 1 for the rescue anchored on m1, ~rank (2 bits), the slot.
__device__ __forceinline__ uint64_t rescue_key(const SeedPass& P, const RescuePlan& e, const bg_alignment_t& q, uint32_t slot, uint64_t cb0,
                                               const PairPrm& pp, int32_t min_score) {
    const uint64_t ca = cb0 + (e.info & 0x1FFF);
    const bool fwd = (e.info >> 20) & 1;
    const uint32_t m = (e.info >> 21) & 1;
    const uint64_t as = P.w_lo[ca] + P.aln[ca].ystart, ae = P.w_lo[ca] + P.aln[ca].yend;
    const uint64_t qs = e.lo + q.ystart, qe = e.lo + q.yend;
    const uint64_t f_start = fwd ? as : qs, b_start = fwd ? qs : as;  // the forward one is `a`, the reverse one `b`
    const uint64_t span = max(ae, qe) - f_start;
    if (!(q.score >= min_score && f_start <= b_start && span >= pp.min_span && span <= pp.max_span)) return 0;
    const uint64_t sum = (uint64_t)((int64_t)P.aln[ca].score + q.score + (1ll << 32));
    const bool orient_a = fwd == (m == 0);  // m1 forward: m1 anchors forward, or m2 anchors in reverse
    return sum << 8 | (uint64_t)orient_a << 7 | (uint64_t)(m == 0) << 6 | (3u - ((e.info >> 18) & 3)) << 4 | slot;
}

// the score sum of a rescue_key
__device__ __forceinline__ int64_t rescue_key_sum(uint64_t key) { return (int64_t)(key >> 8) - (1ll << 32); }

}  // namespace bgpair

#endif
