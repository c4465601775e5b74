// The tiered call's choice between a re-seeded read's two tier winners (include/biogpu.h, "answer of a re-seeded read") as one
// function, used by se_reseed_merge_kernel (seed_tiered.hip).  It needs nothing but <stdint.h>, so a host compiler can include
// it as well (tests/test_tiered_rule.py holds it to the Python statement of the rule).
#ifndef BG_SEED_TIER_RULE_H
#define BG_SEED_TIER_RULE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define BG_TIER_FN __host__ __device__ __forceinline__
#else
#define BG_TIER_FN inline
#endif

namespace bgtier {

constexpr uint8_t kStrandNone = 255;  // BG_HIT_NONE: the tier has no hit for this read

// a tier's winner as the rule sees it: its score, its strand (BG_HIT_FORWARD 0, BG_HIT_REVERSE 1, BG_HIT_NONE 255) and the
// text offset of its window
struct TierHit {
    int32_t score;
    uint8_t strand;
    uint64_t window_start;
};

// true when tier 2's winner is the read's answer.  A tier without a hit loses to one with a hit (both without: tier 1); then
// the higher score, then the forward strand, then the smaller window_start, then tier 1.
BG_TIER_FN bool tier2_wins(const TierHit& t1, const TierHit& t2) {
    if (t2.strand == kStrandNone) return false;
    if (t1.strand == kStrandNone) return true;
    if (t2.score != t1.score) return t2.score > t1.score;
    if (t2.strand != t1.strand) return t2.strand < t1.strand;
    return t2.window_start < t1.window_start;
}

}  // namespace bgtier

#endif
