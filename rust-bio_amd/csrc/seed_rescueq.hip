// A mapping quality for rescued read pairs (bg_seed_extend_pairs_rescue_mapq_batch[_dev]): the stage that follows R4 of
// seed_rescue.hip when the rescue call is asked for bg_multi_hit_t records as well.  Before R1 the pass has written every pair's
// records as the pairs-mapq call writes them (bg_seed_pairq_launch); this stage rewrites the two records of the pairs R4 rescued,
// by the rule of include/biogpu.h, "Mapping quality of rescued read pairs".  It reads what R1-R4 left in the pass scratch: the
// plan, the rescue alignments and the rescued bytes.
#include "seed_rescue_rule.h"

namespace {

using namespace bgpair;

// 16 lanes per pair, pairs with rescued != 0 only (the others keep the records written before R1).
//   1. lane k < n holds planned rescue k of the pair: its key (rescue_key: 0 unless accepted), its anchor (a seeded candidate of
//      the anchoring mate) and its hit (a placement of the other mate).  The maximum key is R4's choice: anchor c_a, hit h,
//      S1 = their score sum.  The two mates' reported hits c_0, c_1 are those two, whichever way round.
//   2. per mate i, one strided walk over its seeded candidates of both strands: the best score among those >= min_score that do
//      not touch c_i.  It is the seeded part of sub_score and, with the partner's score less pen_unpaired, kind (b) of S2_i.
//   3. per mate i, every lane's own rescue, if accepted: its mate-i member (the anchor if it anchors on mate i, else the hit), if
//      it scores >= min_score and does not touch c_i, is an alternative: its score goes into sub_score, the rescue's sum is kind
//      (a) of S2_i.
//   4. lane 0 writes the two records; S1 - S2_i is clamped at 0 in signed arithmetic (a better seeded candidate of the anchor's
//      mate whose own rescue failed gives S2_i > S1 through (b)).
// No LDS, no atomics; every reduction is a max16 on a 64-bit key.
__global__ __launch_bounds__(256) void se_rescue_mapq_kernel(SeedPass P, SeedOut O, PairPrm pp, int32_t rescue_min_score, PairqPrm qp,
                                                             const RescuePlan* __restrict__ plan, SeedRescueAln res) {
    static_assert(kSlots <= 16, "one lane per planned rescue");
    const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t l16 = threadIdx.x & 15;
    if (p >= P.n) return;                // uniform per group of 16
    if (!O.rescued[P.r0 / 2 + p]) return;  // the same
    const uint64_t j0 = res.roff[p];
    const uint32_t n = (uint32_t)(res.roff[p + 1] - j0);
    uint64_t cb[5];
#pragma unroll
    for (int v = 0; v < 5; v++) cb[v] = P.coff[4 * p + v];
    // 1. this lane's rescue (without one: not accepted, and intervals that nothing reads)
    uint64_t key = 0, a_lo = 0, a_hi = 0, h_lo = 0, h_hi = 0;
    int32_t a_score = 0, h_score = 0;
    uint32_t am = 0;  // the anchoring mate
    if (l16 < n) {
        const RescuePlan e = plan[kSlots * p + l16];
        const bg_alignment_t& q = res.aln[j0 + l16];
        key = rescue_key(P, e, q, l16, cb[0], pp, rescue_min_score);
        const uint64_t ca = cb[0] + (e.info & 0x1FFF);
        am = (e.info >> 21) & 1;
        a_score = P.aln[ca].score;
        a_lo = P.w_lo[ca] + P.aln[ca].ystart;
        a_hi = P.w_lo[ca] + P.aln[ca].yend;
        h_score = q.score;
        h_lo = e.lo + q.ystart;
        h_hi = e.lo + q.yend;
    }
    const uint64_t chosen = max16(key);
    if (!chosen) return;  // (never: R4 rescued the pair through an accepted rescue)
    const int64_t S1 = rescue_key_sum(chosen);
    const uint32_t k = (uint32_t)chosen & 15;
    const bool anchor_m1 = __shfl((int)am, (int)k, 16) == 0;  // the chosen rescue anchors on m1: c_0 = c_a, c_1 = h
    const uint64_t ca_lo = bcast16(a_lo, k), ca_hi = bcast16(a_hi, k), ch_lo = bcast16(h_lo, k), ch_hi = bcast16(h_hi, k);
    const int32_t ca_score = __shfl(a_score, (int)k, 16), ch_score = __shfl(h_score, (int)k, 16);
    const uint64_t lo[2] = {anchor_m1 ? ca_lo : ch_lo, anchor_m1 ? ch_lo : ca_lo};
    const uint64_t hi[2] = {anchor_m1 ? ca_hi : ch_hi, anchor_m1 ? ch_hi : ca_hi};
    const int32_t cs[2] = {anchor_m1 ? ca_score : ch_score, anchor_m1 ? ch_score : ca_score};
    uint64_t seeded[2], member[2], through[2];  // best seeded alternative, best alternative among rescue members, kind (a)
#pragma unroll
    for (int i = 0; i < 2; i++) {
        // 2. the mate's seeded candidates elsewhere
        seeded[i] = best_elsewhere(P, l16, cb[2 * i], (uint32_t)(cb[2 * i + 2] - cb[2 * i]), lo[i], hi[i], qp.min_score);
        // 3. the mate-i member of this lane's rescue
        const bool is_anchor = am == (uint32_t)i;
        const int32_t y_score = is_anchor ? a_score : h_score;
        const uint64_t y_lo = is_anchor ? a_lo : h_lo, y_hi = is_anchor ? a_hi : h_hi;
        const bool alt = key != 0 && y_score >= qp.min_score && !(y_lo <= hi[i] && lo[i] <= y_hi);
        member[i] = max16(alt ? score_key(y_score) : 0);
        through[i] = max16(alt ? (key >> 8) + 1 : 0);  // the sum biased to unsigned, + 1 so that 0 means none
    }
    if (l16) return;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        bg_multi_hit_t mh;
        memset(&mh, 0, sizeof(mh));
        const uint64_t sub = max(seeded[i], member[i]);
        const bool other = sub != 0;
        mh.sub_score = other ? score_of(sub) : BG_MIN_SCORE;
        mh.n_loci = other ? 2 : 1;
        mh.n_reported = 1;
        const int64_t s1 = cs[i];
        int64_t num = s1;  // the score this mate's placement is ahead by, 0 ..= s1
        if (s1 > 0 && other) {
            // S2: the pair's best total with this mate elsewhere, through an accepted rescue or unpaired; one of the two exists
            int64_t s2 = INT64_MIN;
            if (seeded[i]) s2 = (int64_t)score_of(seeded[i]) + cs[1 - i] - pp.pen_unpaired;
            if (through[i]) s2 = max(s2, (int64_t)(through[i] - 1) - (1ll << 32));
            num = min(max(S1 - s2, (int64_t)0), s1);  // (S2 > S1 happens: include/biogpu.h)
        }
        mh.mapq = mapq_of(qp.mapq_cap, (uint64_t)num, s1);
        O.multi[P.r0 + 2 * p + i] = mh;
    }
}

}  // namespace

int bg_seed_rescueq_launch(const SeedPass& P, const SeedOut& O, const bg_pair_params_t* pp, const bg_rescue_params_t* rp,
                           const bg_pairq_params_t* qp, const void* d_plan, const SeedRescueAln& res, hipStream_t st) {
    if (P.n == 0) return BG_OK;
    se_rescue_mapq_kernel<<<dim3((unsigned)((P.n * 16 + 255) / 256)), dim3(256), 0, st>>>(
        P, O, pair_prm(pp), rp->min_score, PairqPrm{qp->min_score, qp->mapq_cap}, (const RescuePlan*)d_plan, res);
    BG_HIP(hipGetLastError());
    return BG_OK;
}
