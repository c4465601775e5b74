// A mapping quality for each mate of a read pair (bg_seed_extend_pairs_mapq_batch[_dev]): the stage that replaces S7 of
// seed_extend.hip in this mode.  It is the pair stage (seed_pairs.hip: the same rule and the same writes, from seed_pair_rule.h)
// plus one bg_multi_hit_t per mate.  A mate of a proper pair is judged against the pair: how much score the best placement
// of the PAIR loses when this mate goes to another locus (definition in include/biogpu.h, "Mapping quality of read pairs").
// A mate of a pair that is not proper is judged as the multi call judges a single read at K = 1.
#include "seed_pair_rule.h"

namespace {

using namespace bgpair;

struct PairqPrm {
    int32_t min_score;
    uint32_t mapq_cap;
};

// score (biased to unsigned) as a key of max16; 0: none
__device__ __forceinline__ uint64_t score_key(int32_t s) { return (uint64_t)((uint32_t)s ^ 0x80000000u) | 1ull << 32; }
__device__ __forceinline__ int32_t score_of(uint64_t key) { return (int32_t)((uint32_t)key ^ 0x80000000u); }

// S7 of the pairs-mapq call: 16 lanes per pair, pair p as in se_pair_kernel.
//   1. pair_rule + pair_write: hits, strand, operations and pairs, byte for byte the paired call's.
//   2. the locus each mate is judged against: the chosen combination's member (proper), or the mate's own best if it scores
//      >= min_score (not proper: locus 0 of the multi rule; `pick` is the multi rule's candidate number, forward strand first).
//   3. per mate, a linear walk over its candidates of both strands: the best score among those >= min_score that do not touch
//      that locus.  This is the multi rule's runner-up, and for a proper pair the mate's best alternative (sub_score, kind (b)).
//   4. proper pairs only: a second strided walk over both orientations' products, as pair_rule walks them, that keeps per mate
//      the highest score sum over proper combinations whose member of that mate is an alternative (kind (a)).  Groups whose
//      pair is not proper walk nothing (their bounds are 0) and stay in the reductions.
// No LDS, no atomics; every reduction is a max16 on a 64-bit key.
__global__ __launch_bounds__(256) void se_pairq_kernel(uint64_t n_pairs, uint64_t r0, PairPrm pp, PairqPrm qp,
                                                       const uint64_t* __restrict__ coff, const uint32_t* __restrict__ n_hits,
                                                       const bg_alignment_t* __restrict__ aln, const uint8_t* __restrict__ c_ops,
                                                       const uint64_t* __restrict__ w_lo, bg_seed_hit_t* __restrict__ hits,
                                                       uint8_t* __restrict__ ops, uint64_t ops_stride, uint8_t* __restrict__ strand,
                                                       bg_pair_hit_t* __restrict__ pairs, bg_multi_hit_t* __restrict__ multi) {
    const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t l16 = threadIdx.x & 15;
    if (p >= n_pairs) return;  // uniform per group of 16
    const PairRule R = pair_rule(p, l16, pp, coff, aln, w_lo);
    pair_write(p, l16, r0, pp, R, n_hits, aln, c_ops, w_lo, hits, ops, ops_stride, strand, pairs);

    // 2. "paired or not" as pair_write decides it, and each mate's locus
    bool proper = false;
    int64_t pair_sum = 0;
    uint32_t pick0 = ~(uint32_t)R.own[0], pick1 = ~(uint32_t)R.own[1];  // candidate per mate, relative to cb[2m]
    if (R.n_proper) {
        pair_sum = (int64_t)(R.best >> 21) - (1ll << 32);
        if (pair_sum + pp.pen_unpaired >= (int64_t)key_score(R.own[0]) + key_score(R.own[1])) {
            proper = true;
            const bool orient_a = (R.best >> 20) & 1;
            const uint32_t i = kMaxCand - 1 - (uint32_t)((R.best >> 10) & (kMaxCand - 1));
            const uint32_t j = kMaxCand - 1 - (uint32_t)(R.best & (kMaxCand - 1));
            const uint32_t fwd = i, rev = (uint32_t)((orient_a ? R.cb[3] - R.cb[2] : R.cb[1] - R.cb[0])) + j;
            pick0 = orient_a ? fwd : rev;
            pick1 = orient_a ? rev : fwd;
        }
    }
    bool has[2];           // the mate has a locus
    int32_t cs[2] = {0, 0};  // its score
    uint64_t lo[2] = {~0ull, ~0ull}, hi[2] = {0, 0};  // its text interval (without a locus: one that nothing touches)
#pragma unroll
    for (int m = 0; m < 2; m++) {
        const uint64_t c = R.cb[2 * m] + (m == 0 ? pick0 : pick1);
        has[m] = R.cb[2 * m + 2] != R.cb[2 * m];
        if (has[m]) {
            const bg_alignment_t& a = aln[c];
            cs[m] = a.score;
            if (!proper && cs[m] < qp.min_score) has[m] = false;
        }
        if (has[m]) {
            const bg_alignment_t& a = aln[c];
            lo[m] = w_lo[c] + a.ystart;
            hi[m] = w_lo[c] + a.yend;
        }
    }
    // 3. each mate's best candidate elsewhere
    uint64_t sub[2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
        const uint64_t c0 = R.cb[2 * m];
        const uint32_t nc = has[m] ? (uint32_t)(R.cb[2 * m + 2] - c0) : 0;
        uint64_t best = 0;
        for (uint32_t c = l16; c < nc; c += 16) {
            const bg_alignment_t& a = aln[c0 + c];
            const int32_t score = a.score;
            const uint64_t x_lo = w_lo[c0 + c] + a.ystart, x_hi = w_lo[c0 + c] + a.yend;
            if (score < qp.min_score || (x_lo <= hi[m] && lo[m] <= x_hi)) continue;
            best = max(best, score_key(score));
        }
        sub[m] = max16(best);
    }
    // 4. the best proper combination with mate m elsewhere (key: the sum biased to unsigned, + 1 so that 0 means none)
    uint64_t alt[2] = {0, 0};
#pragma unroll
    for (int o = 0; o < 2; o++) {
        // orientation A: a is m1's, b is m2's; orientation B: a is m2's, b is m1's
        const int ma = o == 0 ? 0 : 1, mb = 1 - ma;
        const uint64_t fa = R.cb[o == 0 ? 0 : 2], fb = R.cb[o == 0 ? 3 : 1];
        const uint32_t na = proper ? (uint32_t)(R.cb[o == 0 ? 1 : 3] - fa) : 0, nb = proper ? (uint32_t)(R.cb[o == 0 ? 4 : 2] - fb) : 0;
        const bool lanes_on_a = na > nb;
        const uint32_t n_out = lanes_on_a ? nb : na, n_in = lanes_on_a ? na : nb;
        for (uint32_t u = 0; u < n_out; u++) {
            for (uint32_t w = l16; w < n_in; w += 16) {
                const uint32_t i = lanes_on_a ? w : u, j = lanes_on_a ? u : w;
                const bg_alignment_t& A = aln[fa + i];
                const bg_alignment_t& B = aln[fb + j];
                const uint64_t a_start = w_lo[fa + i] + A.ystart, b_start = w_lo[fb + j] + B.ystart;
                if (a_start > b_start) continue;
                const uint64_t a_end = w_lo[fa + i] + A.yend, b_end = w_lo[fb + j] + B.yend;
                const uint64_t span = max(a_end, b_end) - a_start;
                if (span < pp.min_span || span > pp.max_span) continue;
                const uint64_t key = (uint64_t)((int64_t)A.score + B.score + (1ll << 32)) + 1;
                if (A.score >= qp.min_score && !(a_start <= hi[ma] && lo[ma] <= a_end)) alt[ma] = max(alt[ma], key);
                if (B.score >= qp.min_score && !(b_start <= hi[mb] && lo[mb] <= b_end)) alt[mb] = max(alt[mb], key);
            }
        }
    }
    alt[0] = max16(alt[0]);
    alt[1] = max16(alt[1]);
    if (l16) return;
#pragma unroll
    for (int m = 0; m < 2; m++) {
        bg_multi_hit_t mh;
        memset(&mh, 0, sizeof(mh));
        mh.sub_score = BG_MIN_SCORE;
        if (has[m]) {
            const bool other = sub[m] != 0;
            const int64_t s1 = cs[m];
            if (other) mh.sub_score = score_of(sub[m]);
            mh.n_loci = other ? 2 : 1;
            mh.n_reported = 1;
            uint64_t num = 0;  // the score this mate's locus is ahead by, 0 ..= s1
            if (s1 > 0) {
                if (!other) {
                    num = (uint64_t)s1;
                } else if (proper) {
                    // S2: the pair's best total with this mate elsewhere, in a proper combination or unpaired
                    int64_t s2 = (int64_t)mh.sub_score + cs[1 - m] - pp.pen_unpaired;
                    if (alt[m]) s2 = max(s2, (int64_t)(alt[m] - 1) - (1ll << 32));
                    num = (uint64_t)min(max(pair_sum - s2, (int64_t)0), s1);  // (S1 >= S2: include/biogpu.h)
                } else {
                    const int64_t runner = max(mh.sub_score, 0);
                    num = runner < s1 ? (uint64_t)(s1 - runner) : 0;
                }
            }
            if (s1 > 0) mh.mapq = (uint8_t)min((uint64_t)qp.mapq_cap, (uint64_t)qp.mapq_cap * num / (uint64_t)s1);
        }
        multi[r0 + 2 * p + m] = mh;
    }
}

}  // namespace

int bg_seed_pairq_launch(const bg_pair_params_t* pp, const bg_pairq_params_t* qp, uint64_t n_pairs, uint64_t r0, const uint64_t* d_coff,
                         const uint32_t* d_n_hits, const bg_alignment_t* d_aln, const uint8_t* d_c_ops, const uint64_t* d_w_lo,
                         bg_seed_hit_t* d_hits, uint8_t* d_ops, uint64_t ops_stride, uint8_t* d_strand, bg_pair_hit_t* d_pairs,
                         bg_multi_hit_t* d_multi, uint32_t max_cand, hipStream_t st) {
    if (max_cand > kMaxCand) return BG_ERR_UNSUPPORTED;
    if (n_pairs == 0) return BG_OK;
    const PairPrm prm{pp->min_span, pp->max_span, pp->pen_unpaired};
    const PairqPrm qprm{qp->min_score, qp->mapq_cap};
    se_pairq_kernel<<<dim3((unsigned)((n_pairs * 16 + 255) / 256)), dim3(256), 0, st>>>(n_pairs, r0, prm, qprm, d_coff, d_n_hits, d_aln,
                                                                                         d_c_ops, d_w_lo, d_hits, d_ops, ops_stride, d_strand,
                                                                                         d_pairs, d_multi);
    BG_HIP(hipGetLastError());
    return BG_OK;
}
