// A mapping quality for each mate of a read pair (bg_seed_extend_pairs_mapq_batch[_dev]): the stage that replaces S7 of
// seed_extend.hip in this mode.  It is the pair stage (seed_pairs.hip: the same rule and the same writes, from seed_pair_rule.h)
// plus one bg_multi_hit_t per mate.  A mate of a proper pair is judged against the pair: how much score the best placement
// of the PAIR loses when this mate goes to another locus (definition in include/biogpu.h, "Mapping quality of read pairs").
// A mate of a pair that is not proper is judged as the multi call judges a single read at K = 1.
#include "seed_pair_rule.h"

namespace {

using namespace bgpair;

// S7 of the pairs-mapq call: 16 lanes per pair, pair p as in se_pair_kernel.
//   1. pair_rule, pair_choice, pair_write: hits, strand, operations and pairs, byte for byte the paired call's.
//   2. the locus each mate is judged against: the chosen combination's member (proper), or the mate's own best if it scores
//      >= min_score (not proper: locus 0 of the multi rule; `pick` is the multi rule's candidate number, forward strand first).
//   3. per mate, best_elsewhere over its candidates of both strands: the best score among those >= min_score that do not touch
//      that locus.  This is the multi rule's runner-up, and for a proper pair the mate's best alternative (sub_score, kind (b)).
//   4. proper pairs only: a second walk over the proper combinations (for_proper, as pair_rule walks them) that keeps per mate
//      the highest score sum over proper combinations whose member of that mate is an alternative (kind (a)).  Groups whose
//      pair is not proper walk nothing (their bounds are 0) and stay in the reductions.
// No LDS, no atomics; every reduction is a max16 on a 64-bit key.
__global__ __launch_bounds__(256) void se_pairq_kernel(SeedPass P, SeedOut O, PairPrm pp, PairqPrm qp) {
    const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t l16 = threadIdx.x & 15;
    if (p >= P.n) return;  // uniform per group of 16
    const PairRule R = pair_rule(P, p, l16, pp);
    const PairChoice ch = pair_choice(P, R, pp);
    pair_write(P, O, p, l16, R, ch);

    // 2. each mate's locus
    bool has[2];           // the mate has a locus
    int32_t cs[2] = {0, 0};  // its score
    uint64_t lo[2] = {~0ull, ~0ull}, hi[2] = {0, 0};  // its text interval (without a locus: one that nothing touches)
#pragma unroll
    for (int m = 0; m < 2; m++) {
        const uint64_t c = R.cb[2 * m] + ch.pick[m];
        has[m] = R.cb[2 * m + 2] != R.cb[2 * m];
        if (has[m]) {
            const bg_alignment_t& a = P.aln[c];
            cs[m] = a.score;
            if (!ch.proper && cs[m] < qp.min_score) has[m] = false;
        }
        if (has[m]) {
            const bg_alignment_t& a = P.aln[c];
            lo[m] = P.w_lo[c] + a.ystart;
            hi[m] = P.w_lo[c] + a.yend;
        }
    }
    // 3. each mate's best candidate elsewhere
    uint64_t sub[2];
#pragma unroll
    for (int m = 0; m < 2; m++)
        sub[m] = best_elsewhere(P, l16, R.cb[2 * m], has[m] ? (uint32_t)(R.cb[2 * m + 2] - R.cb[2 * m]) : 0, lo[m], hi[m], qp.min_score);
    // 4. the best proper combination with mate m elsewhere (key: the sum biased to unsigned, + 1 so that 0 means none)
    uint64_t alt[2] = {0, 0};
    for_proper(P, R.cb, ch.proper, l16, pp, [&](const ProperCombo& k) {
        // orientation A: a is m1's, b is m2's; orientation B: a is m2's, b is m1's
        const int ma = k.o == 0 ? 0 : 1, mb = 1 - ma;
        const uint64_t key = (uint64_t)((int64_t)k.a_score + k.b_score + (1ll << 32)) + 1;
        if (k.a_score >= qp.min_score && !(k.a_start <= hi[ma] && lo[ma] <= k.a_end)) alt[ma] = max(alt[ma], key);
        if (k.b_score >= qp.min_score && !(k.b_start <= hi[mb] && lo[mb] <= k.b_end)) alt[mb] = max(alt[mb], key);
    });
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
                } else if (ch.proper) {
                    // S2: the pair's best total with this mate elsewhere, in a proper combination or unpaired
                    int64_t s2 = (int64_t)mh.sub_score + cs[1 - m] - pp.pen_unpaired;
                    if (alt[m]) s2 = max(s2, (int64_t)(alt[m] - 1) - (1ll << 32));
                    num = (uint64_t)min(max(ch.pair_sum - s2, (int64_t)0), s1);  // (S1 >= S2: include/biogpu.h)
                } else {
                    const int64_t runner = max(mh.sub_score, 0);
                    num = runner < s1 ? (uint64_t)(s1 - runner) : 0;
                }
            }
            mh.mapq = mapq_of(qp.mapq_cap, num, s1);
        }
        O.multi[P.r0 + 2 * p + m] = mh;
    }
}

}  // namespace

int bg_seed_pairq_launch(const SeedPass& P, const SeedOut& O, const bg_pair_params_t* pp, const bg_pairq_params_t* qp, hipStream_t st) {
    if (P.n == 0) return BG_OK;
    se_pairq_kernel<<<dim3((unsigned)((P.n * 16 + 255) / 256)), dim3(256), 0, st>>>(P, O, pair_prm(pp), PairqPrm{qp->min_score, qp->mapq_cap});
    BG_HIP(hipGetLastError());
    return BG_OK;
}
