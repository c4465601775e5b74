// Runner-up loci and a mapping quality in seed-and-extend (bg_seed_extend_multi_batch[_dev]): the stage that replaces S7 of
// seed_extend.hip in multi mode.  The passes of seed_extend.hip run every stage up to the alignment of every candidate
// unchanged; where se_best_kernel keeps one candidate per read, this stage walks them in rank order and keeps up to
// max(K, 2) loci whose text intervals do not touch (definition in include/biogpu.h), reports the first K and derives
// MAPQ from the first two.
#include "seed_rule.h"

namespace {

using namespace bgseed;

struct MultiPrm {
    uint32_t K, rounds;  // rounds = max(K, 2): the runner-up is found even when K = 1
    int32_t min_score;
    uint32_t mapq_cap;
};

// S7 of the multi call: 16 lanes per read.  Read r's candidates are those of its G virtual reads, coff[G r] .. coff[G r + G),
// numbered as se_best_kernel<G> numbers them; lane l owns candidates l, l + 16, ... and keeps one bit per owned candidate
// ("out": below min_score, or touching a locus already kept) in four dwords.  Round k is one pass over the lane's candidates
// that are still in: those that touch the locus kept in round k - 1 go out (the kept one among them), the others compete with
// se_best_kernel's key (score biased to unsigned, ~candidate number) in a 16-lane max.  Round k's winner is locus k: slot
// K (r0 + r) + k of `hits` / `strand` / `ops` while k < K.  The round loop is the same for every lane of the wavefront (the
// four reads of a wavefront have different candidate counts): a group that has run out of candidates stays in it with
// nothing to scan, so that the shuffles of max16 run with every lane active.
template <int G>
__global__ __launch_bounds__(256) void se_multi_kernel(SeedPass P, SeedOut O, MultiPrm mp, uint8_t strand1) {
    const uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t l16 = threadIdx.x & 15;
    const bool live = r < P.n;  // uniform per group of 16
    uint64_t c0 = 0;
    uint32_t nc = 0, n_fwd = 0;
    if (live) {
        c0 = P.coff[G * r];
        nc = (uint32_t)(P.coff[G * r + G] - c0);
        n_fwd = G == 2 ? (uint32_t)(P.coff[2 * r + 1] - c0) : 0;
    }
    uint32_t nsh = 0;
    if (live) nsh = G == 2 ? P.n_hits[2 * r] + P.n_hits[2 * r + 1] : P.n_hits[r];

    uint32_t out0 = 0, out1 = 0, out2 = 0, out3 = 0;  // (named, not an array: a runtime index would put them in scratch)
    static_assert(kMaskWords == 4, "out0 .. out3");
    uint64_t k_lo = ~0ull, k_hi = 0;  // the interval kept last (before the first round: one that nothing touches)
    uint32_t n_loci = 0;
    int32_t s1 = 0, s2 = BG_MIN_SCORE;
    bool done = nc == 0;
    for (uint32_t k = 0; k < mp.rounds; k++) {
        uint64_t best = 0;
        if (!done) {
#pragma unroll 1
            for (uint32_t w = 0; w < kMaskWords; w++) {  // the word in turn is out0: the four rotate once round per pass
                uint32_t m = out0;
#pragma unroll 1
                for (uint32_t b = 0; b < 32; b++) {
                    const uint32_t c = ((w * 32 + b) << 4) + l16;
                    if (c >= nc) break;
                    if (m >> b & 1) continue;
                    const bg_alignment_t& a = P.aln[c0 + c];
                    const int32_t score = a.score;
                    const uint64_t lo = P.w_lo[c0 + c] + a.ystart, hi = P.w_lo[c0 + c] + a.yend;
                    if (score < mp.min_score || (lo <= k_hi && k_lo <= hi)) {
                        m |= 1u << b;
                        continue;
                    }
                    best = max(best, own_key(score, c));
                }
                out0 = out1, out1 = out2, out2 = out3, out3 = m;
            }
        }
        best = max16(best);  // every lane of the wavefront is here
        if (best == 0) done = true;
        if (__all(done)) break;
        if (done) continue;
        const uint32_t c = key_cand(best);
        const bg_alignment_t& a = P.aln[c0 + c];
        k_lo = P.w_lo[c0 + c] + a.ystart;
        k_hi = P.w_lo[c0 + c] + a.yend;
        if (k == 0) s1 = a.score;
        if (k == 1) s2 = a.score;
        n_loci++;
        if (k < mp.K)
            write_cand(P, O, (P.r0 + r) * mp.K + k, l16, c0 + c, G == 2 ? (c >= n_fwd ? BG_HIT_REVERSE : BG_HIT_FORWARD) : strand1, nc, nsh);
    }
    if (!live) return;
    const uint32_t n_rep = min(n_loci, mp.K);
    for (uint32_t k = n_rep; k < mp.K; k++)  // unused slots: written like an unmapped read
        write_cand(P, O, (P.r0 + r) * mp.K + k, l16, 0, BG_HIT_NONE, nc, nsh);
    if (l16) return;
    bg_multi_hit_t mh;
    memset(&mh, 0, sizeof(mh));
    mh.sub_score = s2;
    mh.n_loci = n_loci;
    mh.n_reported = (uint8_t)n_rep;
    const int64_t runner = n_loci > 1 ? max(s2, 0) : 0;
    mh.mapq = mapq_of(mp.mapq_cap, runner < s1 ? (uint64_t)(s1 - runner) : 0, s1);
    O.multi[P.r0 + r] = mh;
}

}  // namespace

int bg_seed_multi_launch(const SeedPass& P, const SeedOut& O, const bg_multi_params_t* mp, uint32_t G, uint8_t strand1, hipStream_t st) {
    if (P.n == 0) return BG_OK;
    const MultiPrm prm{mp->max_hits, mp->max_hits > 2 ? mp->max_hits : 2u, mp->min_score, mp->mapq_cap};
    const dim3 grid((unsigned)((P.n * 16 + 255) / 256)), block(256);
    if (G == 2)
        se_multi_kernel<2><<<grid, block, 0, st>>>(P, O, prm, strand1);
    else
        se_multi_kernel<1><<<grid, block, 0, st>>>(P, O, prm, strand1);
    BG_HIP(hipGetLastError());
    return BG_OK;
}
