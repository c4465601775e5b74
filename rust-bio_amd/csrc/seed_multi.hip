// Runner-up loci and a mapping quality in seed-and-extend (bg_seed_extend_multi_batch[_dev]): the stage that replaces S7 of
// seed_extend.hip in multi mode.  The passes of seed_extend.hip run every stage up to the alignment of every candidate
// unchanged; where se_best_kernel keeps one candidate per read, this stage walks them in rank order and keeps up to
// max(K, 2) loci whose text intervals do not touch (definition in include/biogpu.h), reports the first K and derives
// MAPQ from the first two.
#include "fm_kernels.h"

namespace {

constexpr uint32_t kMaxCand = 1024;   // candidates of one virtual read are at most this: 2 x 1024 per read with both strands
constexpr uint32_t kMaskWords = 4;    // 16 lanes x 4 x 32 bits = 2048 candidates

struct MultiPrm {
    uint32_t K, rounds;  // rounds = max(K, 2): the runner-up is found even when K = 1
    int32_t min_score;
    uint32_t mapq_cap;
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

// S7 of the multi call: 16 lanes per read.  Read r's candidates are those of its G virtual reads, coff[G r] .. coff[G r + G),
// numbered as se_best_kernel<G> numbers them; lane l owns candidates l, l + 16, ... and keeps one bit per owned candidate
// ("out": below min_score, or touching a locus already kept) in four dwords.  Round k is one pass over the lane's candidates
// that are still in: those that touch the locus kept in round k - 1 go out (the kept one among them), the others compete with
// se_best_kernel's key (score biased to unsigned, ~candidate number) in a 16-lane max.  Round k's winner is locus k: slot
// K (r0 + r) + k of `hits` / `strand` / `ops` while k < K.  The round loop is the same for every lane of the wavefront (the
// four reads of a wavefront have different candidate counts): a group that has run out of candidates stays in it with
// nothing to scan, so that the shuffles of max16 run with every lane active.
template <int G>
__global__ __launch_bounds__(256) void se_multi_kernel(uint64_t n_reads, uint64_t r0, MultiPrm mp, const uint64_t* __restrict__ coff,
                                                       const uint32_t* __restrict__ n_hits, const bg_alignment_t* __restrict__ aln,
                                                       const uint8_t* __restrict__ c_ops, const uint64_t* __restrict__ w_lo,
                                                       bg_seed_hit_t* __restrict__ hits, uint8_t* __restrict__ ops, uint64_t ops_stride,
                                                       uint8_t* __restrict__ strand, uint8_t strand1, bg_multi_hit_t* __restrict__ multi) {
    const uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t l16 = threadIdx.x & 15;
    const bool live = r < n_reads;  // uniform per group of 16
    uint64_t c0 = 0;
    uint32_t nc = 0, n_fwd = 0;
    if (live) {
        c0 = coff[G * r];
        nc = (uint32_t)(coff[G * r + G] - c0);
        n_fwd = G == 2 ? (uint32_t)(coff[2 * r + 1] - c0) : 0;
    }
    uint32_t nsh = 0;
    if (live) nsh = G == 2 ? n_hits[2 * r] + n_hits[2 * r + 1] : n_hits[r];

    uint32_t out0 = 0, out1 = 0, out2 = 0, out3 = 0;  // (named, not an array: a runtime index would put them in scratch)
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
                    const bg_alignment_t& a = aln[c0 + c];
                    const int32_t score = a.score;
                    const uint64_t lo = w_lo[c0 + c] + a.ystart, hi = w_lo[c0 + c] + a.yend;
                    if (score < mp.min_score || (lo <= k_hi && k_lo <= hi)) {
                        m |= 1u << b;
                        continue;
                    }
                    best = max(best, ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint32_t)~c);
                }
                out0 = out1, out1 = out2, out2 = out3, out3 = m;
            }
        }
        best = max16(best);  // every lane of the wavefront is here
        if (best == 0) done = true;
        if (__all(done)) break;
        if (done) continue;
        const uint32_t c = ~(uint32_t)best;
        const bg_alignment_t& a = aln[c0 + c];
        const uint64_t wl = w_lo[c0 + c];
        const int32_t score = a.score;
        k_lo = wl + a.ystart;
        k_hi = wl + a.yend;
        if (k == 0) s1 = score;
        if (k == 1) s2 = score;
        n_loci++;
        if (k < mp.K) {
            const uint64_t slot = (r0 + r) * mp.K + k;
            const uint32_t n_ops = a.n_ops;
            const uint64_t to = (slot + 1) * ops_stride - n_ops;
            if (ops && c_ops) {
                const uint64_t from = a.ops_off;
#pragma unroll 4
                for (uint32_t i = l16; i < n_ops; i += 16) ops[to + i] = c_ops[from + i];
            }
            if (l16 == 0) {
                bg_seed_hit_t h;
                h.aln = a;
                h.aln.ops_off = to;
                h.window_start = wl;
                h.ref_start = k_lo;
                h.ref_end = k_hi;
                h.n_candidates = nc;
                h.n_seed_hits = nsh;
                hits[slot] = h;
                if (strand) strand[slot] = G == 2 ? (c >= n_fwd ? BG_HIT_REVERSE : BG_HIT_FORWARD) : strand1;
            }
        }
    }
    if (!live || l16) return;
    const uint32_t n_rep = min(n_loci, mp.K);
    bg_seed_hit_t h;
    memset(&h, 0, sizeof(h));
    h.aln.score = BG_MIN_SCORE;
    h.window_start = h.ref_start = h.ref_end = ~0ull;
    h.n_candidates = nc;
    h.n_seed_hits = nsh;
    for (uint32_t k = n_rep; k < mp.K; k++) {  // unused slots: written like an unmapped read
        const uint64_t slot = (r0 + r) * mp.K + k;
        h.aln.ops_off = (slot + 1) * ops_stride;
        hits[slot] = h;
        if (strand) strand[slot] = BG_HIT_NONE;
    }
    bg_multi_hit_t mh;
    memset(&mh, 0, sizeof(mh));
    mh.sub_score = s2;
    mh.n_loci = n_loci;
    mh.n_reported = (uint8_t)n_rep;
    const int64_t runner = n_loci > 1 ? max(s2, 0) : 0;
    if (n_loci && s1 > 0 && runner < s1)
        mh.mapq = (uint8_t)min((uint64_t)mp.mapq_cap, (uint64_t)mp.mapq_cap * (uint64_t)(s1 - runner) / (uint64_t)s1);
    multi[r0 + r] = mh;
}

}  // namespace

int bg_seed_multi_launch(const bg_multi_params_t* mp, uint32_t G, uint8_t strand1, uint64_t n_reads, uint64_t r0, const uint64_t* d_coff,
                         const uint32_t* d_n_hits, const bg_alignment_t* d_aln, const uint8_t* d_c_ops, const uint64_t* d_w_lo,
                         bg_seed_hit_t* d_hits, uint8_t* d_ops, uint64_t ops_stride, uint8_t* d_strand, bg_multi_hit_t* d_multi,
                         uint32_t max_cand, hipStream_t st) {
    if (max_cand > kMaxCand || G * kMaxCand > 16 * 32 * kMaskWords) return BG_ERR_UNSUPPORTED;
    if (n_reads == 0) return BG_OK;
    const MultiPrm prm{mp->max_hits, mp->max_hits > 2 ? mp->max_hits : 2u, mp->min_score, mp->mapq_cap};
    const dim3 grid((unsigned)((n_reads * 16 + 255) / 256)), block(256);
    if (G == 2)
        se_multi_kernel<2><<<grid, block, 0, st>>>(n_reads, r0, prm, d_coff, d_n_hits, d_aln, d_c_ops, d_w_lo, d_hits, d_ops, ops_stride,
                                                   d_strand, strand1, d_multi);
    else
        se_multi_kernel<1><<<grid, block, 0, st>>>(n_reads, r0, prm, d_coff, d_n_hits, d_aln, d_c_ops, d_w_lo, d_hits, d_ops, ops_stride,
                                                   d_strand, strand1, d_multi);
    BG_HIP(hipGetLastError());
    return BG_OK;
}
