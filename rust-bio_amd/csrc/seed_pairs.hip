// Read pairs in seed-and-extend (bg_seed_extend_pairs_batch[_dev]): the pair stage that replaces S7 of seed_extend.hip
// in pair mode.  The passes of seed_extend.hip run every stage up to the alignment of every candidate unchanged on the virtual
// reads m1, rc(m1), m2, rc(m2) of each pair of interleaved mates; this stage reduces over all candidates of those four at
// once: the best proper FR combination (definition in include/biogpu.h) or each mate's own best.
#include "fm_kernels.h"

namespace {

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

// S7 of the paired call: 16 lanes per pair.  Pair p of the pass is caller reads 2p, 2p + 1 (r0 + 2p of the call) and virtual
// reads 4p .. 4p + 3 = m1, rc(m1), m2, rc(m2): candidates coff[4p + v] .. coff[4p + v + 1) of each.  Orientation A pairs m1's
// forward candidates (v = 0) with m2's reverse ones (v = 3), orientation B m2's forward ones (v = 2) with m1's reverse ones
// (v = 1).  The lanes walk each orientation's product, strided over the longer list, with one key per combination: the
// score sum biased to unsigned (33 bits), 1 for orientation A, ~i, ~j (10 bits each: both below kMaxCand), so the max is
// the rule's best.  Each mate's own best is se_best_kernel<2>'s key; a mate that is not part of a proper pair reports exactly
// what se_best_kernel<2> writes for it.
__global__ __launch_bounds__(256) void se_pair_kernel(uint64_t n_pairs, uint64_t r0, PairPrm pp, const uint64_t* __restrict__ coff,
                                                      const uint32_t* __restrict__ n_hits, const bg_alignment_t* __restrict__ aln,
                                                      const uint8_t* __restrict__ c_ops, const uint64_t* __restrict__ w_lo,
                                                      bg_seed_hit_t* __restrict__ hits, uint8_t* __restrict__ ops, uint64_t ops_stride,
                                                      uint8_t* __restrict__ strand, bg_pair_hit_t* __restrict__ pairs) {
    const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t l16 = threadIdx.x & 15;
    if (p >= n_pairs) return;  // uniform per group of 16
    uint64_t cb[5];
#pragma unroll
    for (int v = 0; v < 5; v++) cb[v] = coff[4 * p + v];
    // each mate's own best over both strands: highest score, forward strand on a tie, smallest start
    uint64_t own[2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
        const uint64_t c0 = cb[2 * m];
        const uint32_t nc = (uint32_t)(cb[2 * m + 2] - c0);
        uint64_t best = 0;
        for (uint32_t c = l16; c < nc; c += 16) {
            const uint32_t sc = (uint32_t)aln[c0 + c].score ^ 0x80000000u;
            best = max(best, ((uint64_t)sc << 32) | (uint32_t)~c);
        }
        own[m] = max16(best);
    }
    // proper combinations of both orientations
    uint64_t best = 0;
    uint32_t n_proper = 0;
#pragma unroll
    for (int o = 0; o < 2; o++) {
        const uint64_t fa = cb[o == 0 ? 0 : 2], fb = cb[o == 0 ? 3 : 1];
        const uint32_t na = (uint32_t)(cb[o == 0 ? 1 : 3] - fa), nb = (uint32_t)(cb[o == 0 ? 4 : 2] - fb);
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
    best = max16(best);
#pragma unroll
    for (int o = 8; o; o >>= 1) n_proper += (uint32_t)__shfl_xor((int)n_proper, o, 16);
    // rule 4: the best proper pair, if it gives up at most pen_unpaired against the mates' own bests
    bool proper = false;
    uint64_t pick[2] = {~(uint32_t)own[0], ~(uint32_t)own[1]};  // candidate per mate, relative to cb[2m]
    uint64_t span = 0;
    if (n_proper) {
        const int64_t pair_sum = (int64_t)(best >> 21) - (1ll << 32);
        const int64_t own_sum = (int64_t)(int32_t)((uint32_t)(own[0] >> 32) ^ 0x80000000u) + (int32_t)((uint32_t)(own[1] >> 32) ^ 0x80000000u);
        if (pair_sum + pp.pen_unpaired >= own_sum) {
            proper = true;
            const bool orient_a = (best >> 20) & 1;
            const uint32_t i = kMaxCand - 1 - (uint32_t)((best >> 10) & (kMaxCand - 1));
            const uint32_t j = kMaxCand - 1 - (uint32_t)(best & (kMaxCand - 1));
            const uint64_t ca = (orient_a ? cb[0] : cb[2]) + i, cr = (orient_a ? cb[3] : cb[1]) + j;  // forward, reverse
            const uint64_t a_start = w_lo[ca] + aln[ca].ystart;
            span = max(w_lo[ca] + aln[ca].yend, w_lo[cr] + aln[cr].yend) - a_start;
            pick[0] = (orient_a ? ca : cr) - cb[0];
            pick[1] = (orient_a ? cr : ca) - cb[2];
        }
    }
#pragma unroll
    for (int m = 0; m < 2; m++) {
        const uint64_t r = 2 * p + m;
        const uint64_t c0 = cb[2 * m];
        const uint32_t nc = (uint32_t)(cb[2 * m + 2] - c0);
        bg_seed_hit_t h;
        memset(&h, 0, sizeof(h));
        h.aln.score = BG_MIN_SCORE;
        h.window_start = h.ref_start = h.ref_end = ~0ull;
        h.n_candidates = nc;
        h.n_seed_hits = n_hits[4 * p + 2 * m] + n_hits[4 * p + 2 * m + 1];
        h.aln.ops_off = (r0 + r + 1) * ops_stride;
        uint8_t won = BG_HIT_NONE;
        if (nc) {
            const uint64_t c = pick[m];
            won = c >= cb[2 * m + 1] - c0 ? BG_HIT_REVERSE : BG_HIT_FORWARD;
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
    if (l16 == 0) {
        bg_pair_hit_t ph;
        memset(&ph, 0, sizeof(ph));
        ph.span = span;
        ph.n_proper = n_proper;
        ph.proper = proper ? 1 : 0;
        pairs[r0 / 2 + p] = ph;
    }
}

}  // namespace

int bg_seed_pairs_launch(const bg_pair_params_t* pp, uint64_t n_pairs, uint64_t r0, const uint64_t* d_coff, const uint32_t* d_n_hits,
                         const bg_alignment_t* d_aln, const uint8_t* d_c_ops, const uint64_t* d_w_lo, bg_seed_hit_t* d_hits,
                         uint8_t* d_ops, uint64_t ops_stride, uint8_t* d_strand, bg_pair_hit_t* d_pairs, uint32_t max_cand, hipStream_t st) {
    if (max_cand > kMaxCand) return BG_ERR_UNSUPPORTED;
    if (n_pairs == 0) return BG_OK;
    const PairPrm prm{pp->min_span, pp->max_span, pp->pen_unpaired};
    se_pair_kernel<<<dim3((unsigned)((n_pairs * 16 + 255) / 256)), dim3(256), 0, st>>>(n_pairs, r0, prm, d_coff, d_n_hits, d_aln, d_c_ops,
                                                                                        d_w_lo, d_hits, d_ops, ops_stride, d_strand, d_pairs);
    BG_HIP(hipGetLastError());
    return BG_OK;
}
