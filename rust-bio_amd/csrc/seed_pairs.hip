// Read pairs in seed-and-extend (bg_seed_extend_pairs_batch[_dev]): the pair stage that replaces S7 of seed_extend.hip
// in pair mode.  The passes of seed_extend.hip run every stage up to the alignment of every candidate unchanged on the virtual
// reads m1, rc(m1), m2, rc(m2) of each pair of interleaved mates; this stage reduces over all candidates of those four at
// once: the best proper FR combination (definition in include/biogpu.h) or each mate's own best.
#include "seed_pair_rule.h"

namespace {

using namespace bgpair;

// S7 of the paired call: 16 lanes per pair.  Pair p of the pass is caller reads 2p, 2p + 1 (r0 + 2p of the call) and virtual
// reads 4p .. 4p + 3 = m1, rc(m1), m2, rc(m2): candidates coff[4p + v] .. coff[4p + v + 1) of each.  The rule and the writes
// are seed_pair_rule.h's (the rescue call's plan stage runs the same two).
__global__ __launch_bounds__(256) void se_pair_kernel(uint64_t n_pairs, uint64_t r0, PairPrm pp, const uint64_t* __restrict__ coff,
                                                      const uint32_t* __restrict__ n_hits, const bg_alignment_t* __restrict__ aln,
                                                      const uint8_t* __restrict__ c_ops, const uint64_t* __restrict__ w_lo,
                                                      bg_seed_hit_t* __restrict__ hits, uint8_t* __restrict__ ops, uint64_t ops_stride,
                                                      uint8_t* __restrict__ strand, bg_pair_hit_t* __restrict__ pairs) {
    const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t l16 = threadIdx.x & 15;
    if (p >= n_pairs) return;  // uniform per group of 16
    const PairRule R = pair_rule(p, l16, pp, coff, aln, w_lo);
    pair_write(p, l16, r0, pp, R, n_hits, aln, c_ops, w_lo, hits, ops, ops_stride, strand, pairs);
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
