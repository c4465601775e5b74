// Read pairs in seed-and-extend (bg_seed_extend_pairs_batch[_dev]): the pair stage that replaces S7 of seed_extend.hip
// in pair mode.  The passes of seed_extend.hip run every stage up to the alignment of every candidate unchanged on the virtual
// reads m1, rc(m1), m2, rc(m2) of each pair of interleaved mates; this stage reduces over all candidates of those four at
// once: the best proper FR combination (definition in include/biogpu.h) or each mate's own best.
#include "seed_pair_rule.h"

namespace {

using namespace bgpair;

// S7 of the paired call: 16 lanes per pair.  Pair p of the pass is caller reads 2p, 2p + 1 (r0 + 2p of the call) and virtual
// reads 4p .. 4p + 3 = m1, rc(m1), m2, rc(m2): candidates coff[4p + v] .. coff[4p + v + 1) of each.  The rule and the writes
// are seed_pair_rule.h's (the rescue call's plan stage runs the same).
__global__ __launch_bounds__(256) void se_pair_kernel(SeedPass P, SeedOut O, PairPrm pp) {
    const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t l16 = threadIdx.x & 15;
    if (p >= P.n) return;  // uniform per group of 16
    const PairRule R = pair_rule(P, p, l16, pp);
    pair_write(P, O, p, l16, R, pair_choice(P, R, pp));
}

}  // namespace

int bg_seed_pairs_launch(const SeedPass& P, const SeedOut& O, const bg_pair_params_t* pp, hipStream_t st) {
    if (P.n == 0) return BG_OK;
    se_pair_kernel<<<dim3((unsigned)((P.n * 16 + 255) / 256)), dim3(256), 0, st>>>(P, O, pair_prm(pp));
    BG_HIP(hipGetLastError());
    return BG_OK;
}
