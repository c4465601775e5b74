// Mate rescue in seed-and-extend (bg_seed_extend_pairs_rescue_batch[_dev]): the stages that replace S7 of seed_extend.hip in
// pair mode when rescue is asked for.  A pair whose seeded candidates hold no proper combination is given a second chance:
// each mate's best candidates ("anchors") say where the other mate must lie, and that mate is aligned semiglobally against
// the anchor's insert window (definition in include/biogpu.h, "Mate rescue").
//   R1 plan     per pair: the pair rule and the paired call's own writes (seed_pair_rule.h, shared with se_pair_kernel); for a
//               pair without a proper combination the anchors of each mate -> rescue plan entries + per-pair counts
//      (scan of the per-pair rescue / x-byte / y-byte counts; the three totals are the ONE extra host round trip of a pass)
//   R2 gather   (other mate on the sought strand, anchor window) pairs, offsets         -> x, x_off, y, y_off
//   R3 align    Aligner::semiglobal on every rescue pair (bg_align_batch_dev_hint, by seed_extend.hip)
//   R4 pick     per pair: acceptance, choice, "paired or not"; a rescued pair's two hits, strands, operations, pair record
//               and rescued byte overwrite what R1 wrote for it
// A pass without a single rescue alignment stops after R1's read-back.
#include <algorithm>

#include "seed_rescue_rule.h"

namespace {

using namespace bgpair;

// R1: 16 lanes per pair.  Every pair is first answered as the paired call answers it (rescued = 0).  The anchors of a mate are
// its first A candidates in rank order: A rounds of the own-best key's max over the keys below the last one found.
__global__ __launch_bounds__(256) void se_rescue_plan_kernel(SeedPass P, SeedOut O, PairPrm pp, RescuePrm rp, SeedRescuePlan out) {
    const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t l16 = threadIdx.x & 15;
    if (p >= P.n) return;  // uniform per group of 16
    const PairRule R = pair_rule(P, p, l16, pp);
    pair_write(P, O, p, l16, R, pair_choice(P, R, pp));
    RescuePlan* plan = (RescuePlan*)out.plan;
    uint32_t nr = 0, xb = 0, yb = 0;
    if (R.n_proper == 0) {
#pragma unroll
        for (int m = 0; m < 2; m++) {
            const uint64_t c0 = R.cb[2 * m];
            const uint32_t nc = (uint32_t)(R.cb[2 * m + 2] - c0), n_fwd = (uint32_t)(R.cb[2 * m + 1] - c0);
            if (!nc) continue;
            const int other = 1 - m;
            const uint32_t Lo = (uint32_t)(P.voff[4 * p + 2 * other + 1] - P.voff[4 * p + 2 * other]);  // the sought mate's length
            uint64_t prev = ~0ull;
            for (uint32_t k = 0; k < rp.max_anchors; k++) {
                uint64_t best = 0;
                for (uint32_t c = l16; c < nc; c += 16) {
                    const uint64_t key = own_key(P.aln[c0 + c].score, c);
                    if (key < prev) best = max(best, key);
                }
                best = max16(best);
                if (!best) break;  // fewer than A candidates (a candidate's key is never 0)
                prev = best;
                const uint32_t c = key_cand(best);
                const bool fwd = c < n_fwd;
                const bg_alignment_t& a = P.aln[c0 + c];
                const uint64_t rs = P.w_lo[c0 + c] + a.ystart, re = P.w_lo[c0 + c] + a.yend;
                if (re - rs > pp.max_span) continue;
                const uint64_t lo = fwd ? rs : (re > pp.max_span ? re - pp.max_span : 0u);
                const uint64_t hi = fwd ? min(rp.n_text, rs + pp.max_span) : re;
                if (hi <= lo || Lo == 0) continue;
                if (l16 == 0) {
                    RescuePlan e;
                    e.lo = lo;
                    e.len = (uint32_t)(hi - lo);
                    // the forward anchor's mate is sought on the reverse strand: its revcomp, virtual read 2 other + 1
                    e.info = (uint32_t)(c0 + c - R.cb[0]) | (uint32_t)(2 * other + (fwd ? 1 : 0)) << 16 | k << 18 | (fwd ? 1u : 0u) << 20 |
                             (uint32_t)m << 21;
                    plan[kSlots * p + nr] = e;
                }
                nr++;
                xb += Lo;
                yb += (uint32_t)(hi - lo);
            }
        }
    }
    if (l16 == 0) {
        O.rescued[P.r0 / 2 + p] = 0;
        out.n_res[p] = nr;
        out.x_bytes[p] = xb;
        out.y_bytes[p] = yb;
        // own(m): 0 for a mate without candidates
        out.own_sum[p] = (int64_t)(R.cb[2] > R.cb[0] ? key_score(R.own[0]) : 0) + (R.cb[4] > R.cb[2] ? key_score(R.own[1]) : 0);
    }
}

// R2: one wavefront per pair, four per block: the (x, window) pairs of its planned rescues + their offsets.  x is read from the
// pass's virtual reads, which hold both strands of every mate.
__global__ __launch_bounds__(256) void se_rescue_gather_kernel(SeedPass P, const uint8_t* __restrict__ vreads, const uint8_t* __restrict__ text,
                                                               const RescuePlan* __restrict__ plan, SeedXYOff off, SeedPairsXY xy) {
    const uint64_t p = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (p >= P.n) return;
    if (p + 1 == P.n && lane == 0) {  // closing offsets
        xy.x_off[off.roff[P.n]] = off.xoff[P.n];
        xy.y_off[off.roff[P.n]] = off.yoff[P.n];
    }
    const uint64_t j0 = off.roff[p];
    const uint32_t n = (uint32_t)(off.roff[p + 1] - j0);
    uint64_t xo = off.xoff[p], yo = off.yoff[p];
    for (uint32_t k = 0; k < n; k++) {
        const RescuePlan e = plan[kSlots * p + k];
        const uint64_t v = 4 * p + ((e.info >> 16) & 3);
        const uint64_t ro = P.voff[v];
        const uint32_t L = (uint32_t)(P.voff[v + 1] - ro);
        if (lane == 0) {
            xy.x_off[j0 + k] = xo;
            xy.y_off[j0 + k] = yo;
        }
        for (uint32_t i = lane; i < L; i += 64) xy.x[xo + i] = vreads[ro + i];
        for (uint32_t i = lane; i < e.len; i += 64) xy.y[yo + i] = text[e.lo + i];
        xo += L;
        yo += e.len;
    }
}

// R4: 16 lanes per pair, one lane per planned rescue (kSlots <= 16).  The max of the accepted rescues' keys (rescue_key of
// seed_rescue_rule.h) is the rule's choice.
__global__ __launch_bounds__(256) void se_rescue_pick_kernel(SeedPass P, SeedOut O, PairPrm pp, RescuePrm rp, SeedRescuePlan in,
                                                             SeedRescueAln res) {
    static_assert(kSlots <= 16, "one lane per planned rescue");
    const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t l16 = threadIdx.x & 15;
    if (p >= P.n) return;  // uniform per group of 16
    const RescuePlan* plan = (const RescuePlan*)in.plan;
    const uint64_t j0 = res.roff[p];
    const uint32_t n = (uint32_t)(res.roff[p + 1] - j0);
    if (!n) return;
    PairRule R;
#pragma unroll
    for (int v = 0; v < 5; v++) R.cb[v] = P.coff[4 * p + v];
    uint64_t key = 0;
    if (l16 < n) {
        const RescuePlan e = plan[kSlots * p + l16];
        key = rescue_key(P, e, res.aln[j0 + l16], l16, R.cb[0], pp, rp.min_score);
    }
    key = max16(key);
    if (!key) return;
    const int64_t sum = rescue_key_sum(key);
    if (sum + pp.pen_unpaired < in.own_sum[p]) return;
    const uint32_t k = (uint32_t)key & 15;
    const RescuePlan e = plan[kSlots * p + k];
    const bg_alignment_t q = res.aln[j0 + k];
    const bool fwd = (e.info >> 20) & 1;
    const int m = (e.info >> 21) & 1, other = 1 - m;
    const uint64_t ca = R.cb[0] + (e.info & 0x1FFF);
    // the anchor's mate reports the anchor candidate exactly as the paired call writes a candidate ...
    write_mate(P, O, p, m, l16, R, (uint32_t)(ca - R.cb[2 * m]));
    // ... the other mate the rescued hit on the opposite strand
    const uint64_t r = 2 * p + other;
    write_hit(O, P.r0 + r, l16, &q, e.lo, res.ops, fwd ? BG_HIT_REVERSE : BG_HIT_FORWARD,
              ReadCounts{(uint32_t)(R.cb[2 * other + 2] - R.cb[2 * other]), P.n_hits[4 * p + 2 * other] + P.n_hits[4 * p + 2 * other + 1]});
    if (l16 == 0) {
        const uint64_t as = P.w_lo[ca] + P.aln[ca].ystart, ae = P.w_lo[ca] + P.aln[ca].yend;
        const uint64_t qs = e.lo + q.ystart, qe = e.lo + q.yend;
        bg_pair_hit_t ph;
        memset(&ph, 0, sizeof(ph));
        ph.span = max(ae, qe) - (fwd ? as : qs);
        ph.n_proper = 0;  // the seeded count: a pair with a proper seeded combination is not rescued
        ph.proper = 1;
        O.pairs[P.r0 / 2 + p] = ph;
        O.rescued[P.r0 / 2 + p] = (uint8_t)(other + 1);
    }
}

// totals[3]: the rescued pairs of the whole call, one add per wavefront
__global__ __launch_bounds__(256) void se_rescue_count_kernel(uint64_t n_pairs, const uint8_t* __restrict__ rescued,
                                                              unsigned long long* __restrict__ count) {
    uint32_t n = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * blockDim.x) n += rescued[p] != 0;
#pragma unroll
    for (int o = 32; o; o >>= 1) n += (uint32_t)__shfl_xor((int)n, o);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(count, (unsigned long long)n);
}

}  // namespace

int bg_seed_rescue_count_launch(uint64_t n_pairs, const uint8_t* d_rescued, uint64_t* d_count, hipStream_t st) {
    if (n_pairs == 0) return BG_OK;
    const unsigned grid = (unsigned)std::min<uint64_t>((n_pairs + 255) / 256, 2048);
    se_rescue_count_kernel<<<dim3(grid), dim3(256), 0, st>>>(n_pairs, d_rescued, (unsigned long long*)d_count);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

size_t bg_seed_rescue_plan_bytes(uint64_t n_pairs) { return n_pairs * kSlots * sizeof(RescuePlan); }

int bg_seed_rescue_plan_launch(const SeedPass& P, const SeedOut& O, const bg_pair_params_t* pp, const bg_rescue_params_t* rp, uint64_t n_text,
                               const SeedRescuePlan& plan, hipStream_t st) {
    if (P.n == 0) return BG_OK;
    const RescuePrm rprm{rp->max_anchors, rp->min_score, n_text};
    se_rescue_plan_kernel<<<dim3((unsigned)((P.n * 16 + 255) / 256)), dim3(256), 0, st>>>(P, O, pair_prm(pp), rprm, plan);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

int bg_seed_rescue_gather_launch(const SeedPass& P, const uint8_t* d_vreads, const uint8_t* d_text, const void* d_plan, const SeedXYOff& off,
                                 const SeedPairsXY& xy, hipStream_t st) {
    if (P.n == 0) return BG_OK;
    se_rescue_gather_kernel<<<dim3((unsigned)((P.n + 3) / 4)), dim3(256), 0, st>>>(P, d_vreads, d_text, (const RescuePlan*)d_plan, off, xy);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

int bg_seed_rescue_pick_launch(const SeedPass& P, const SeedOut& O, const bg_pair_params_t* pp, const bg_rescue_params_t* rp,
                               const SeedRescuePlan& plan, const SeedRescueAln& res, hipStream_t st) {
    if (P.n == 0) return BG_OK;
    const RescuePrm rprm{rp->max_anchors, rp->min_score, 0};
    se_rescue_pick_kernel<<<dim3((unsigned)((P.n * 16 + 255) / 256)), dim3(256), 0, st>>>(P, O, pair_prm(pp), rprm, plan, res);
    BG_HIP(hipGetLastError());
    return BG_OK;
}
