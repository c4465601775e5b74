// FM index with 64-bit text positions (round 5, what lifts the engine's 2^32 - 2 symbol limit): the generic search.
//
// The reference indexes with usize throughout — Interval { lower, upper } (/root/reference/src/data_structures/fmindex.rs:
// 70-71), Occ's counters (bwt.rs:94-125), less (bwt.rs:186-199), suffix-array entries (suffix_array.rs:264) — so a text of
// 4.3 G symbols and more is nothing special there; here the rank blocks, less[], l / r and the suffix-array samples were
// uint32 in five kernels and two builders (rounds 1-4: BG_ERR_TOO_LARGE).  The layout fm_kernels.h describes under "64-bit
// positions" — the 64-byte blocks of K5 with counters relative to a superblock, one absolute 64-bit base per code and
// superblock, everything a position can reach in 64 bits — is served by the kernels that are one body over FmLayout<WIDE>
// (the 2x fast search in fm_index.hip, K6 in sa_locate.hip, K7 in fmd_smems.hip, the builders); this file keeps what has a
// schedule of its own on that layout, the generic search, its launcher, and fm_wide_threshold.
//   (the index itself is laid out by fm_build.hip, the one builder of both layouts: the block kernel of the narrow index, a
//    64-bit scan of the per-block counts, heads relative to the superblock's first block)
//   fmw_search2x_kernel FMIndexable::backward_search (fmindex.rs:144-208), the generic search: two queries per quad, l and r
//                       64-bit, Occ::get = base[superblock][code] + cnt[code] + popcount; byte, packed and seed-window
//                       patterns.  fm_index.hip's fm_search decides when it runs: alone, or behind the 2x fast kernel
//                       (fm_search_fast2x_kernel<WIDE>, on the 2-step blocks fm_step2.hip builds) for what that defers
// Narrow indexes (n < 2^32 - 1) never come here: their kernels, layouts and speed are those of rounds 1-4.  A wide
// index takes packed patterns, 2-step rank blocks, seed-and-extend and the FMD-index kernels (fmd_smems.hip,
// through the entry points with 64-bit records).  What is NOT offered on one (BG_ERR_UNSUPPORTED): alphabets that need
// rank bit vectors, the FMD entry points with 32-bit records, and the counted search (bg_fm_backward_search_count_lines_dev).
#include <algorithm>
#include <cstring>
#include <string.h>
#include <vector>

#include "fm_kernels.h"

using namespace bgfm;

uint64_t fm_wide_threshold(const bg_ctx* ctx) { return ctx ? ctx->fm_wide_from : 0xFFFFFFFFull; }

namespace {

// K5 on 64-bit positions: FMIndexable::backward_search (fmindex.rs:144-208) with TWO queries per quad (round 5; what
// fm_search_fast2x_kernel is to the narrow index, fm_index.hip): a step is one dependent block access, eight wavefronts per
// SIMD are all the hardware holds, and the parallelism left to add is a second independent query inside the wavefront.
// Phase A reads both streams' symbols and classes and issues their block loads and superblock bases — unconditional, in one
// basic block (a stream without a coded symbol reads block 0; the line of l - 1 is requested even where it is the line of
// r) — phase B ranks and updates both.  Stream (quad, u) takes queries (2 quad + u) + k * 2 quads.  On the 4.4 G-symbol
// index: 302 M queries/s with one query per quad, 404 M with two (profiles/r05_fm_wide_4g4.json), same arrays.
// Round 6: the flavours the narrow generic kernel has — SEEDS (the seed windows of a batch of reads: query q is seed q % S of
// read q / S, fm_kernels.h SeedSrc), PACKED (`pat` is a 2-bit stream in the index's codes, offsets in symbols: the class of a
// symbol is its code) and DEFER (only the queries the 2x fast kernel in front left tagged kTagDeferred).
template <bool SEEDS, bool PACKED, bool DEFER>
__global__ __launch_bounds__(256) void fmw_search2x_kernel(FmWideDev fm, uint64_t n_q, const uint8_t* __restrict__ pat,
                                                           const uint64_t* __restrict__ pat_off, uint8_t* __restrict__ tag,
                                                           uint64_t* __restrict__ lower, uint64_t* __restrict__ upper,
                                                           uint32_t* __restrict__ matched_len, const SeedSrc seeds) {
    constexpr int U = 2;
    __shared__ uint16_t s_class[256];
    __shared__ uint64_t s_less[256];
    __shared__ uint64_t s_exc[kMaxExcLds];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) {
        s_class[i] = fm.sym_class[i];
        // PACKED: entry c (< 4) is less[] of the byte that code c stands for
        s_less[i] = (PACKED && i < 4) ? fm.less[(seeds.code_bytes >> (8 * i)) & 0xFFu] : fm.less[i];
    }
    for (uint32_t i = threadIdx.x; i < fm.n_exc; i += blockDim.x) s_exc[i] = fm.exc_pos[i];
    __syncthreads();
    const uint32_t* __restrict__ pk = (const uint32_t*)pat;
    const uint32_t t = threadIdx.x & 3;
    const uint64_t n_streams = (uint64_t)gridDim.x * (blockDim.x >> 2) * U;
    struct St {
        uint64_t q, off, l, r;
        uint32_t pos, matched, a_next;
        bool active;
    };
    St S[U];
    auto emit = [&](uint64_t q, uint32_t tg, uint64_t lo, uint64_t hi, uint32_t ml) {
        if (t == 0) {
            tag[q] = (uint8_t)tg;
            lower[q] = lo;
            upper[q] = hi;
            matched_len[q] = ml;
        }
    };
    auto symbol = [&](uint64_t at) -> uint32_t {  // the pattern symbol at stream position `at`: a byte, or a 2-bit code
        if (PACKED) return (pk[at >> 4] >> (2 * ((uint32_t)at & 15u))) & 3u;
        return pat[at];
    };
    auto fetch = [&](St& s) {  // the stream's next non-empty query; empty patterns are Absent at once (fmindex.rs:185-207)
        s.active = false;
        while (s.q < n_q) {
            if (DEFER && tag[s.q] != kTagDeferred) {
                s.q += n_streams;
                continue;
            }
            const uint32_t len = query_span<SEEDS>(pat_off, seeds, s.q, s.off);
            if (len) {
                s.pos = len;
                s.l = 0;
                s.r = fm.n - 1;  // fmindex.rs:148
                s.matched = 0;
                s.a_next = symbol(s.off + len - 1);
                s.active = true;
                return;
            }
            emit(s.q, BG_FM_ABSENT, 0, 0, 0);
            s.q += n_streams;
        }
    };
#pragma unroll
    for (int u = 0; u < U; u++) {
        S[u].q = ((uint64_t)blockIdx.x * (blockDim.x >> 2) + (threadIdx.x >> 2)) * U + u;
        S[u].off = S[u].l = S[u].r = 0;
        S[u].pos = S[u].matched = S[u].a_next = 0;
        fetch(S[u]);
    }
    for (;;) {
        bool any_active = false;
#pragma unroll
        for (int u = 0; u < U; u++) any_active |= S[u].active;
        if (!__any(any_active)) break;
        // ---- phase A
        uint4 vr[U], vl[U];
        uint64_t base_r[U], base_l[U], br[U], bl[U];
        uint32_t orr[U], ol[U], a[U], cls[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            St& s = S[u];
            a[u] = s.a_next;
            const uint32_t p1 = s.active ? s.pos - 1u : 0u;
            if (s.active && p1) s.a_next = symbol(s.off + p1 - 1);  // (address independent of the ranks)
            cls[u] = PACKED ? a[u] : (uint32_t)s_class[a[u]];
            const bool coded = s.active && cls[u] < 4;
            const uint64_t r_ = coded ? s.r : 0, l_ = coded && s.l ? s.l - 1 : 0;
            br[u] = r_ / kSymPerBlock;
            bl[u] = coded && s.l ? l_ / kSymPerBlock : br[u];
            orr[u] = (uint32_t)(r_ - br[u] * kSymPerBlock);
            ol[u] = (uint32_t)(l_ - bl[u] * kSymPerBlock);
            const uint32_t code = coded ? cls[u] : 0u;
            vr[u] = fm.blocks[br[u] * 4 + t];
            vl[u] = fm.blocks[bl[u] * 4 + t];
            base_r[u] = fm.sb[(br[u] >> fm.sb_shift) * 4 + code];  // (sb_base() written out: through the helper the loads are scheduled differently)
            base_l[u] = fm.sb[(bl[u] >> fm.sb_shift) * 4 + code];
        }
        // ---- phase B: one iteration of the loop at fmindex.rs:160-182 per stream
#pragma unroll
        for (int u = 0; u < U; u++) {
            St& s = S[u];
            if (!s.active) continue;
            s.pos -= 1;
            const uint64_t less_a = s_less[a[u]];
            uint64_t occ_r = 0, occ_l = 0;
            bool stop = false;
            uint32_t stop_tag = BG_FM_PARTIAL;
            if (!PACKED && cls[u] == kClsPanic) {
                stop = true;
                stop_tag = BG_FM_PANIC;
            } else if (PACKED || cls[u] < 4) {
                occ_r = base_r[u] + (uint64_t)quad_sum(block_part(vr[u], t, orr[u], cls[u]));
                if (s.l > 0) occ_l = base_l[u] + (uint64_t)quad_sum(block_part(vl[u], t, ol[u], cls[u]));
                if (cls[u] == 0 && fm.n_exc) {  // sparse exceptions sit in the stream as code 0
                    occ_r -= count_le(s_exc, 0u, fm.n_exc, s.r);
                    if (s.l > 0) occ_l -= count_le(s_exc, 0u, fm.n_exc, s.l - 1);
                }
            } else if (cls[u] >= kClsSparse) {  // (no dense symbols on a wide index)
                const uint32_t e = cls[u] - kClsSparse;
                const uint32_t lo = fm.sparse_off[e], hi = fm.sparse_off[e + 1];
                occ_r = count_le(fm.exc_sym_pos, lo, hi, s.r) - lo;
                if (s.l > 0) occ_l = count_le(fm.exc_sym_pos, lo, hi, s.l - 1) - lo;
            }  // kClsZero: both stay 0
            const uint64_t pl = s.l, pr = s.r;
            if (!stop) {
                if (occ_r == 0) {  // fmindex.rs:167-170
                    stop = true;
                } else {
                    s.l = less_a + occ_l;  // fmindex.rs:171
                    s.r = less_a + occ_r - 1;
                    if (s.l > s.r)  // fmindex.rs:177-180
                        stop = true;
                    else
                        s.matched += 1;
                }
            }
            if (stop) {
                if (stop_tag == BG_FM_PANIC)
                    emit(s.q, BG_FM_PANIC, 0, 0, s.matched);
                else if (s.matched)
                    emit(s.q, BG_FM_PARTIAL, pl, pr + 1, s.matched);
                else
                    emit(s.q, BG_FM_ABSENT, 0, 0, 0);
                s.q += n_streams;
                fetch(s);
            } else if (s.pos == 0) {
                emit(s.q, BG_FM_COMPLETE, s.l, s.r + 1, s.matched);
                s.q += n_streams;
                fetch(s);
            }
        }
    }
}

}  // namespace

template <bool SEEDS, bool PACKED, bool DEFER>
int fm_wide_search_launch(bg_fm* fm, uint64_t n_q, const uint8_t* d_pat, const uint64_t* d_pat_off, uint8_t* d_tag, uint64_t* d_lower,
                          uint64_t* d_upper, uint32_t* d_matched_len, const SeedSrc& src, hipStream_t st) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fmw_search2x_kernel<SEEDS, PACKED, DEFER>, 256, 0) != hipSuccess || per_cu < 1) per_cu = 4;
    const uint64_t blocks = std::min<uint64_t>((n_q + 127) / 128, 256ull * (uint64_t)per_cu);
    fmw_search2x_kernel<SEEDS, PACKED, DEFER><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(fm->wdev, n_q, d_pat, d_pat_off, d_tag, d_lower, d_upper,
                                                                                          d_matched_len, src);
    BG_HIP(hipGetLastError());
    return BG_OK;
}
// the flavours fm_search (fm_index.hip) launches
#define FMW_SEARCH_LAUNCH(SEEDS, PACKED, DEFER)                                                                                       \
    template int fm_wide_search_launch<SEEDS, PACKED, DEFER>(bg_fm*, uint64_t, const uint8_t*, const uint64_t*, uint8_t*, uint64_t*, \
                                                             uint64_t*, uint32_t*, const SeedSrc&, hipStream_t);
FMW_SEARCH_LAUNCH(false, false, false)
FMW_SEARCH_LAUNCH(false, false, true)
FMW_SEARCH_LAUNCH(true, false, false)
FMW_SEARCH_LAUNCH(true, false, true)
FMW_SEARCH_LAUNCH(false, true, false)
FMW_SEARCH_LAUNCH(false, true, true)
#undef FMW_SEARCH_LAUNCH
