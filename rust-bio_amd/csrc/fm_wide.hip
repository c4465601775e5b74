// FM index with 64-bit text positions (round 5): what lifts the engine's 2^32 - 2 symbol limit.
//
// The reference indexes with usize throughout — Interval { lower, upper } (/root/reference/src/data_structures/fmindex.rs:
// 70-71), Occ's counters (bwt.rs:94-125), less (bwt.rs:186-199), suffix-array entries (suffix_array.rs:264) — so a text of
// 4.3 G symbols and more is nothing special there; here the rank blocks, less[], l / r and the suffix-array samples were
// uint32 in five kernels and two builders (rounds 1-4: BG_ERR_TOO_LARGE).  This file is the same search on the layout
// fm_kernels.h describes under "64-bit positions": the 64-byte blocks of K5 with counters relative to a superblock, one
// absolute 64-bit base per code and superblock, everything a position can reach in 64 bits.
//   (the index itself is laid out by fm_build.hip, the one builder of both layouts: the block kernel of the narrow index, a
//    64-bit scan of the per-block counts, heads relative to the superblock's first block)
//   fmw_search2x_kernel FMIndexable::backward_search (fmindex.rs:144-208), the generic search: two queries per quad, l and r
//                       64-bit, Occ::get = base[superblock][code] + cnt[code] + popcount; byte, packed and seed-window
//                       patterns.  fm_index.hip's fm_search decides when it runs: alone, or behind the 2x fast kernel
//                       (fm_search_fast2x_kernel<WIDE>, on the 2-step blocks fm_step2.hip builds) for what that defers
//   fmw_sampled_get_kernel / fmw_raw_get_kernel   Interval::occ over a SampledSuffixArray / a raw one (suffix_array.rs:
//                       134-184) with 64-bit samples
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

constexpr uint32_t kWideMaxExc = kMaxExcLds;

// Occ::get(r, code) for the quad: the block's line is in `v` (lane t holds bytes [16t, 16t + 16)), `base` the superblock's
// absolute count of the code
__device__ __forceinline__ uint64_t wide_rank(const FmWideDev& fm, const uint4 v, uint32_t t, uint64_t blk, uint32_t o, uint32_t code) {
    return fm.sb[(blk >> fm.sb_shift) * 4 + code] + (uint64_t)quad_sum(block_part(v, t, o, code));
}

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
    __shared__ uint64_t s_exc[kWideMaxExc];
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
            uint32_t len;
            if (SEEDS) {
                const uint64_t rd = s.q / seeds.S;
                const uint32_t k = (uint32_t)(s.q - rd * seeds.S);
                const uint64_t o = pat_off[rd];
                s.off = o + (uint64_t)k * seeds.stride;
                len = (uint64_t)k * seeds.stride + seeds.seed_len <= pat_off[rd + 1] - o ? seeds.seed_len : 0u;
            } else {
                s.off = pat_off[s.q];
                len = (uint32_t)(pat_off[s.q + 1] - s.off);
            }
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
            base_r[u] = fm.sb[(br[u] >> fm.sb_shift) * 4 + code];
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
                    occ_r -= count_le64(s_exc, 0u, fm.n_exc, s.r);
                    if (s.l > 0) occ_l -= count_le64(s_exc, 0u, fm.n_exc, s.l - 1);
                }
            } else if (cls[u] >= kClsSparse) {  // (no dense symbols on a wide index)
                const uint32_t e = cls[u] - kClsSparse;
                const uint32_t lo = fm.sparse_off[e], hi = fm.sparse_off[e + 1];
                occ_r = count_le64(fm.exc_sym_pos, lo, hi, s.r) - lo;
                if (s.l > 0) occ_l = count_le64(fm.exc_sym_pos, lo, hi, s.l - 1) - lo;
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

struct SaWideDev {
    const uint64_t* sa;         // raw SA or the samples
    const uint64_t* extra_row;  // sorted
    const uint64_t* extra_pos;
    const uint8_t* exc_byte;    // byte of exception e (parallel to FmWideDev::exc_pos)
    uint32_t n_extra;
    uint32_t rate;
    uint32_t sentinel;
    uint32_t code_byte;         // byte of code c in bits [8c, 8c+8)
};

__global__ __launch_bounds__(256) void fmw_raw_get_kernel(const uint64_t* __restrict__ sa, uint64_t n_text, uint64_t n, const uint64_t* index,
                                                          uint64_t* pos_out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t r = index[i];
    pos_out[i] = r < n_text ? sa[r] : BG_SA_NONE;
}

// SampledSuffixArray::get (suffix_array.rs:157-184): every row LF-walks until it reaches a sampled row or a row whose BWT
// byte is the sentinel; a quad per row, the rank block and the word that holds bwt[pos] loaded together
__global__ __launch_bounds__(256) void fmw_sampled_get_kernel(FmWideDev fm, SaWideDev sa, uint64_t n, const uint64_t* index, uint64_t* pos_out) {
    __shared__ uint16_t s_class[256];
    __shared__ uint64_t s_less[256];
    __shared__ uint64_t s_exc[kWideMaxExc];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) {
        s_class[i] = fm.sym_class[i];
        s_less[i] = fm.less[i];
    }
    for (uint32_t i = threadIdx.x; i < fm.n_exc; i += blockDim.x) s_exc[i] = fm.exc_pos[i];
    __syncthreads();
    const uint32_t t = threadIdx.x & 3;
    const uint64_t n_quads = (uint64_t)gridDim.x * (blockDim.x >> 2);
    uint64_t q = (uint64_t)blockIdx.x * (blockDim.x >> 2) + (threadIdx.x >> 2);
    const uint32_t* blocks32 = (const uint32_t*)fm.blocks;
    bool active = false;
    uint64_t pos = 0, offset = 0;
    auto emit = [&](uint64_t v) {
        if (t == 0) pos_out[q] = v;
    };
    auto fetch = [&]() {
        active = false;
        while (q < n) {
            const uint64_t r = index[q];
            if (r < fm.n) {
                pos = r;
                offset = 0;
                active = true;
                return;
            }
            emit(BG_SA_NONE);  // SuffixArray::get -> None
            q += n_quads;
        }
    };
    fetch();
    while (__any(active)) {
        if (active) {
            if (pos % sa.rate == 0) {  // suffix_array.rs:162-164
                emit(sa.sa[pos / sa.rate] + offset);
                q += n_quads;
                fetch();
                continue;
            }
            const uint64_t pb = pos / kSymPerBlock, rb = (pos - 1) / kSymPerBlock;
            const uint32_t po = (uint32_t)(pos - pb * kSymPerBlock), ro = (uint32_t)((pos - 1) - rb * kSymPerBlock);
            const uint4 vr = fm.blocks[rb * 4 + t];
            const uint32_t word = blocks32[pb * 16 + 4 + (po >> 4)];
            const uint32_t code = (word >> (2 * (po & 15))) & 3u;
            uint32_t c = (sa.code_byte >> (8 * code)) & 255u;
            if (code == 0 && fm.n_exc) {  // sparse exceptions sit in the stream as code 0
                const uint32_t e = count_le64(s_exc, 0u, fm.n_exc, pos);
                if (e > 0 && s_exc[e - 1] == pos) c = sa.exc_byte[e - 1];
            }
            if (c == sa.sentinel) {  // suffix_array.rs:168-175
                uint32_t lo = 0, hi = sa.n_extra;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (sa.extra_row[mid] < pos)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                emit(lo < sa.n_extra && sa.extra_row[lo] == pos ? sa.extra_pos[lo] + offset : BG_SA_PANIC);
                q += n_quads;
                fetch();
                continue;
            }
            // pos = less[c] + occ.get(bwt, pos - 1, c)  (suffix_array.rs:177-178)
            const uint32_t cls = s_class[c];
            uint64_t occ = 0;
            if (cls < 4) {
                occ = wide_rank(fm, vr, t, rb, ro, cls);
                if (cls == 0 && fm.n_exc) occ -= count_le64(s_exc, 0u, fm.n_exc, pos - 1);
            } else if (cls != kClsPanic && cls >= kClsSparse) {
                const uint32_t e = cls - kClsSparse;
                const uint32_t lo = fm.sparse_off[e], hi = fm.sparse_off[e + 1];
                occ = count_le64(fm.exc_sym_pos, lo, hi, pos - 1) - lo;
            }
            pos = s_less[c] + occ;
            offset += 1;
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

int fm_wide_sa_get(bg_fm* fm, uint64_t n, const uint64_t* d_index, uint64_t* d_pos, hipStream_t st) {
    if (n == 0) return BG_OK;
    if (fm->sa_kind == 1) {
        fmw_raw_get_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>((const uint64_t*)fm->d_sa, fm->wdev.n, n, d_index, d_pos);
    } else {
        SaWideDev sa = {};
        sa.sa = (const uint64_t*)fm->d_sa;
        sa.extra_row = (const uint64_t*)fm->d_extra_row;
        sa.extra_pos = (const uint64_t*)fm->d_extra_pos;
        sa.exc_byte = (const uint8_t*)fm->d_exc_byte;
        sa.n_extra = (uint32_t)fm->n_extra;
        sa.rate = fm->sa_rate;
        sa.sentinel = fm->sa_sentinel;
        sa.code_byte = (uint32_t)fm->code_byte[0] | (uint32_t)fm->code_byte[1] << 8 | (uint32_t)fm->code_byte[2] << 16 |
                       (uint32_t)fm->code_byte[3] << 24;
        const uint64_t blocks = std::min<uint64_t>((n + 63) / 64, 256 * 8);
        fmw_sampled_get_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(fm->wdev, sa, n, d_index, d_pos);
    }
    BG_HIP(hipGetLastError());
    return BG_OK;
}
