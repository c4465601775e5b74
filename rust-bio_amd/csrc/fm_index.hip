// FM-index backward search on gfx950 (kernel K5); the index is laid out by fm_build.hip.
//
// Replaces, for a batch of patterns, FMIndexable::backward_search
// (/root/reference/src/data_structures/fmindex.rs:144-208) with Occ::get
// (/root/reference/src/data_structures/bwt.rs:129-182) and Less[a] (fmindex.rs:228-230).
//
// Device layout (ours; results equal the byte-table definition for every (r, a)):
//   * the BWT is re-coded to 2 bits/symbol: the four most frequent byte values get codes
//     0..3; every other byte value that occurs (the sentinel `$`, stray N, ...) is an
//     *exception*: stored as code 0 in the packed stream and listed (sorted) on the side;
//   * one 64-byte block per 192 symbols, self-contained for a rank query:
//       uint32 cnt[4]   occurrences of code c in bwt[0 .. 192*b)      (16 B)
//       uint32 sym[12]  192 symbols, 16 per word, symbol s at bits [2s, 2s+2)   (48 B)
//     so Occ::get(r, a) = cnt[code(a)] + popcount(matches in the first r%192+1 symbols)
//     costs exactly one 64-B line;
//   * a quad of 4 lanes serves one query: lane t of the quad loads bytes [16t, 16t+16) of
//     the block (one coalesced 64-B request per rank), counts its share, and the quad
//     reduces with two DPP adds.  rank(l-1) and rank(r) are issued together; when both fall
//     in the same block (the common case once the interval is narrow) the line is loaded once;
//   * symbol classes, Less[] and the exception list are staged in LDS;
//   * general alphabets (bwt.rs:94-182 works for any): when more than 1024 BWT positions hold a byte outside the
//     four most frequent ones (a genome with runs of N, a protein text), only the THREE most frequent bytes keep
//     2-bit codes (1..3; code 0 = "something else"), the rare bytes stay sorted lists (<= 1024 positions in all),
//     and every other byte gets a one-hot rank bit vector of its own — 64-byte blocks of a 32-bit counter + 480
//     bits — so that Occ::get is still exactly one 64-byte line, whatever the symbol.  n / 7.5 bytes per such
//     symbol (a 20-letter protein text: 2.7 bytes per symbol of index); the raw BWT is kept for K6 (bwt[pos]).
// No MFMA: this is a latency/bandwidth-bound table walk (DESIGN.md §FM roofline).
#include <cstring>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>

#include "fm_kernels.h"

using namespace bgfm;

namespace {

// SEEDS: the patterns are the seed windows of a batch of reads (seed-and-extend, seed_extend.hip) — query q is
// seed q % S of read q / S: pat[pat_off[r] + k * stride ..+ seed_len) while it fits in the read (else an empty
// pattern: Absent), so overlapping windows need no copy of the reads.
// PACKED: `pat` is a 2-bit stream (16 symbols per little-endian dword, symbol s in bits 2 (s % 16) of dword s / 16, the
// codes being the index's own: bg_fm_pattern_codes / bg_pack2_dev) and `pat_off` counts SYMBOLS: a pattern costs a dword
// load every 16 steps instead of a byte load per step, its symbols are codes already (no class lookup, none of the
// sparse / dense / panic arms).  Only for indexes whose four codes are all symbols (DNA-like BWTs).
// COUNT: the block loads of the launch are counted (bench.py: requested lines against the gather ceiling of
// tools/microbench/ub_gather64.hip); the results are the same.
// (the DEFER launch reads every tag once — n_q bytes, ~10 us per 10 M queries — and the fast kernel writes every tag it
//  owns, deferred or answered, so a caller's stale tag buffer cannot fake a deferral)
// DEFER: only the queries whose tag is kTagDeferred are searched (second launch behind a fast kernel)
template <bool SEEDS, bool PACKED, bool COUNT, bool DEFER>
__global__ __launch_bounds__(256) void fm_backward_search_kernel(
    FmDev fm, uint64_t n_q, const uint8_t* __restrict__ pat, const uint64_t* __restrict__ pat_off,
    uint8_t* __restrict__ tag, uint64_t* __restrict__ lower, uint64_t* __restrict__ upper,
    uint32_t* __restrict__ matched_len, const SeedSrc seeds) {
    __shared__ uint16_t s_class[256];
    __shared__ uint32_t s_less[256];
    __shared__ uint32_t s_exc[kMaxExcLds];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) {
        s_class[i] = fm.sym_class[i];
        // PACKED: entry c (< 4) is less[] of the byte that code c stands for
        s_less[i] = (PACKED && i < 4) ? fm.less[(seeds.code_bytes >> (8 * i)) & 0xFFu] : fm.less[i];
    }
    for (uint32_t i = threadIdx.x; i < fm.n_exc; i += blockDim.x) s_exc[i] = fm.exc_pos[i];  // n_exc <= kMaxExcLds
    __syncthreads();
    const uint32_t* __restrict__ pk = (const uint32_t*)pat;
    uint32_t pk_cur = 0;      // PACKED: the dword that holds the next symbol
    uint32_t n_lines = 0;     // COUNT

    const uint32_t t = threadIdx.x & 3;
    const uint64_t n_quads = (uint64_t)gridDim.x * (blockDim.x >> 2);
    uint64_t q = (uint64_t)blockIdx.x * (blockDim.x >> 2) + (threadIdx.x >> 2);

    // per-query state (uniform inside a quad)
    bool active = false;
    uint64_t off = 0;
    uint32_t len = 0, pos = 0, l = 0, r = 0, matched = 0;
    uint32_t a_next = 0;

    auto emit = [&](uint32_t tg, uint32_t lo, uint32_t hi, uint32_t ml) {
        if (t == 0) {
            tag[q] = (uint8_t)tg;
            lower[q] = lo;
            upper[q] = hi;
            matched_len[q] = ml;
        }
    };
    // load the next non-empty query into the state; empty patterns are Absent at once
    // (matched_len == 0, fmindex.rs:185-207)
    auto fetch = [&]() {
        active = false;
        while (q < n_q) {
            if (DEFER && tag[q] != kTagDeferred) {
                q += n_quads;
                continue;
            }
            len = query_span<SEEDS>(pat_off, seeds, q, off);
            if (len) {
                pos = len;
                l = 0;
                r = fm.n - 1;  // fmindex.rs:148
                matched = 0;
                if (PACKED) {
                    const uint64_t gs = off + pos - 1;
                    pk_cur = pk[gs >> 4];
                    a_next = (pk_cur >> (2 * ((uint32_t)gs & 15u))) & 3u;
                } else {
                    a_next = pat[off + pos - 1];
                }
                active = true;
                return;
            }
            emit(BG_FM_ABSENT, 0, 0, 0);
            q += n_quads;
        }
    };
    fetch();

    while (__any(active)) {
        if (active) {
            // one iteration of the loop at fmindex.rs:160-182
            const uint32_t a = a_next;
            pos -= 1;
            if (PACKED) {
                if (pos) {  // the next symbol: a new dword every 16 steps
                    const uint64_t gs = off + pos - 1;
                    if (((uint32_t)gs & 15u) == 15u) pk_cur = pk[gs >> 4];
                    a_next = (pk_cur >> (2 * ((uint32_t)gs & 15u))) & 3u;
                }
            } else if (pos) {
                a_next = pat[off + pos - 1];  // prefetch; address independent of the ranks
            }
            const uint32_t cls = PACKED ? a : (uint32_t)s_class[a];
            const uint32_t less_a = s_less[a];
            uint32_t occ_r = 0, occ_l = 0;
            bool stop = false;
            uint32_t stop_tag = BG_FM_PARTIAL;
            if (!PACKED && cls == kClsPanic) {
                stop = true;
                stop_tag = BG_FM_PANIC;
            } else if (PACKED || cls < 4) {
                const uint32_t br = r / kSymPerBlock, orr = r - br * kSymPerBlock;
                const uint4 vr = fm.blocks[(uint64_t)br * 4 + t];
                uint4 vl = vr;
                uint32_t ol = 0;
                if (l > 0) {
                    const uint32_t bl = (l - 1) / kSymPerBlock;
                    ol = (l - 1) - bl * kSymPerBlock;
                    if (bl != br) {
                        vl = fm.blocks[(uint64_t)bl * 4 + t];
                        if (COUNT) n_lines += 1;
                    }
                }
                if (COUNT) n_lines += 1;
                occ_r = quad_sum(block_part(vr, t, orr, cls));
                if (l > 0) occ_l = quad_sum(block_part(vl, t, ol, cls));
                if (cls == 0 && fm.n_exc) {  // sparse exceptions sit in the stream as code 0
                    if (fm.n_exc == 1) {     // a text with one sentinel and nothing else outside its four letters: no search loop
                        const uint32_t e0 = s_exc[0];
                        occ_r -= e0 <= r ? 1u : 0u;
                        if (l > 0) occ_l -= e0 <= l - 1 ? 1u : 0u;
                    } else {
                        occ_r -= count_le(s_exc, 0u, fm.n_exc, r);
                        if (l > 0) occ_l -= count_le(s_exc, 0u, fm.n_exc, l - 1);
                    }
                }
            } else if (PACKED) {
            } else if (cls >= kClsDense) {  // one-hot bit vector of this symbol: one 64-byte block per rank
                const uint32_t d = cls - kClsDense;
                uint32_t orr, ol = 0;
                const uint4 vr = bv_load(fm, d, r, t, orr);
                uint4 vl = vr;
                if (l > 0) {
                    if ((l - 1) / kBvBits != r / kBvBits)
                        vl = bv_load(fm, d, l - 1, t, ol);
                    else
                        ol = (l - 1) % kBvBits;
                }
                occ_r = quad_sum(bv_part(vr, t, orr));
                if (l > 0) occ_l = quad_sum(bv_part(vl, t, ol));
            } else if (cls >= kClsSparse) {
                const uint32_t e = cls - kClsSparse;
                const uint32_t lo = fm.sparse_off[e], hi = fm.sparse_off[e + 1];
                occ_r = count_le(fm.exc_sym_pos, lo, hi, r) - lo;
                if (l > 0) occ_l = count_le(fm.exc_sym_pos, lo, hi, l - 1) - lo;
            }  // kClsZero: both stay 0
            const uint32_t pl = l, pr = r;
            if (!stop) {
                if (occ_r == 0) {  // fmindex.rs:167-170
                    stop = true;
                } else {
                    l = less_a + occ_l;  // fmindex.rs:171
                    r = less_a + occ_r - 1;
                    if (l > r)  // fmindex.rs:177-180
                        stop = true;
                    else
                        matched += 1;
                }
            }
            if (stop) {
                if (stop_tag == BG_FM_PANIC)
                    emit(BG_FM_PANIC, 0, 0, matched);
                else if (matched)
                    emit(BG_FM_PARTIAL, pl, pr + 1, matched);
                else
                    emit(BG_FM_ABSENT, 0, 0, 0);
                q += n_quads;
                fetch();
            } else if (pos == 0) {
                emit(BG_FM_COMPLETE, l, r + 1, matched);
                q += n_quads;
                fetch();
            }
        }
    }
    if (COUNT && t == 0 && n_lines) atomicAdd(seeds.lines, (unsigned long long)n_lines);
}

// K5 fast path for byte patterns over a DNA-like index (four 2-bit codes, no dense symbols): when a quad takes its next
// query, the wavefront turns the pattern into 2-bit codes — a coalesced byte load and a class lookup per 64 symbols, the
// 16 lanes of a DPP row OR their codes into a dword — parked in the quad's LDS slot (kFastSyms symbols); the LF loop
// then is the packed kernel's: one LDS read per
// step for the symbol, no byte load, no class / less lookups by byte, none of the sparse / dense / panic arms.  A
// pattern with a byte outside the four codes (N, lower case, anything that would make the reference panic) or longer
// than the slot is tagged kTagDeferred and answered by the generic kernel launched right behind (DEFER).  Same results
// (tests/test_gpu_fm.py, test_gpu_pack2.py); 466 -> ~560 M queries/s on the 100 Mbp index.
// PACKED: `pat` is a 2-bit stream already (pack2.hip, the index's codes; offsets in symbols): taking a query is a funnel
// shift of up to 16 dwords into the slot, nothing can be "bad".
// Single LF steps on the 1-step blocks: what answers an index without 2-step rank blocks, and searches with "no_step2"
// set; fm_search_fast2x_kernel is the same search on the 2-step blocks.
template <bool SEEDS, bool COUNT, bool PACKED>
__global__ __launch_bounds__(256) void fm_search_fast_kernel(FmDev fm, uint64_t n_q, const uint8_t* __restrict__ pat,
                                                             const uint64_t* __restrict__ pat_off, uint8_t* __restrict__ tag,
                                                             uint64_t* __restrict__ lower, uint64_t* __restrict__ upper,
                                                             uint32_t* __restrict__ matched_len, const SeedSrc seeds) {
    __shared__ uint16_t s_class[256];
    __shared__ uint32_t s_less4[4];
    __shared__ uint32_t s_exc[kMaxExcLds];
    // (+1 and its zero store: no code here reads that dword, but without them the prologue compiles differently — 45
    //  VGPRs instead of 43; with them the kernel keeps the instructions it had when a 2-step branch still read it)
    __shared__ uint32_t s_pk[64 * (kFastSyms / 16) + 1];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) s_class[i] = fm.sym_class[i];
    if (threadIdx.x < 4) s_less4[threadIdx.x] = fm.less[(seeds.code_bytes >> (8 * threadIdx.x)) & 0xFFu];
    for (uint32_t i = threadIdx.x; i < fm.n_exc; i += blockDim.x) s_exc[i] = fm.exc_pos[i];
    if (threadIdx.x == 0) s_pk[64 * (kFastSyms / 16)] = 0;
    __syncthreads();

    const uint32_t t = threadIdx.x & 3;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t* const slot = s_pk + (threadIdx.x >> 2) * (kFastSyms / 16);
    uint32_t* const wave_slots = s_pk + (threadIdx.x >> 6) * 16 * (kFastSyms / 16);  // the 16 slots of this wavefront
    const uint64_t n_quads = (uint64_t)gridDim.x * (blockDim.x >> 2);
    uint64_t q = (uint64_t)blockIdx.x * (blockDim.x >> 2) + (threadIdx.x >> 2);
    bool active = false, need = true;
    uint32_t pos = 0, l = 0, r = 0, matched = 0, n_lines = 0;

    // Taking the next query is a job of the WHOLE wavefront, one waiting quad at a time (round 3; a quad packing its own
    // pattern ran ~300 instructions with 4 of 64 lanes active, 15 % of the kernel): the quad's query index, pattern
    // offset and length are wave-uniform (read from the quad's leader lane), lane i looks symbol base + i up — one
    // coalesced byte load per 64 symbols — and the 16 lanes of a DPP row OR their 2-bit codes into the dword of their 16
    // symbols, which the row's last lane writes into the quad's LDS slot.  ~30 instructions per query.
    auto fetch_all = [&]() {
        uint64_t waiting = __ballot(need && t == 0);  // leaders of the quads that wait
        while (waiting) {
            const uint32_t leader = (uint32_t)__ffsll((unsigned long long)waiting) - 1u;
            const bool mine = (lane >> 2) == (leader >> 2);
            const uint64_t qs = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(q >> 32), leader) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)q, leader);
            if (qs >= n_q) {  // nothing left for this quad
                if (mine) {
                    need = false;
                    active = false;
                }
                waiting &= waiting - 1;
                continue;
            }
            uint64_t off;
            uint32_t len;
            if (SEEDS) {
                const uint64_t rd = qs / seeds.S;
                const uint32_t k = (uint32_t)(qs - rd * seeds.S);
                const uint64_t o = pat_off[rd];
                off = o + (uint64_t)k * seeds.stride;
                len = (uint64_t)k * seeds.stride + seeds.seed_len <= pat_off[rd + 1] - o ? seeds.seed_len : 0u;
            } else {
                off = pat_off[qs];
                const uint64_t len64 = pat_off[qs + 1] - off;
                len = len64 > kFastSyms ? kFastSyms + 1 : (uint32_t)len64;
            }
            bool bad = len > kFastSyms;
            if (PACKED && len && !bad) {
                uint32_t* const dst = wave_slots + (leader >> 2) * (kFastSyms / 16);
                const uint32_t* pk = (const uint32_t*)pat;
                if (lane < ((len + 15u) >> 4)) {  // dword `lane` of the slot: symbols off + 16 lane ... of the stream
                    const uint64_t w0 = (off >> 4) + lane;
                    const uint32_t sh = 2u * ((uint32_t)off & 15u);
                    const uint32_t lo = pk[w0], hi = pk[w0 + 1];  // the stream is padded by one dword
                    dst[lane] = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
                }
            } else if (len && !bad) {
                uint32_t* const dst = wave_slots + (leader >> 2) * (kFastSyms / 16);
                for (uint32_t base = 0; base < len; base += 64) {
                    const uint32_t idx = base + lane;
                    uint32_t c = 0;
                    if (idx < len) {
                        c = s_class[pat[off + idx]];
                        bad = bad || c >= 4;
                    }
                    uint32_t word = (c & 3u) << (2 * (lane & 15u));
                    word |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)word, 0x111 /*row_shr:1*/, 0xf, 0xf, true);
                    word |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)word, 0x112 /*row_shr:2*/, 0xf, 0xf, true);
                    word |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)word, 0x114 /*row_shr:4*/, 0xf, 0xf, true);
                    word |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)word, 0x118 /*row_shr:8*/, 0xf, 0xf, true);
                    if ((lane & 15u) == 15u && base + (lane & ~15u) < len) dst[(base >> 4) + (lane >> 4)] = word;
                }
                bad = __any(bad);
            }
            if (len == 0 || bad) {  // empty: Absent (fmindex.rs:185-207); a byte without a code / too long: the generic kernel's
                if (lane == leader) {
                    if (len == 0) {
                        tag[qs] = (uint8_t)BG_FM_ABSENT;
                        lower[qs] = 0;
                        upper[qs] = 0;
                        matched_len[qs] = 0;
                    } else {
                        tag[qs] = kTagDeferred;
                    }
                }
                if (mine) q += n_quads;  // the same quad takes the next one in the next turn of this loop
                continue;
            }
            if (mine) {
                pos = len;
                l = 0;
                r = fm.n - 1;  // fmindex.rs:148
                matched = 0;
                active = true;
                need = false;
            }
            waiting &= waiting - 1;
        }
    };
    auto emit = [&](uint32_t tg, uint32_t lo, uint32_t hi, uint32_t ml) {
        if (t == 0) {
            tag[q] = (uint8_t)tg;
            lower[q] = lo;
            upper[q] = hi;
            matched_len[q] = ml;
        }
    };
    for (;;) {
        if (__any(need)) fetch_all();
        if (!__any(active)) break;
        if (active) {
            // one iteration of the loop at fmindex.rs:160-182; the symbol is a code already
            pos -= 1;
            const uint32_t a = (slot[pos >> 4] >> (2 * (pos & 15u))) & 3u;
            const uint32_t less_a = s_less4[a];
            // straight-line up to the (rare) second block load: l == 0 ranks position 0 and drops the result
            const uint32_t lm1 = l ? l - 1 : 0u;
            const uint32_t br = r / kSymPerBlock, orr = r - br * kSymPerBlock;
            const uint32_t bl = lm1 / kSymPerBlock, ol = lm1 - bl * kSymPerBlock;
            const uint4 vr = fm.blocks[(uint64_t)br * 4 + t];
            uint4 vl = vr;
            if (bl != br) {
                vl = fm.blocks[(uint64_t)bl * 4 + t];
                if (COUNT) n_lines += 1;
            }
            if (COUNT) n_lines += 1;
            uint32_t occ_r = quad_sum(block_part_bf(vr, t, orr, a));
            uint32_t occ_l = quad_sum(block_part_bf(vl, t, ol, a));
            if (fm.n_exc == 1) {  // (uniform) the one sparse exception — the sentinel — sits in the stream as code 0
                const uint32_t e0 = s_exc[0];
                occ_r -= (a == 0 && e0 <= r) ? 1u : 0u;
                occ_l -= (a == 0 && e0 <= lm1) ? 1u : 0u;
            } else if (a == 0 && fm.n_exc) {
                occ_r -= count_le(s_exc, 0u, fm.n_exc, r);
                occ_l -= count_le(s_exc, 0u, fm.n_exc, lm1);
            }
            occ_l = l ? occ_l : 0u;
            const uint32_t pl = l, pr = r;
            bool stop = occ_r == 0;  // fmindex.rs:167-170
            if (!stop) {
                l = less_a + occ_l;  // fmindex.rs:171
                r = less_a + occ_r - 1;
                if (l > r)  // fmindex.rs:177-180
                    stop = true;
                else
                    matched += 1;
            }
            if (stop) {
                if (matched)
                    emit(BG_FM_PARTIAL, pl, pr + 1, matched);
                else
                    emit(BG_FM_ABSENT, 0, 0, 0);
                need = true;
            } else if (pos == 0) {
                emit(BG_FM_COMPLETE, l, r + 1, matched);
                need = true;
            }
            if (need) {
                q += n_quads;
                active = false;
            }
        }
    }
    if (COUNT && t == 0 && n_lines) atomicAdd(seeds.lines, (unsigned long long)n_lines);
}

// K5x — fm_search_fast2x_kernel: the fast kernel's search on the index's 2-step rank blocks (fm_kernels.h: Fm2Dev;
// f2.blocks2 != null), TWO queries per quad.  The LF loop takes two pattern symbols per block access — half the requests of
// a query against a request-rate limit (round 4) — and single steps (the last symbol of an odd-length pattern, and the two
// symbols of a pair that no row of the interval has in front) from the same blocks.  One code path for both: k symbols, a
// 4-bit code whose low half is masked off for a single step, and ONE end condition — Occ(r) == Occ(l - 1) is "the pair
// does not occur" for a double step and, for a single one, both of the reference's (occ_r == 0 implies it; l > r is it),
// which report the same (pl, pr, matched_len).
// Two queries per quad (round 5): with its requests halved the search waits neither for memory throughput nor for the
// vector unit (0.60 of the 128-byte gather rate at 3 Gbp, VALU 31 % busy, eight wavefronts per SIMD — the most the hardware
// holds): it waits for the latency of one block access per step, and the only parallelism left to add is inside a wavefront.  Every quad walks two independent queries:
// phase A computes the block addresses of both and issues their loads — all of them unconditional and in one basic block,
// so that the second query's requests leave before the first one's data is waited for (the line of l - 1 is requested even
// where it is the line of r: a hit in the vector cache) — phase B ranks and updates both.  Stream (quad, u) takes queries
// (quad * 2 + u) + k * (quads * 2); results, deferral and LDS pattern slots as in fm_search_fast_kernel.
// Measured against one query per quad (profiles/r05_fm_ilp.txt, 10 M x 100 bp): 846 -> 1076 M queries/s on the 100 Mbp index, 608 -> 794 M at 3 Gbp
// (packed patterns 908 -> 1121 and 657 -> 860).  86 VGPRs: five wavefronts per SIMD, ten queries in flight per SIMD-slot
// against eight.  More is not better: three queries per quad (116 VGPRs, four wavefronts: twelve) reach 988 / 752, four
// (147: three wavefronts) 838 / 673, and the same two queries compiled for six wavefronts (80 VGPRs, three values in
// scratch) 1006 / 715 — the optimum is where this kernel sits.
// WIDE (round 6): the same kernel on 64-bit positions (FmLayout<true>: l, r, less, C2 and the exception positions are
// uint64; the blocks' counters are relative to a superblock whose absolute base — sixteen pair codes + four single-step sums —
// is one more load per rank, issued in phase A next to the block's).  The narrow instantiation compiles to the code it was.
template <bool SEEDS, bool COUNT, bool PACKED, bool WIDE>
__global__ __launch_bounds__(256) void fm_search_fast2x_kernel(typename FmLayout<WIDE>::Dev fm, uint64_t n_q, const uint8_t* __restrict__ pat,
                                                               const uint64_t* __restrict__ pat_off, uint8_t* __restrict__ tag,
                                                               uint64_t* __restrict__ lower, uint64_t* __restrict__ upper,
                                                               uint32_t* __restrict__ matched_len, const SeedSrc seeds,
                                                               const typename FmLayout<WIDE>::Dev2 f2) {
    using P = typename FmLayout<WIDE>::Pos;
    constexpr int U = 2;                       // queries per quad
    constexpr uint32_t SLOT = kFastSyms / 16;  // dwords per pattern slot
    __shared__ uint16_t s_class[256];
    __shared__ P s_less4[4];
    __shared__ uint32_t s_pk[64 * U * SLOT + 1];  // (+1: the 2-step funnel reads one dword past a slot's last)
    __shared__ P s_c2[16], s_e2pos[kMaxExc2];
    __shared__ uint32_t s_e2nib[kMaxExc2];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) s_class[i] = fm.sym_class[i];
    if (threadIdx.x < 4) s_less4[threadIdx.x] = fm.less[(seeds.code_bytes >> (8 * threadIdx.x)) & 0xFFu];
    if (threadIdx.x == 0) s_pk[64 * U * SLOT] = 0;
    if (threadIdx.x < 16) s_c2[threadIdx.x] = f2.c2[threadIdx.x];
    if (threadIdx.x < kMaxExc2) {
        s_e2pos[threadIdx.x] = f2.exc_pos[threadIdx.x];
        s_e2nib[threadIdx.x] = f2.exc_nib[threadIdx.x];
    }
    __syncthreads();

    const uint32_t t = threadIdx.x & 3;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n_streams = (uint64_t)gridDim.x * (blockDim.x >> 2) * U;
    struct St {
        uint64_t q;
        P l, r;
        uint32_t pos, matched;
        bool active, need, force1;
    };
    St S[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        S[u].q = ((uint64_t)blockIdx.x * (blockDim.x >> 2) + (threadIdx.x >> 2)) * U + u;
        S[u].pos = S[u].l = S[u].r = S[u].matched = 0;
        S[u].active = false;
        S[u].need = true;
        S[u].force1 = false;
    }
    uint32_t n_lines = 0;

    // taking the next query of stream u: a job of the whole wavefront, one waiting quad at a time (fm_search_fast_kernel)
    auto fetch_all = [&](St& s, const int u) {
        uint64_t waiting = __ballot(s.need && t == 0);
        while (waiting) {
            const uint32_t leader = (uint32_t)__ffsll((unsigned long long)waiting) - 1u;
            const bool mine = (lane >> 2) == (leader >> 2);
            const uint64_t qs = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(s.q >> 32), leader) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)s.q, leader);
            if (qs >= n_q) {
                if (mine) {
                    s.need = false;
                    s.active = false;
                }
                waiting &= waiting - 1;
                continue;
            }
            uint64_t off;
            uint32_t len;
            if (SEEDS) {
                const uint64_t rd = qs / seeds.S;
                const uint32_t k = (uint32_t)(qs - rd * seeds.S);
                const uint64_t o = pat_off[rd];
                off = o + (uint64_t)k * seeds.stride;
                len = (uint64_t)k * seeds.stride + seeds.seed_len <= pat_off[rd + 1] - o ? seeds.seed_len : 0u;
            } else {
                off = pat_off[qs];
                const uint64_t len64 = pat_off[qs + 1] - off;
                len = len64 > kFastSyms ? kFastSyms + 1 : (uint32_t)len64;
            }
            bool bad = len > kFastSyms;
            uint32_t* const dst = s_pk + ((((threadIdx.x >> 6) * 16) + (leader >> 2)) * U + u) * SLOT;
            if (PACKED && len && !bad) {
                const uint32_t* pk = (const uint32_t*)pat;
                if (lane < ((len + 15u) >> 4)) {
                    const uint64_t w0 = (off >> 4) + lane;
                    const uint32_t sh = 2u * ((uint32_t)off & 15u);
                    const uint32_t lo = pk[w0], hi = pk[w0 + 1];  // the stream is padded by one dword
                    dst[lane] = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
                }
            } else if (len && !bad) {
                for (uint32_t base = 0; base < len; base += 64) {
                    const uint32_t idx = base + lane;
                    uint32_t c = 0;
                    if (idx < len) {
                        c = s_class[pat[off + idx]];
                        bad = bad || c >= 4;
                    }
                    uint32_t word = (c & 3u) << (2 * (lane & 15u));
                    word |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)word, 0x111 /*row_shr:1*/, 0xf, 0xf, true);
                    word |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)word, 0x112 /*row_shr:2*/, 0xf, 0xf, true);
                    word |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)word, 0x114 /*row_shr:4*/, 0xf, 0xf, true);
                    word |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)word, 0x118 /*row_shr:8*/, 0xf, 0xf, true);
                    if ((lane & 15u) == 15u && base + (lane & ~15u) < len) dst[(base >> 4) + (lane >> 4)] = word;
                }
                bad = __any(bad);
            }
            if (len == 0 || bad) {  // empty: Absent (fmindex.rs:185-207); a byte without a code / too long: the generic kernel's
                if (lane == leader) {
                    if (len == 0) {
                        tag[qs] = (uint8_t)BG_FM_ABSENT;
                        lower[qs] = 0;
                        upper[qs] = 0;
                        matched_len[qs] = 0;
                    } else {
                        tag[qs] = kTagDeferred;
                    }
                }
                if (mine) s.q += n_streams;  // the same stream takes the next one in the next turn of this loop
                continue;
            }
            if (mine) {
                s.pos = len;
                s.l = 0;
                s.r = fm.n - 1;  // fmindex.rs:148
                s.matched = 0;
                s.active = true;
                s.need = false;
                s.force1 = false;
            }
            waiting &= waiting - 1;
        }
    };
    auto emit = [&](uint64_t q, uint32_t tg, P lo, P hi, uint32_t ml) {
        if (t == 0) {
            tag[q] = (uint8_t)tg;
            lower[q] = lo;
            upper[q] = hi;
            matched_len[q] = ml;
        }
    };
    for (;;) {
        bool any_active = false;
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (__any(S[u].need)) fetch_all(S[u], u);
            any_active |= S[u].active;
        }
        if (!__any(any_active)) break;
        // ---- phase A: the symbols and the block loads of both streams (a stream without a query reads block 0)
        uint4 rc[U], rs[U], lc[U], ls[U];
        uint32_t c[U], p2[U], orr[U], ol[U];
        P lm1[U];
        uint64_t sbr[U], sbl[U];  // WIDE: the superblock's absolute count of this step's code (or single-step sum)
        bool single[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const St& s = S[u];
            single[u] = s.force1 || s.pos == 1;
            p2[u] = s.active ? s.pos - (single[u] ? 1u : 2u) : 0u;
            const uint32_t* const slot = s_pk + ((threadIdx.x >> 2) * U + u) * SLOT;
            const uint32_t ix = p2[u] >> 4;
            // symbols pos-2 (second: low bits) and pos-1 (first) as one nibble; a single step reads its symbol into the high half
            const uint32_t cc = __builtin_amdgcn_alignbit(slot[ix + 1], slot[ix], 2 * (p2[u] & 15u));
            c[u] = single[u] ? (cc & 3u) << 2 : (cc & 15u);
            lm1[u] = s.l ? s.l - 1 : 0u;
            const P r_ = s.active ? s.r : 0u, l_ = s.active ? lm1[u] : 0u;
            const P br = r_ / kSym2PerBlock, bl = l_ / kSym2PerBlock;
            orr[u] = (uint32_t)(r_ % kSym2PerBlock);
            ol[u] = (uint32_t)(l_ % kSym2PerBlock);
            rc[u] = f2.blocks2[(uint64_t)br * 8 + t];
            rs[u] = f2.blocks2[(uint64_t)br * 8 + 4 + t];
            lc[u] = f2.blocks2[(uint64_t)bl * 8 + t];
            ls[u] = f2.blocks2[(uint64_t)bl * 8 + 4 + t];
            if constexpr (WIDE) {
                const uint32_t bi = single[u] ? 16u + (c[u] >> 2) : c[u];
                sbr[u] = f2.sb2[(br >> f2.sb_shift) * 20 + bi];
                sbl[u] = f2.sb2[(bl >> f2.sb_shift) * 20 + bi];
            } else {
                sbr[u] = sbl[u] = 0;
            }
            if (COUNT && s.active) n_lines += bl != br ? 2u : 1u;
        }
        // ---- phase B: fmindex.rs:160-182, twice per block access (or once: `single`)
#pragma unroll
        for (int u = 0; u < U; u++) {
            St& s = S[u];
            if (!s.active) continue;
            const uint32_t k = single[u] ? 1u : 2u;
            const P base = single[u] ? s_less4[c[u] >> 2] : s_c2[c[u]];
            const Pair2Key key2 = pair2_key(c[u], single[u]);
            P occ_r = quad_sum(block2_part(rc[u], rs[u], t, orr[u], c[u], single[u], key2));
            P occ_l = quad_sum(block2_part(lc[u], ls[u], t, ol[u], c[u], single[u], key2));
            if constexpr (WIDE) {
                occ_r += sbr[u];
                occ_l += sbl[u];
            }
            // positions that hold a 0 for a symbol without a code: the first two inline (one sentinel: exactly two; unused
            // entries sit at the largest position, which no rank reaches), more of them (several sentinels) in a loop
            {
                const uint32_t key = single[u] ? 16u : c[u];
                const P e0 = f2.exc_pos[0];
                const uint32_t n0 = single[u] ? (f2.exc_nib[0] & 16u) | (c[u] ? 32u : 0u) : (f2.exc_nib[0] & 15u);
                const P e1 = f2.exc_pos[1];
                const uint32_t n1 = single[u] ? (f2.exc_nib[1] & 16u) | (c[u] ? 32u : 0u) : (f2.exc_nib[1] & 15u);
                occ_r -= (n0 == key && e0 <= s.r) ? 1u : 0u;
                occ_l -= (n0 == key && e0 <= lm1[u]) ? 1u : 0u;
                occ_r -= (n1 == key && e1 <= s.r) ? 1u : 0u;
                occ_l -= (n1 == key && e1 <= lm1[u]) ? 1u : 0u;
                for (uint32_t e = 2; e < f2.n_exc; e++) {  // (uniform)
                    const P pe = s_e2pos[e];
                    const uint32_t ne = s_e2nib[e];
                    const uint32_t nk = single[u] ? (ne & 16u) | (c[u] ? 32u : 0u) : (ne & 15u);
                    occ_r -= (nk == key && pe <= s.r) ? 1u : 0u;
                    occ_l -= (nk == key && pe <= lm1[u]) ? 1u : 0u;
                }
            }
            occ_l = s.l ? occ_l : 0u;
            const bool empty = occ_r == occ_l;
            if (empty && !single[u]) {
                s.force1 = true;  // nothing changes: the two single steps that follow say how the query ends
            } else if (empty) {
                if (s.matched)
                    emit(s.q, BG_FM_PARTIAL, s.l, s.r + 1, s.matched);
                else
                    emit(s.q, BG_FM_ABSENT, 0, 0, 0);
                s.need = true;
            } else {
                s.l = base + occ_l;  // fmindex.rs:171 (twice for a double step)
                s.r = base + occ_r - 1;
                s.pos = p2[u];
                s.matched += k;
                if (s.pos == 0) {
                    emit(s.q, BG_FM_COMPLETE, s.l, s.r + 1, s.matched);
                    s.need = true;
                }
            }
            if (s.need) {
                s.q += n_streams;
                s.active = false;
                s.force1 = false;
            }
        }
    }
    if (COUNT && t == 0 && n_lines) atomicAdd(seeds.lines, (unsigned long long)n_lines);
}

}  // namespace

// (the builders, bg_fm_build and bg_fm_build_dev: fm_build.hip)

extern "C" int bg_fm_free(bg_fm* fm) {
    if (!fm) return BG_OK;
    hipFree(fm->d_blocks);
    hipFree(fm->d_sb);
    hipFree(fm->d_sb2);
    hipFree(fm->d_blocks2);
    hipFree(fm->d_exc_pos);
    hipFree(fm->d_exc_sym_pos);
    hipFree(fm->d_class);
    hipFree(fm->d_less);
    hipFree(fm->d_exc_byte);
    hipFree(fm->d_sparse_off);
    hipFree(fm->d_bitvecs);
    hipFree(fm->d_bwt_raw);
    if (fm->text_owned) hipFree(fm->d_text);
    hipFree(fm->d_sa);
    hipFree(fm->d_extra_row);
    hipFree(fm->d_extra_pos);
    delete fm;
    return BG_OK;
}

extern "C" uint64_t bg_fm_device_bytes(const bg_fm* fm) { return fm ? fm->bytes : 0; }
extern "C" uint64_t bg_fm_step2_bytes(const bg_fm* fm) {
    if (fm && fm->wide) return fm->wdev2.blocks2 && !fm->no_step2 ? (fm->wdev.n + kSym2PerBlock - 1) / kSym2PerBlock * 128 : 0;
    return fm && fm->dev2.blocks2 && !fm->no_step2 ? ((uint64_t)fm->dev.n + kSym2PerBlock - 1) / kSym2PerBlock * 128 : 0;
}

static SeedSrc fm_codes(const bg_fm* fm) {
    SeedSrc ex{};
    ex.code_bytes = fm_code_bytes(fm);
    return ex;
}
// grid of fm_search_fast2x_kernel: persistent blocks, as many as are resident (its registers decide), 128 queries each
template <typename K>
static uint64_t fm_2x_blocks(K kernel, uint64_t n_q) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1) per_cu = 4;
    return std::min<uint64_t>((n_q + 127) / 128, 256ull * (uint64_t)per_cu);
}

// Every backward search, on either layout and in every flavour (SEEDS: the seed windows of src; PACKED: 2-bit patterns,
// offsets in symbols; COUNT: the block loads counted into src.lines, narrow index only).  The fast kernels apply when the
// four 2-bit codes all stand for symbols (no dense symbols), the patterns may fit their LDS slots, no test option says
// otherwise and, on a wide index, the index has 2-step blocks (no single-step fast kernel there).  They answer what their
// slots hold and tag the rest (a byte outside the codes, more than kFastSyms symbols) kTagDeferred for the generic kernel
// launched behind them; otherwise the generic kernel answers every query.
template <bool SEEDS, bool PACKED, bool COUNT>
static int fm_search(bg_fm* fm, uint64_t n_q, const uint8_t* d_pat, const uint64_t* d_pat_off, uint8_t* d_tag, uint64_t* d_lower,
                     uint64_t* d_upper, uint32_t* d_matched_len, const SeedSrc& src, hipStream_t st) {
    const bool step2 = (fm->wide ? fm->wdev2.blocks2 : fm->dev2.blocks2) && !fm->no_step2;
    const bool fast = fm->n_codes == 4 && (fm->wide ? step2 : !fm->dev.n_dense) && !fm->no_fast && (!SEEDS || src.seed_len <= kFastSyms);
    if (fm->wide) {
        if constexpr (COUNT) {
            return BG_ERR_UNSUPPORTED;
        } else {
            if (!fast) return fm_wide_search_launch<SEEDS, PACKED, false>(fm, n_q, d_pat, d_pat_off, d_tag, d_lower, d_upper, d_matched_len, src, st);
            auto kernel = fm_search_fast2x_kernel<SEEDS, false, PACKED, true>;
            kernel<<<dim3((unsigned)fm_2x_blocks(kernel, n_q)), dim3(256), 0, st>>>(fm->wdev, n_q, d_pat, d_pat_off, d_tag, d_lower, d_upper,
                                                                                    d_matched_len, src, fm->wdev2);
            BG_HIP(hipGetLastError());
            return fm_wide_search_launch<SEEDS, PACKED, true>(fm, n_q, d_pat, d_pat_off, d_tag, d_lower, d_upper, d_matched_len, src, st);
        }
    }
    const dim3 grid((unsigned)std::min<uint64_t>((n_q + 63) / 64, 256 * 8));  // 8 resident 256-thread blocks per CU
    if (!fast) {
        fm_backward_search_kernel<SEEDS, PACKED, COUNT, false><<<grid, dim3(256), 0, st>>>(fm->dev, n_q, d_pat, d_pat_off, d_tag, d_lower,
                                                                                        d_upper, d_matched_len, src);
    } else {
        if (step2) {
            auto kernel = fm_search_fast2x_kernel<SEEDS, COUNT, PACKED, false>;
            kernel<<<dim3((unsigned)fm_2x_blocks(kernel, n_q)), dim3(256), 0, st>>>(fm->dev, n_q, d_pat, d_pat_off, d_tag, d_lower, d_upper,
                                                                                    d_matched_len, src, fm->dev2);
        } else {
            fm_search_fast_kernel<SEEDS, COUNT, PACKED><<<grid, dim3(256), 0, st>>>(fm->dev, n_q, d_pat, d_pat_off, d_tag, d_lower, d_upper,
                                                                                   d_matched_len, src);
        }
        fm_backward_search_kernel<SEEDS, PACKED, COUNT, true><<<grid, dim3(256), 0, st>>>(fm->dev, n_q, d_pat, d_pat_off, d_tag, d_lower,
                                                                                       d_upper, d_matched_len, src);
    }
    BG_HIP(hipGetLastError());
    return BG_OK;
}

// `search` under the ctx's timing events: with ctx->timing, its span on `st` counts as one launch in ctx->last.fm_ms
template <typename F>
static int fm_timed(bg_ctx* ctx, hipStream_t st, F&& search) {
    const bool timed = ctx && ctx->timing;
    if (timed) BG_HIP(hipEventRecord(ctx->ev[0], st));
    const int rc = search();
    if (rc || !timed) return rc;
    BG_HIP(hipEventRecord(ctx->ev[1], st));
    BG_HIP(hipEventSynchronize(ctx->ev[1]));
    float ms = 0;
    BG_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    ctx->last.fm_ms += ms;
    ctx->last.fm_launches += 1;
    return BG_OK;
}

extern "C" int bg_fm_set_option(bg_fm* fm, const char* key, int64_t value) {
    if (!fm || !key) return BG_ERR_INVALID_ARG;
    if (!strcmp(key, "no_step2")) {  // searches take single steps only, whether the index has 2-step blocks or not (tests, A/B)
        fm->no_step2 = value != 0;
        return BG_OK;
    }
    if (!strcmp(key, "no_fast")) {  // tests: every search through the generic kernel
        fm->no_fast = value != 0;
        return BG_OK;
    }
    return BG_ERR_INVALID_ARG;
}

extern "C" int bg_fm_backward_search_batch_dev(bg_fm* fm, uint64_t n_q, const uint8_t* d_pat,
                                               const uint64_t* d_pat_off, uint8_t* d_tag,
                                               uint64_t* d_lower, uint64_t* d_upper,
                                               uint32_t* d_matched_len, void* stream) {
    if (!fm || (n_q && (!d_pat_off || !d_tag || !d_lower || !d_upper || !d_matched_len)))
        return BG_ERR_INVALID_ARG;
    if (n_q == 0) return BG_OK;
    hipStream_t st = (hipStream_t)stream;
    return fm_timed(fm->ctx, st, [&] {
        return fm_search<false, false, false>(fm, n_q, d_pat, d_pat_off, d_tag, d_lower, d_upper, d_matched_len, fm_codes(fm), st);
    });
}

// the seed windows of a batch of reads as patterns (see SeedSrc): n_reads * S queries, results indexed [read * S + seed]
// (timed: the seed search inside bg_seed_extend_batch_dev, kernel_ms.seed_search of bench.py)
int bg_fm_search_seeds_dev(bg_fm* fm, uint64_t n_reads, const uint8_t* d_reads, const uint64_t* d_read_off, uint32_t S,
                           uint32_t stride, uint32_t seed_len, uint8_t* d_tag, uint64_t* d_lower, uint64_t* d_upper,
                           uint32_t* d_matched_len, hipStream_t st) {
    const uint64_t n_q = n_reads * S;
    if (n_q == 0) return BG_OK;
    SeedSrc src = fm_codes(fm);
    src.S = S, src.stride = stride, src.seed_len = seed_len;
    return fm_timed(fm->ctx, st, [&] {
        return fm_search<true, false, false>(fm, n_q, d_reads, d_read_off, d_tag, d_lower, d_upper, d_matched_len, src, st);
    });
}

// ---- 2-bit packed patterns (north_star: "coalesced HBM loads of packed 2-bit reads") -------------------------------
extern "C" int bg_fm_pattern_codes(const bg_fm* fm, uint8_t codes[4]) {
    if (!fm || !codes) return BG_ERR_INVALID_ARG;
    // the four 2-bit codes must all stand for symbols of the text (a DNA-like BWT): with dense symbols code 0 means
    // "something else", and an index over fewer than four letters has codes no pattern symbol may use
    if ((!fm->wide && fm->dev.n_dense) || fm->n_codes != 4) return BG_ERR_UNSUPPORTED;
    for (int c = 0; c < 4; c++) codes[c] = fm->code_byte[c];
    return BG_OK;
}

extern "C" int bg_fm_backward_search_packed_dev(bg_fm* fm, uint64_t n_q, const uint32_t* d_packed, const uint64_t* d_sym_off,
                                                uint8_t* d_tag, uint64_t* d_lower, uint64_t* d_upper, uint32_t* d_matched_len,
                                                void* stream) {
    if (!fm || (n_q && (!d_packed || !d_sym_off || !d_tag || !d_lower || !d_upper || !d_matched_len))) return BG_ERR_INVALID_ARG;
    if ((!fm->wide && fm->dev.n_dense) || fm->n_codes != 4) return BG_ERR_UNSUPPORTED;
    if (n_q == 0) return BG_OK;
    hipStream_t st = (hipStream_t)stream;
    return fm_timed(fm->ctx, st, [&] {
        return fm_search<false, true, false>(fm, n_q, (const uint8_t*)d_packed, d_sym_off, d_tag, d_lower, d_upper, d_matched_len, fm_codes(fm), st);
    });
}

// measurement aid: the same search with its 64-byte block loads counted (synchronous; *lines_out on the host)
extern "C" int bg_fm_backward_search_count_lines_dev(bg_fm* fm, uint64_t n_q, const uint8_t* d_pat, const uint64_t* d_pat_off,
                                                     uint8_t* d_tag, uint64_t* d_lower, uint64_t* d_upper,
                                                     uint32_t* d_matched_len, uint64_t* lines_out, void* stream) {
    if (!fm || !lines_out || (n_q && (!d_pat_off || !d_tag || !d_lower || !d_upper || !d_matched_len))) return BG_ERR_INVALID_ARG;
    *lines_out = 0;
    if (fm->wide) return BG_ERR_UNSUPPORTED;  // (a measurement aid of the 32-bit kernels)
    if (n_q == 0) return BG_OK;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(fm->ctx->device));
    unsigned long long* d_cnt = nullptr;
    BG_HIP(hipMalloc((void**)&d_cnt, 8));
    auto run = [&]() -> int {
        BG_HIP(hipMemsetAsync(d_cnt, 0, 8, st));
        SeedSrc ex = fm_codes(fm);
        ex.lines = d_cnt;
        const int rc = fm_search<false, false, true>(fm, n_q, d_pat, d_pat_off, d_tag, d_lower, d_upper, d_matched_len, ex, st);
        if (rc) return rc;
        BG_HIP(hipMemcpyAsync(lines_out, d_cnt, 8, hipMemcpyDeviceToHost, st));
        BG_HIP(hipStreamSynchronize(st));
        return BG_OK;
    };
    const int rc = run();
    hipFree(d_cnt);
    return rc;
}

// ---- bg_fm_backward_search_batch: host buffers in and out -----------------------------------------------------------
// Round 2 made six hipMallocs and pageable copies per call (150 M queries/s against 460 M device-resident).  Now the
// batch flows in stages of kFmStage queries through three staging sets that persist in the ctx: host threads copy a
// stage's pattern bytes into pinned memory and rebase its offsets, the copy-in stream uploads them, the ctx stream
// searches, the copy-out stream downloads the four result arrays into pinned memory, and a second host thread copies
// them into the caller's arrays while the following stages are in flight — no allocation in a warmed-up call.
struct bg_fm_pipe {
    static constexpr int NSET = 3;
    struct Set {
        uint8_t *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr;
        size_t in_cap = 0, out_cap = 0;
        hipEvent_t in_done = nullptr, k_done = nullptr, out_done = nullptr;
    } set[NSET];
    hipStream_t s_in = nullptr, s_out = nullptr;
};
void bg_fm_pipe_free(bg_fm_pipe* p) {
    if (!p) return;
    for (auto& s : p->set) {
        if (s.h_in) hipHostFree(s.h_in);
        if (s.h_out) hipHostFree(s.h_out);
        hipFree(s.d_in);
        hipFree(s.d_out);
        for (hipEvent_t e : {s.in_done, s.k_done, s.out_done})
            if (e) hipEventDestroy(e);
    }
    if (p->s_in) hipStreamDestroy(p->s_in);
    if (p->s_out) hipStreamDestroy(p->s_out);
    delete p;
}
namespace {
template <typename F>
void fm_parallel_for(uint64_t n, uint64_t grain, F&& f) {
    const unsigned nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(bg_host_threads(), n / std::max<uint64_t>(grain, 1) + 1));
    if (nt == 1) {
        f((uint64_t)0, n);
        return;
    }
    bg_pool_run(nt, [&](unsigned t) { f(n * t / nt, n * (t + 1) / nt); });
}
constexpr uint64_t kFmStage = 1u << 20;  // queries per stage
}  // namespace

extern "C" int bg_fm_backward_search_batch(bg_fm* fm, uint64_t n_q, const uint8_t* pat,
                                           const uint64_t* pat_off, uint8_t* tag, uint64_t* lower,
                                           uint64_t* upper, uint32_t* matched_len) {
    if (!fm || (n_q && (!pat_off || !tag || !lower || !upper || !matched_len)))
        return BG_ERR_INVALID_ARG;
    if (n_q == 0) return BG_OK;
    bg_ctx* ctx = fm->ctx;
    BG_HIP(hipSetDevice(ctx->device));
    if (pat_off[n_q] && !pat) return BG_ERR_INVALID_ARG;
    if (!ctx->fm_pipe) {
        ctx->fm_pipe = new bg_fm_pipe();
        BG_HIP(hipStreamCreateWithFlags(&ctx->fm_pipe->s_in, hipStreamNonBlocking));
        BG_HIP(hipStreamCreateWithFlags(&ctx->fm_pipe->s_out, hipStreamNonBlocking));
        for (auto& s : ctx->fm_pipe->set)
            for (hipEvent_t* e : {&s.in_done, &s.k_done, &s.out_done}) BG_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    bg_fm_pipe& P = *ctx->fm_pipe;
    const uint64_t chunk = std::min<uint64_t>(kFmStage, n_q);
    const uint64_t nch = (n_q + chunk - 1) / chunk;
    uint64_t max_pb = 0;
    for (uint64_t c = 0; c < nch; c++) {
        const uint64_t q0 = c * chunk, q1 = std::min(n_q, q0 + chunk);
        if (pat_off[q1] < pat_off[q0]) return BG_ERR_INVALID_ARG;
        max_pb = std::max(max_pb, pat_off[q1] - pat_off[q0]);
    }
    // staging layout: in = pattern bytes | offsets ; out = lower | upper | matched_len | tag
    const uint64_t o_off = (max_pb + 8 + 255) & ~255ull;  // (+8: the packed flavour's dword past the last symbol)
    const size_t in_need = o_off + (chunk + 1) * 8 + 256;
    const uint64_t o_hi = chunk * 8, o_ml = 2 * chunk * 8, o_tag = o_ml + chunk * 4;
    const size_t out_need = o_tag + chunk + 256;
    for (auto& s : P.set) {
        if (s.in_cap < in_need) {
            if (s.h_in) hipHostFree(s.h_in);
            hipFree(s.d_in);
            s.h_in = s.d_in = nullptr;
            s.in_cap = 0;
            BG_HIP(hipHostMalloc((void**)&s.h_in, in_need, hipHostMallocDefault));
            BG_HIP(hipMalloc((void**)&s.d_in, in_need));
            s.in_cap = in_need;
        }
        if (s.out_cap < out_need) {
            if (s.h_out) hipHostFree(s.h_out);
            hipFree(s.d_out);
            s.h_out = s.d_out = nullptr;
            s.out_cap = 0;
            BG_HIP(hipHostMalloc((void**)&s.h_out, out_need, hipHostMallocDefault));
            BG_HIP(hipMalloc((void**)&s.d_out, out_need));
            s.out_cap = out_need;
        }
    }
    hipStream_t s_k = ctx->stream;
    std::atomic<bool> any_panic{false};
    // The patterns travel as 2-bit codes where the index takes them (bg_fm_pattern_codes) — packed by the worker threads
    // into the pinned stage instead of copied there: a quarter of the bytes to write and to send over the link, and the
    // packed kernel on the other side.  A stage with a byte outside the four codes is staged as bytes after all.
    uint8_t pcodes[4] = {0, 0, 0, 0};
    const bool can_pack = !ctx->fm_host_bytes && bg_fm_pattern_codes(fm, pcodes) == BG_OK;
    uint64_t n_packed_stages = 0;
    // BG_TRACE_HOST=1: where the host side of the stages spends its time (ms, summed over the call)
    const bool trace = getenv("BG_TRACE_HOST") != nullptr;
    double t_pack = 0, t_launch = 0, t_wait_set = 0, t_d_wait = 0, t_d_copy = 0;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    auto drain = [&](uint64_t c) -> int {
        bg_fm_pipe::Set& S = P.set[c % bg_fm_pipe::NSET];
        double t0 = now();
        BG_HIP(hipEventSynchronize(S.out_done));
        t_d_wait += now() - t0;
        t0 = now();
        const uint64_t q0 = c * chunk, nq = std::min(n_q, q0 + chunk) - q0;
        fm_parallel_for(nq, 1 << 16, [&](uint64_t a, uint64_t b) {
            memcpy(lower + q0 + a, S.h_out + a * 8, (b - a) * 8);
            memcpy(upper + q0 + a, S.h_out + o_hi + a * 8, (b - a) * 8);
            memcpy(matched_len + q0 + a, S.h_out + o_ml + a * 4, (b - a) * 4);
            memcpy(tag + q0 + a, S.h_out + o_tag + a, b - a);
            bool pn = false;
            for (uint64_t q = a; q < b; q++) pn = pn || S.h_out[o_tag + q] == BG_FM_PANIC;
            if (pn) any_panic = true;
        });
        t_d_copy += now() - t0;
        return BG_OK;
    };
    std::mutex mu;
    std::condition_variable cv;
    uint64_t submitted = 0, drained = 0;
    bool abort_drain = false;
    int drain_rc = BG_OK;
    std::string drain_err;
    const int device = ctx->device;
    std::thread drainer([&] {
        if (hipSetDevice(device) != hipSuccess) {
            std::lock_guard<std::mutex> lk(mu);
            drain_rc = BG_ERR_HIP;
            drained = nch;
            cv.notify_all();
            return;
        }
        for (uint64_t c = 0; c < nch; c++) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return submitted > c || abort_drain; });
                if (submitted <= c) break;
            }
            const int r = drain(c);
            std::lock_guard<std::mutex> lk(mu);
            if (r && drain_rc == BG_OK) {
                drain_rc = r;
                drain_err = bg_tls_error;
            }
            drained = c + 1;
            cv.notify_all();
        }
        std::lock_guard<std::mutex> lk(mu);
        drained = nch;
        cv.notify_all();
    });
    auto stop_drainer = [&] {
        {
            std::lock_guard<std::mutex> lk(mu);
            abort_drain = true;
        }
        cv.notify_all();
        drainer.join();
    };
    for (uint64_t c = 0; c < nch; c++) {
        double t0 = now();
        if (c >= bg_fm_pipe::NSET) {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return drained >= c - bg_fm_pipe::NSET + 1; });
        }
        t_wait_set += now() - t0;
        t0 = now();
        bg_fm_pipe::Set& S = P.set[c % bg_fm_pipe::NSET];
        const uint64_t q0 = c * chunk, nq = std::min(n_q, q0 + chunk) - q0;
        const uint64_t b0 = pat_off[q0], pb = pat_off[q0 + nq] - b0;
        bool packed = can_pack && pb != 0;
        if (packed) {
            std::atomic<bool> all_codes{true};
            // (ranges start at multiples of 64 symbols: whole dwords per thread)
            fm_parallel_for((pb + 63) / 64, 1 << 14, [&](uint64_t a, uint64_t b) {
                const uint64_t s0 = a * 64, s1 = std::min(pb, b * 64);
                if (!bgpack::pack2_host(pat + b0 + s0, s1 - s0, pcodes, (uint32_t*)S.h_in + s0 / 16)) all_codes = false;
            });
            packed = all_codes;
        }
        if (!packed) fm_parallel_for(pb, 1 << 20, [&](uint64_t a, uint64_t b) { memcpy(S.h_in + a, pat + b0 + a, b - a); });
        n_packed_stages += packed ? 1 : 0;
        const uint64_t in_bytes = packed ? ((pb + 15) / 16 + 1) * 4 : pb;
        uint64_t* hoff = (uint64_t*)(S.h_in + o_off);
        fm_parallel_for(nq + 1, 1 << 16, [&](uint64_t a, uint64_t b) {
            for (uint64_t q = a; q < b; q++) hoff[q] = pat_off[q0 + q] - b0;
        });
        t_pack += now() - t0;
        t0 = now();
        bool ok = true;
        if (pb) ok = ok && bg_copy_pieces(S.d_in, S.h_in, in_bytes, hipMemcpyHostToDevice, P.s_in) == hipSuccess;
        ok = ok && hipMemcpyAsync(S.d_in + o_off, S.h_in + o_off, (nq + 1) * 8, hipMemcpyHostToDevice, P.s_in) == hipSuccess;
        ok = ok && hipEventRecord(S.in_done, P.s_in) == hipSuccess && hipStreamWaitEvent(s_k, S.in_done, 0) == hipSuccess;
        int rc = !ok ? BG_ERR_HIP
                 : packed
                     ? bg_fm_backward_search_packed_dev(fm, nq, (const uint32_t*)S.d_in, (const uint64_t*)(S.d_in + o_off), S.d_out + o_tag,
                                                        (uint64_t*)S.d_out, (uint64_t*)(S.d_out + o_hi), (uint32_t*)(S.d_out + o_ml), s_k)
                     : bg_fm_backward_search_batch_dev(fm, nq, S.d_in, (const uint64_t*)(S.d_in + o_off), S.d_out + o_tag,
                                                       (uint64_t*)S.d_out, (uint64_t*)(S.d_out + o_hi), (uint32_t*)(S.d_out + o_ml), s_k);
        if (rc == BG_OK && (hipEventRecord(S.k_done, s_k) != hipSuccess || hipStreamWaitEvent(P.s_out, S.k_done, 0) != hipSuccess ||
                            bg_copy_pieces(S.h_out, S.d_out, o_tag + nq, hipMemcpyDeviceToHost, P.s_out) != hipSuccess ||
                            hipEventRecord(S.out_done, P.s_out) != hipSuccess))
            rc = BG_ERR_HIP;
        if (rc) {
            hipDeviceSynchronize();
            stop_drainer();
            return rc;
        }
        t_launch += now() - t0;
        {
            std::lock_guard<std::mutex> lk(mu);
            submitted = c + 1;
        }
        cv.notify_all();
    }
    const double t0j = now();
    drainer.join();
    if (trace)
        fprintf(stderr, "[bg fm host] %llu stages (%llu as 2-bit codes): pack %.2f launch %.2f wait-for-set %.2f join %.2f | drainer: wait %.2f copy %.2f ms\n",
                (unsigned long long)nch, (unsigned long long)n_packed_stages, t_pack, t_launch, t_wait_set, now() - t0j, t_d_wait, t_d_copy);
    if (drain_rc) {
        bg_tls_error = drain_err;
        return drain_rc;
    }
    return any_panic ? BG_ERR_OUT_OF_ALPHABET : BG_OK;
}
