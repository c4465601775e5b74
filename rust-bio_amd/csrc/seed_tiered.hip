// The tiered seed-and-extend call (bg_seed_extend_tiered_batch[_dev]): fixed windows searched once on an FMD index over T$R$
// for every read (tier 1), SMEMs for the reads whose tier-1 winner scores below reseed_below (tier 2).  Definition:
// include/biogpu.h.  The stages of a pass that are the call's own (se_candidates and se_reseed of seed_extend.hip run them):
//   S1 K5<SEEDS>   the nr x S window slots of the caller's reads (not of their revcomps: the index holds both strands)
//   S1" records    one thread per slot: (tag, lower, upper) -> the six-uint64 record K7 writes for an SMEM, the read's own
//                  number of windows; S2', S3, S4' and S5-S7 then run as in the SMEM call with M = S
//   T1 select      one thread per read: score < reseed_below -> flag and byte count (scanned: compact index, byte offset)
//      (the count and the bytes of the re-seeded reads are the pass's extra host round trip; count 0 ends the pass)
//   T2 gather      one wavefront per read: the flagged reads' bytes and offsets back to back, compact index -> read of the pass
//   tier 2         the SMEM call's pass on the compact reads, into scratch hits / strand / operation slots
//   T3 merge       one wavefront per re-seeded read: the better of the two tier winners (seed_tier_rule.h), the counts of both
//                  tiers, the tier byte; a winning tier-2 hit and its operations move into the caller's slot
#include "seed_pass.h"
#include "seed_tier_rule.h"

namespace {

using namespace bgseed;

// S1": slot q = (read r, window k).  The record is {lower, lower_rev (not known from a one-sided search: 0), size, match_size,
// position on the read, length}; a window that is not Complete, or that the read does not have, is a record of size 0.
__global__ __launch_bounds__(256) void se_window_records_kernel(uint64_t n_q, uint32_t S, uint32_t stride, uint32_t seed_len,
                                                                const uint64_t* __restrict__ read_off, const uint8_t* __restrict__ tag,
                                                                const uint64_t* __restrict__ lower, const uint64_t* __restrict__ upper,
                                                                uint32_t* __restrict__ count, uint64_t* __restrict__ rec,
                                                                uint32_t* __restrict__ flags) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    const uint64_t r = q / S;
    const uint32_t k = (uint32_t)(q - r * S);
    const uint64_t L = read_off[r + 1] - read_off[r];
    const uint32_t n_win = L >= seed_len ? (uint32_t)min((L - seed_len) / stride + 1, (uint64_t)S) : 0u;
    if (k == 0) count[r] = n_win;
    uint64_t lo = 0, size = 0;
    if (k < n_win) {
        const uint8_t tg = tag[q];
        if (tg == BG_FM_PANIC) atomicOr(flags, kFlagPanic);  // the window reached a byte outside the alphabet: it does not vote
        if (tg == BG_FM_COMPLETE) {
            lo = lower[q];
            size = upper[q] - lo;
        }
    }
    ulonglong2* out = (ulonglong2*)(rec + q * 6);  // 48 bytes per slot: 16-byte aligned
    out[0] = make_ulonglong2(lo, 0);
    out[1] = make_ulonglong2(size, seed_len);
    out[2] = make_ulonglong2((uint64_t)k * stride, seed_len);
}

// T1: read r of the pass is re-seeded when its tier-1 winner scores below `below` (a read without candidates: BG_MIN_SCORE)
__global__ __launch_bounds__(256) void se_reseed_select_kernel(uint64_t nr, uint64_t r0, const bg_seed_hit_t* __restrict__ hits,
                                                               const uint64_t* __restrict__ read_off, int32_t below,
                                                               uint32_t* __restrict__ flag, uint32_t* __restrict__ n_bytes,
                                                               uint8_t* __restrict__ tier) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nr) return;
    const bool again = hits[r0 + r].aln.score < below;
    flag[r] = again ? 1u : 0u;
    n_bytes[r] = again ? (uint32_t)(read_off[r0 + r + 1] - read_off[r0 + r]) : 0u;
    if (tier) tier[r0 + r] = BG_TIER_NONE;
}

// T2: one wavefront per read of the pass, four per block.  idx / boff: the scans of T1's flags and byte counts (nr + 1 each).
__global__ __launch_bounds__(256) void se_reseed_gather_kernel(uint64_t nr, uint64_t r0, const uint8_t* __restrict__ reads,
                                                               const uint64_t* __restrict__ read_off, const uint32_t* __restrict__ flag,
                                                               const uint64_t* __restrict__ idx, const uint64_t* __restrict__ boff,
                                                               uint8_t* __restrict__ out, uint64_t* __restrict__ out_off,
                                                               uint32_t* __restrict__ map) {
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (r >= nr) return;
    if (r + 1 == nr && lane == 0) out_off[idx[nr]] = boff[nr];  // the closing offset
    if (!flag[r]) return;
    const uint64_t j = idx[r], b = boff[r], ro = read_off[r0 + r], L = read_off[r0 + r + 1] - ro;
    if (lane == 0) {
        map[j] = (uint32_t)r;
        out_off[j] = b;
    }
    for (uint64_t i = lane; i < L; i += 64) out[b + i] = reads[ro + i];
}

// n bytes from src to dst by the 64 lanes of a wavefront: 16 bytes per lane where the two share their alignment
__device__ __forceinline__ void copy_wave(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n, uint32_t lane) {
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) != 0) {
        for (uint32_t i = lane; i < n; i += 64) dst[i] = src[i];
        return;
    }
    const uint32_t head = min(n, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15));
    const uint32_t n_vec = (n - head) / 16;
    if (lane < head) dst[lane] = src[lane];
    const uint4* s16 = (const uint4*)(src + head);
    uint4* d16 = (uint4*)(dst + head);
    for (uint32_t i = lane; i < n_vec; i += 64) d16[i] = s16[i];
    for (uint32_t i = head + 16 * n_vec + lane; i < n; i += 64) dst[i] = src[i];
}

// T3: one wavefront per re-seeded read, four per block.  Compact read j is caller read r = r0 + map[j]: its tier-1 answer is in
// the caller's slot r (strand1: the caller's strand array or the call's scratch, indexed by caller read), its tier-2 answer in
// slot j of hits2 / strand2 / ops2, laid out with the same ops_stride.
__global__ __launch_bounds__(256) void se_reseed_merge_kernel(uint64_t n2, uint64_t r0, const uint32_t* __restrict__ map, SeedOut O,
                                                              uint8_t* __restrict__ strand1, const bg_seed_hit_t* __restrict__ hits2,
                                                              const uint8_t* __restrict__ strand2, const uint8_t* __restrict__ ops2,
                                                              uint8_t* __restrict__ tier) {
    const uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (j >= n2) return;
    const uint64_t r = r0 + map[j];
    const bg_seed_hit_t h1 = O.hits[r], h2 = hits2[j];
    const uint8_t s1 = strand1[r], s2 = strand2[j];
    const bool second = bgtier::tier2_wins(bgtier::TierHit{h1.aln.score, s1, h1.window_start}, bgtier::TierHit{h2.aln.score, s2, h2.window_start});
    bg_seed_hit_t h = second ? h2 : h1;
    h.n_candidates = h1.n_candidates + h2.n_candidates;
    h.n_seed_hits = h1.n_seed_hits + h2.n_seed_hits;
    if (second) {
        h.aln.ops_off = (r + 1) * O.ops_stride - h.aln.n_ops;
        if (O.ops && ops2) copy_wave(O.ops + h.aln.ops_off, ops2 + h2.aln.ops_off, h.aln.n_ops, lane);
    }
    if (lane == 0) {
        O.hits[r] = h;
        strand1[r] = second ? s2 : s1;
        if (tier) tier[r] = second ? BG_TIER_SECOND : BG_TIER_FIRST;
    }
}

}  // namespace

int bg_seed_tiered_records_launch(uint64_t nr, uint32_t S, uint32_t stride, uint32_t seed_len, const uint64_t* d_read_off,
                                  const uint8_t* d_tag, const uint64_t* d_lower, const uint64_t* d_upper, uint32_t* d_count,
                                  uint64_t* d_rec, uint32_t* d_flags, hipStream_t st) {
    const uint64_t n_q = nr * S;
    if (!n_q) return BG_OK;
    se_window_records_kernel<<<dim3((unsigned)((n_q + 255) / 256)), dim3(256), 0, st>>>(n_q, S, stride, seed_len, d_read_off, d_tag, d_lower,
                                                                                        d_upper, d_count, d_rec, d_flags);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

int bg_seed_tiered_select_launch(uint64_t nr, uint64_t r0, const bg_seed_hit_t* d_hits, const uint64_t* d_read_off, int32_t reseed_below,
                                 uint32_t* d_flag, uint32_t* d_bytes, uint8_t* d_tier, hipStream_t st) {
    se_reseed_select_kernel<<<dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, st>>>(nr, r0, d_hits, d_read_off, reseed_below, d_flag,
                                                                                      d_bytes, d_tier);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

int bg_seed_tiered_gather_launch(uint64_t nr, uint64_t r0, const uint8_t* d_reads, const uint64_t* d_read_off, const uint32_t* d_flag,
                                 const uint64_t* d_idx, const uint64_t* d_boff, uint8_t* d_out, uint64_t* d_out_off, uint32_t* d_map,
                                 hipStream_t st) {
    se_reseed_gather_kernel<<<dim3((unsigned)((nr + 3) / 4)), dim3(256), 0, st>>>(nr, r0, d_reads, d_read_off, d_flag, d_idx, d_boff, d_out,
                                                                                  d_out_off, d_map);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

int bg_seed_tiered_merge_launch(uint64_t n2, uint64_t r0, const uint32_t* d_map, const bgseed::SeedOut& O, uint8_t* d_strand1,
                                const bg_seed_hit_t* d_hits2, const uint8_t* d_strand2, const uint8_t* d_ops2, uint8_t* d_tier,
                                hipStream_t st) {
    se_reseed_merge_kernel<<<dim3((unsigned)((n2 + 3) / 4)), dim3(256), 0, st>>>(n2, r0, d_map, O, d_strand1, d_hits2, d_strand2, d_ops2,
                                                                                 d_tier);
    BG_HIP(hipGetLastError());
    return BG_OK;
}
