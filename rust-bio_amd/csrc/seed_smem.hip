// Seed-and-extend seeded with the SMEMs of an FMD index (bg_seed_extend_smem_batch[_dev]): stages S1', S2' and S4' of a pass,
// in the place of S1, S2 and S4 of seed_extend.hip (se_candidates branches on SeedCall::smem; S0, S3 and S5-S7 are shared).
//
// The index is over T$R$ (T the forward text of n_t symbols, R its reverse complement), so one FMDIndex::all_smems walk of
// the caller's read (K7, fmd_smems.hip) seeds both strands: a suffix-array row of an SMEM's interval that lies in the T half
// places the read on the forward strand, one in the R half places revcomp(read).  Definition: include/biogpu.h.
//   S1' K7 (all = 1, uint64 records), one walk per caller read, M = max_smems record slots per read   -> count, rec
//   S2' votes      one thread per (read, slot): BiInterval.size if the slot holds a record and 1 <= size <= max_occ, the
//                  interval's first row                                                                -> votes, lower
//   S4' propose    one wavefront per caller read: (strand, s) of every hit as one key with the strand in its top bit, one
//                  sort, merge within a strand -> the read's kept starts, the forward strand's first, and the counts of its
//                  virtual reads
#include "seed_pass.h"

namespace {

using namespace bgseed;

constexpr uint32_t kSmemPanic = 0xFFFFFFFFu;  // K7's count of a read the reference panics on

__global__ __launch_bounds__(256) void se_smem_lengths_kernel(uint64_t nr, const uint64_t* __restrict__ read_off, uint32_t max_read_len,
                                                              uint32_t* __restrict__ flags) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nr && read_off[r + 1] - read_off[r] > max_read_len) atomicOr(flags, kFlagLongRead);
}

// S2': votes and first row of every record slot
__global__ __launch_bounds__(256) void se_smem_votes_kernel(uint64_t n_q, SeedSmemPrm prm, const uint32_t* __restrict__ count,
                                                            const uint64_t* __restrict__ rec, uint32_t* __restrict__ votes,
                                                            uint64_t* __restrict__ lower, uint32_t* __restrict__ flags) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    const uint64_t r = q / prm.M;
    const uint32_t t = (uint32_t)(q - r * prm.M);
    const uint32_t cnt = count[r];
    uint32_t c = 0;
    uint64_t lo = 0;
    if (cnt == kSmemPanic) {  // the reference panics on this read: none of its records votes
        if (t == 0) atomicOr(flags, kFlagPanic);
    } else {
        if (cnt > prm.M && t == 0) atomicOr(flags, kFlagTruncated);  // only the first M records vote
        if (t < cnt) {
            const uint64_t size = rec[q * 6 + 2];
            if (size >= 1 && size <= prm.max_occ) {
                c = (uint32_t)size;
                lo = rec[q * 6];  // BiInterval::forward() = [lower, lower + size)
            }
        }
    }
    votes[q] = c;
    lower[q] = lo;
}

// S4': one wavefront per caller read.  Its hits are pos[hoff[r * M] .. hoff[(r + 1) * M)), grouped by record slot (at most
// kMaxCand: M * max_occ).  Hit p of the record at read position a with length len:
//   forward half   p + len <= n_t:                       s = p - a                 (dropped if p < a)
//   reverse half   p >= n_t + 1, p + len <= 2 n_t + 1:   s = n_t + a - (p - n_t - 1) - L of revcomp(read) (dropped if negative)
//   anything else (a hit across a sentinel, BG_SA_NONE / BG_SA_PANIC), s >= n_t and a strand that does not run: dropped.
// The key is s with the strand in the top bit of T (n_t < 2^31 on 32-bit positions; the bit is free on 64-bit ones as well), so
// one sort orders both strands' lists; equal keys merge, then starts within pad / 2 of the last one kept on the same strand.
template <typename T>
__global__ __launch_bounds__(64) void se_smem_propose_kernel(SeedSmemPrm prm, uint64_t nr, const uint64_t* __restrict__ read_off,
                                                             const uint64_t* __restrict__ hoff, const uint64_t* __restrict__ rec,
                                                             uint64_t* __restrict__ pos, uint64_t* __restrict__ soff,
                                                             uint32_t* __restrict__ n_cand, uint32_t* __restrict__ n_hits,
                                                             uint32_t* __restrict__ x_bytes, uint32_t* __restrict__ y_bytes) {
    constexpr T kNoStart = ~(T)0;
    constexpr T kRev = (T)1 << (8 * sizeof(T) - 1);
    __shared__ T s_val[kMaxCand];
    __shared__ uint32_t s_off[kMaxCand + 1];  // the slots' hit offsets, relative to the read's first
    __shared__ uint32_t s_kept[2];
    const uint64_t r = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    if (r >= nr) return;
    const uint32_t M = prm.M;
    const uint64_t n_t = prm.n_t;
    const uint32_t L = (uint32_t)(read_off[r + 1] - read_off[r]);
    const uint64_t h0 = hoff[r * M];
    for (uint32_t k = lane; k <= M; k += 64) s_off[k] = (uint32_t)(hoff[r * M + k] - h0);  // M <= kMaxCand (checked by the host)
    __syncthreads();
    const uint32_t nh = min(s_off[M], kMaxCand);
    uint32_t kept_f = 0, kept_r = 0, hits_f = 0, hits_r = 0;
    if (nh) {
        uint32_t P = 64;
        while (P < nh) P <<= 1;
        auto proposal = [&](uint32_t i) -> T {
            T v = kNoStart;
            if (i < nh) {
                // the slot of hit i: the last k with s_off[k] <= i whose interval is not empty, found by bisection (s_off[M] > i)
                uint32_t lo = 0, hi = M - 1;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s_off[mid + 1] > i)
                        hi = mid;
                    else
                        lo = mid + 1;
                }
                const uint64_t* rc = rec + (r * M + lo) * 6;
                const uint64_t a = rc[4], len = rc[5];
                const uint64_t p = pos[h0 + i];
                if (p < 2 * n_t + 2) {  // (BG_SA_NONE / BG_SA_PANIC are not)
                    if (p + len <= n_t) {
                        hits_f += (prm.strands & BG_STRAND_FORWARD) ? 1u : 0u;
                        if ((prm.strands & BG_STRAND_FORWARD) && p >= a && p - a < n_t) v = (T)(p - a);
                    } else if (p >= n_t + 1 && p + len <= 2 * n_t + 1) {
                        const uint64_t q = p - n_t - 1;
                        hits_r += (prm.strands & BG_STRAND_REVERSE) ? 1u : 0u;
                        if ((prm.strands & BG_STRAND_REVERSE) && q + L <= n_t + a && n_t + a - q - L < n_t) v = kRev | (T)(n_t + a - q - L);
                    }
                }
            }
            return v;
        };
        if (nh <= 64) {
            // the usual read (a handful of hits): every lane finds its key's rank among the wavefront's by looking at each of
            // the nh keys once (a broadcast per key) — no LDS passes, no barriers
            const T v = proposal(lane);
            uint32_t rank = 0;
            for (uint32_t j = 0; j < nh; j++) {
                T u;
                if constexpr (sizeof(T) == 8)
                    u = (T)((uint64_t)(uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), (int)j) << 32 | (uint32_t)__shfl((int)(uint32_t)v, (int)j));
                else
                    u = (T)(uint32_t)__shfl((int)(uint32_t)v, (int)j);
                rank += (u < v || (u == v && j < lane)) ? 1u : 0u;
            }
            // (lanes >= nh hold kNoStart, the largest key: their ranks are nh .. 63 in lane order)
            s_val[lane < nh ? rank : lane] = v;
            __syncthreads();
        } else {
            for (uint32_t i = lane; i < P; i += 64) s_val[i] = proposal(i);
            __syncthreads();
            // bitonic sort of P keys by the 64 lanes
            for (uint32_t k2 = 2; k2 <= P; k2 <<= 1) {
                for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
                    for (uint32_t i = lane; i < P; i += 64) {
                        const uint32_t ixj = i ^ j;
                        if (ixj > i) {
                            const T a = s_val[i], b = s_val[ixj];
                            const bool up = (i & k2) == 0;
                            if ((a > b) == up) {
                                s_val[i] = b;
                                s_val[ixj] = a;
                            }
                        }
                    }
                    __syncthreads();
                }
            }
        }
        // merge equal keys (compacted in place: a key never moves up, and a step reads before it writes) ...
        uint32_t base = 0;
        for (uint32_t b0 = 0; b0 < P; b0 += 64) {
            const uint32_t i = b0 + lane;
            const T v = s_val[i];
            const bool keep = v != kNoStart && (i == 0 || s_val[i - 1] != v);
            const uint64_t m = __ballot(keep);
            __syncthreads();
            if (keep) s_val[base + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = v;
            base += (uint32_t)__popcll(m);
        }
        __syncthreads();
        // ... and starts within pad / 2 of the last one kept, in order, never across the strand boundary; the kept starts go back
        // over the read's own slots of `pos`, the forward strand's first
        if (lane == 0) {
            const T merge = (T)(prm.pad / 2);
            uint32_t kept = 0, fwd = 0;
            T last = 0;
            bool last_rev = false;
            for (uint32_t i = 0; i < base; i++) {
                const bool rev = (s_val[i] & kRev) != 0;
                const T s = s_val[i] & (T)~kRev;
                if (kept == 0 || rev != last_rev || s - last > merge) {
                    pos[h0 + kept++] = s;
                    last = s;
                    last_rev = rev;
                    fwd += rev ? 0u : 1u;
                }
            }
            s_kept[0] = fwd;
            s_kept[1] = kept - fwd;
        }
        __syncthreads();
        kept_f = s_kept[0];
        kept_r = s_kept[1];
    }
    // window bytes of each strand's candidates (second pass: the starts are final now), and the hits of each half
    uint32_t y_f = 0, y_r = 0;
    for (uint32_t c = lane; c < kept_f + kept_r; c += 64) {
        const uint64_t v = pos[h0 + c];
        const uint64_t lo = v > prm.pad ? v - prm.pad : 0u;
        const uint64_t hi = min(n_t, v + L + prm.pad);
        if (c < kept_f)
            y_f += (uint32_t)(hi - lo);
        else
            y_r += (uint32_t)(hi - lo);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        y_f += (uint32_t)__shfl_xor((int)y_f, o);
        y_r += (uint32_t)__shfl_xor((int)y_r, o);
        hits_f += (uint32_t)__shfl_xor((int)hits_f, o);
        hits_r += (uint32_t)__shfl_xor((int)hits_r, o);
    }
    if (lane == 0) {
        auto put = [&](uint64_t v, uint64_t first, uint32_t nc, uint32_t hits, uint32_t yb) {
            soff[v] = first;
            n_cand[v] = nc;
            n_hits[v] = hits;
            x_bytes[v] = nc * L;
            y_bytes[v] = yb;
        };
        if (prm.strands == BG_STRAND_BOTH) {
            put(2 * r, h0, kept_f, hits_f, y_f);
            put(2 * r + 1, h0 + kept_f, kept_r, hits_r, y_r);
        } else if (prm.strands == BG_STRAND_REVERSE) {
            put(r, h0, kept_r, hits_r, y_r);  // (no forward proposal was made: the reverse starts are the read's first)
        } else {
            put(r, h0, kept_f, hits_f, y_f);
        }
    }
}

}  // namespace

int bg_seed_smem_lengths_launch(uint64_t nr, const uint64_t* d_read_off, uint32_t max_read_len, uint32_t* d_flags, hipStream_t st) {
    se_smem_lengths_kernel<<<dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, st>>>(nr, d_read_off, max_read_len, d_flags);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

int bg_seed_smem_seeds_launch(bg_fm* fm, const SeedSmemPrm& prm, uint32_t min_seed_len, uint64_t nr, const uint8_t* d_reads,
                              const uint64_t* d_read_off, uint32_t max_read_len, uint32_t* d_count, uint64_t* d_rec, uint32_t* d_votes,
                              uint64_t* d_lower, uint32_t* d_flags, hipStream_t st) {
    // K7's device entry point reports neither a truncated read nor a panic in its status: both stay in the counts, and S2' turns
    // them into flag bits, so every read of the pass is answered
    if (int rc = bg_fmd_smems_batch64_dev(fm, 1, nr, d_reads, d_read_off, nullptr, min_seed_len, max_read_len, prm.M, d_count, d_rec, st)) return rc;
    return bg_seed_smem_votes_launch(nr * prm.M, prm, d_count, d_rec, d_votes, d_lower, d_flags, st);
}

int bg_seed_smem_votes_launch(uint64_t n_q, const SeedSmemPrm& prm, const uint32_t* d_count, const uint64_t* d_rec, uint32_t* d_votes,
                              uint64_t* d_lower, uint32_t* d_flags, hipStream_t st) {
    if (!n_q) return BG_OK;
    se_smem_votes_kernel<<<dim3((unsigned)((n_q + 255) / 256)), dim3(256), 0, st>>>(n_q, prm, d_count, d_rec, d_votes, d_lower, d_flags);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

int bg_seed_smem_propose_launch(bool wide, const SeedSmemPrm& prm, uint64_t nr, const uint64_t* d_read_off, const uint64_t* d_hoff,
                                const uint64_t* d_rec, uint64_t* d_pos, uint64_t* d_soff, uint32_t* d_n_cand, uint32_t* d_n_hits,
                                uint32_t* d_x_bytes, uint32_t* d_y_bytes, hipStream_t st) {
    const dim3 grid((unsigned)nr), block(64);
    if (wide)
        se_smem_propose_kernel<uint64_t><<<grid, block, 0, st>>>(prm, nr, d_read_off, d_hoff, d_rec, d_pos, d_soff, d_n_cand, d_n_hits, d_x_bytes, d_y_bytes);
    else
        se_smem_propose_kernel<uint32_t><<<grid, block, 0, st>>>(prm, nr, d_read_off, d_hoff, d_rec, d_pos, d_soff, d_n_cand, d_n_hits, d_x_bytes, d_y_bytes);
    BG_HIP(hipGetLastError());
    return BG_OK;
}
