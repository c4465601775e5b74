// bg_fastq_qual_cut[_dev], bg_fastq_qual_select[_dev] and bg_fastq_qc_tables[_dev]: the kernels that read the quality
// column of a parse, a trim, a filter or a split (include/biogpu.h has the three rules; rust-bio has none of them).  The
// per-read and per-lane bodies, and the serial statement they are tested against, are in fastq_qual_rule.h.
//
// Cut and select, 1 launch each: a read's bytes are contiguous, so a group of 16 lanes takes a read and loads 16
// neighbouring bytes a step; a block's 16 groups stride over the batch.
//   RUNSUM is an inclusive scan of the step's terms over the group, a minimum (the first lane at which the carried sum goes
//   negative) and a maximum (the largest prefix in front of it, the first among equals), then the carried state moves on.  A
//   read whose end is good stops in its first step, so the usual cost is one step per end, not the read's length.
//   WINDOW is the same scan over q[j + W] - q[j]: the window sum at every start of the step, a minimum for the first failing
//   one, and a walk back of 16 symbols a step.
//   Select sums a lane's share of the symbols and reduces (sum, weight sum, low count, minimum) by shuffles; the weight table
//   travels by value into LDS; the pair rule is one shuffle with the neighbouring group, which no lane leaves before.
// The lanes of a group write the 16 words of a cut record and the 8 of a statistics record.  Totals are summed per lane,
// per wavefront and then by one 64-bit atomic add each: sums of integers, the same on every run.
//
// The tables, 1 memset and 1 launch: a privatised histogram.  A block keeps uint32 counters in LDS for the first
// min(max_cycles, 160) rows of base and qhist (160 * 69 * 4 = 44 160 bytes) and for len_hist, meanq_hist and n_reads (4 364
// bytes), strides over the selected reads with 16 lanes a read and 512 threads a block, and at the end adds every non-zero counter to the table by
// one 64-bit atomic.  Rows from 160 on and the row that collects positions at or beyond max_cycles are added to directly.
// Overflow: every counter kept in LDS grows by at most 1 per read (a read has one symbol per position below max_cycles,
// one length and one mean), and the grid is chosen so that a block takes fewer than 2^32 reads; the collecting row, which
// a long read hits many times, is never kept in LDS.  Ordinary vector atomics only.
//
// The host flavours make their device copies through a bg_stage.
#include "fastq_cols.h"
#include "fastq_qual_rule.h"

namespace {

constexpr uint32_t kGroupsPerBlock = 256 / QL_G;
constexpr uint32_t kMaxBlocks = 8192;

// ---- the group's shuffles ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t grp_scan(int32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t o = 1; o < QL_G; o <<= 1) {
        const int32_t u = __shfl_up(v, o, QL_G);
        if (lane >= o) v += u;
    }
    return v;
}
__device__ __forceinline__ uint32_t grp_min(uint32_t v) {
#pragma unroll
    for (uint32_t o = QL_G / 2; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, QL_G));
    return v;
}
__device__ __forceinline__ uint32_t grp_max(uint32_t v) {
#pragma unroll
    for (uint32_t o = QL_G / 2; o; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, QL_G));
    return v;
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, uint32_t o, uint32_t width) {
    return (uint64_t)__shfl_xor((unsigned long long)v, o, width);
}
__device__ __forceinline__ uint64_t grp_sum64(uint64_t v) {
#pragma unroll
    for (uint32_t o = QL_G / 2; o; o >>= 1) v += shfl_xor64(v, o, QL_G);
    return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (uint32_t o = 32; o; o >>= 1) v += shfl_xor64(v, o, 64);
    return v;
}
__device__ __forceinline__ void add64(uint64_t* p, uint64_t v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

// ---- cut ----------------------------------------------------------------------------------------------------------------
// symbols RUNSUM cuts from one end; the loops are uniform over the group
__device__ uint32_t cut_runsum(const uint8_t* q, uint32_t L, uint32_t phred_offset, uint32_t cutoff_in, bool from_end, uint32_t lane) {
    const int32_t cutoff = ql_run_cutoff(cutoff_in);
    ql_run st = ql_run_start();
    for (uint64_t t0 = 0; t0 < L && !st.stopped; t0 += QL_G) {
        const int32_t p = grp_scan(ql_run_term(q, L, phred_offset, cutoff, from_end, t0, lane), lane);
        const uint32_t first_neg = grp_min(ql_run_neg(st, p, L, t0, lane, QL_G));
        const uint32_t key = grp_max(ql_run_key(p, L, t0, lane, first_neg));
        ql_run_carry(st, t0, first_neg, key, __shfl(p, QL_G - 1, QL_G), QL_G);
    }
    return (uint32_t)st.cnt;
}
__device__ uint32_t cut_window(const uint8_t* q, uint32_t L, uint32_t phred_offset, uint32_t cutoff, uint32_t window, uint32_t lane) {
    if (L == 0) return 0;
    const uint32_t W = window < L ? window : L;
    const uint64_t threshold = (uint64_t)cutoff * W;
    uint64_t D = grp_sum64(ql_win_share(q, W, phred_offset, lane, QL_G));
    uint64_t e = L;
    bool found = false;
    for (uint64_t j0 = 0; j0 + W <= L; j0 += QL_G) {
        const int32_t d = ql_win_term(q, L, W, phred_offset, j0, lane);
        const int32_t incl = grp_scan(d, lane);
        const uint32_t f = grp_min(ql_win_fails(D, incl - d, threshold, L, W, j0, lane, QL_G));
        if (f < QL_G) {
            e = j0 + f;
            found = true;
            break;
        }
        D = (uint64_t)((int64_t)D + __shfl(incl, QL_G - 1, QL_G));
    }
    while (found) {
        const uint32_t f = grp_min(ql_back_stops(q, e, phred_offset, cutoff, lane, QL_G));
        e -= f < QL_G ? f : QL_G;
        if (f < QL_G) break;
    }
    return (uint32_t)e;
}

// totals: null, or two zeroed words — reads cut, symbols removed
__global__ __launch_bounds__(256) void ql_cut_kernel(uint64_t n, uint64_t iters, const bg_qual_cut_t prm, const uint8_t* __restrict__ qual,
                                                     const uint64_t* __restrict__ qual_off, bg_alignment_t* __restrict__ cut_out,
                                                     uint64_t* __restrict__ totals) {
    const uint32_t lane = threadIdx.x % QL_G;
    const uint64_t stride = (uint64_t)gridDim.x * kGroupsPerBlock;
    uint64_t n_cut = 0, n_sym = 0;
    for (uint64_t it = 0; it < iters; it++) {
        const uint64_t r = it * stride + ((uint64_t)blockIdx.x * 256 + threadIdx.x) / QL_G;
        if (r >= n) continue;  // the whole group
        const uint64_t q0 = qual_off[r];
        const uint32_t L = (uint32_t)(qual_off[r + 1] - q0);
        const uint8_t* q = qual + q0;
        uint32_t b = 0, e = L;
        if (prm.method_5p == BG_QCUT_RUNSUM) b = cut_runsum(q, L, prm.phred_offset, prm.cutoff_5p, false, lane);
        if (prm.method_3p == BG_QCUT_RUNSUM) e = L - cut_runsum(q, L, prm.phred_offset, prm.cutoff_3p, true, lane);
        if (prm.method_3p == BG_QCUT_WINDOW) e = cut_window(q, L, prm.phred_offset, prm.cutoff_3p, prm.window, lane);
        if (e < b) e = b;
        ((uint32_t*)(cut_out + r))[lane] = ql_cut_word(L, b, e, lane);
        if (lane == 0 && L - (e - b) != 0) {
            n_cut++;
            n_sym += L - (e - b);
        }
    }
    if (!totals) return;
    n_cut = wave_sum64(n_cut);
    n_sym = wave_sum64(n_sym);
    if ((threadIdx.x & 63) == 0 && n_cut) {
        add64(totals, n_cut);
        add64(totals + 1, n_sym);
    }
}

int cut_check(const bg_ctx* ctx, uint64_t n, const bg_qual_cut_t* p, const void* qual, const void* qual_off, const void* cut_out) {
    if (!p) return bg_refuse("bg_fastq_qual_cut: null params");
    if (p->method_5p == BG_QCUT_WINDOW) return bg_refuse("bg_fastq_qual_cut: WINDOW as method_5p");
    if (p->method_5p != BG_QCUT_NONE && p->method_5p != BG_QCUT_RUNSUM) return bg_refuse("bg_fastq_qual_cut: unknown method");
    if (p->method_3p != BG_QCUT_NONE && p->method_3p != BG_QCUT_RUNSUM && p->method_3p != BG_QCUT_WINDOW)
        return bg_refuse("bg_fastq_qual_cut: unknown method");
    if (p->method_3p == BG_QCUT_WINDOW && p->window == 0) return bg_refuse("bg_fastq_qual_cut: window 0 with WINDOW");
    if (p->phred_offset > 255) return bg_refuse("bg_fastq_qual_cut: phred_offset above 255");
    if (!qual_off) return bg_refuse("bg_fastq_qual_cut: null qual_off");
    if (n && (!qual || !cut_out)) return bg_refuse("bg_fastq_qual_cut: null qual or cut_out");
    if (!ctx) return bg_refuse("bg_fastq_qual_cut: null ctx");
    return BG_OK;
}

// ---- select -------------------------------------------------------------------------------------------------------------
struct ql_weights {
    uint32_t w[256];
};

// With BG_QSEL_PAIRED n is even, and so are the groups of a block and of a stride: a read's mate is in the same wavefront
// and in range exactly when the read is.  totals: null, or one zeroed word — records passed.
__global__ __launch_bounds__(256) void ql_select_kernel(uint64_t n, uint64_t iters, const bg_qual_select_t prm, const bool has_weight,
                                                        const ql_weights weight, const uint8_t* __restrict__ qual,
                                                        const uint64_t* __restrict__ qual_off, bg_qual_stats_t* __restrict__ stats_out,
                                                        uint32_t* __restrict__ bin_out, uint64_t* __restrict__ totals) {
    __shared__ uint32_t s_w[256];
    if (has_weight) s_w[threadIdx.x] = weight.w[threadIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x % QL_G;
    const uint64_t stride = (uint64_t)gridDim.x * kGroupsPerBlock;
    uint64_t n_pass = 0;
    for (uint64_t it = 0; it < iters; it++) {
        const uint64_t r = it * stride + ((uint64_t)blockIdx.x * 256 + threadIdx.x) / QL_G;
        const bool live = r < n;
        const uint64_t q0 = live ? qual_off[r] : 0;
        const uint32_t L = live ? (uint32_t)(qual_off[r + 1] - q0) : 0;
        bg_qual_stats_t s = ql_stats_share(qual + q0, L, prm.phred_offset, prm.low_q, has_weight ? s_w : nullptr, lane, QL_G);
#pragma unroll
        for (uint32_t o = QL_G / 2; o; o >>= 1) {
            const bg_qual_stats_t t = {shfl_xor64(s.sum_q, o, QL_G), shfl_xor64(s.weight_sum, o, QL_G), 0, (uint32_t)__shfl_xor((int)s.n_low, o, QL_G),
                                       (uint32_t)__shfl_xor((int)s.min_q, o, QL_G), 0};
            s = ql_stats_merge(s, t);
        }
        s = ql_stats_close(s, L);
        const bool own = ql_passes(prm, s, has_weight);
        const bool mate = __shfl_xor((int)own, QL_G, 64) != 0;
        if (!live) continue;
        const bool keep = ql_keeps(prm.flags, own, mate);
        if (stats_out && lane < 8) ((uint32_t*)(stats_out + r))[lane] = ql_stats_word(s, lane);
        if (lane == 0) {
            if (bin_out) bin_out[r] = keep ? 0u : 1u;
            n_pass += keep;
        }
    }
    if (!totals) return;
    n_pass = wave_sum64(n_pass);
    if ((threadIdx.x & 63) == 0 && n_pass) add64(totals, n_pass);
}

int select_check(const bg_ctx* ctx, uint64_t n, const bg_qual_select_t* p, const void* qual, const void* qual_off, const void* stats_out,
                 const void* bin_out) {
    if (!p) return bg_refuse("bg_fastq_qual_select: null params");
    if (p->flags & ~(uint32_t)(BG_QSEL_PAIRED | BG_QSEL_PAIR_BOTH)) return bg_refuse("bg_fastq_qual_select: unknown flag bits");
    if ((p->flags & BG_QSEL_PAIR_BOTH) && !(p->flags & BG_QSEL_PAIRED)) return bg_refuse("bg_fastq_qual_select: PAIR_BOTH without PAIRED");
    if ((p->flags & BG_QSEL_PAIRED) && (n & 1)) return bg_refuse("bg_fastq_qual_select: PAIRED with an odd record count");
    if (p->phred_offset > 255) return bg_refuse("bg_fastq_qual_select: phred_offset above 255");
    if (p->_reserved != 0) return bg_refuse("bg_fastq_qual_select: non-zero _reserved");
    if (!qual_off) return bg_refuse("bg_fastq_qual_select: null qual_off");
    if (n && !qual) return bg_refuse("bg_fastq_qual_select: null qual");
    if (n && !stats_out && !bin_out) return bg_refuse("bg_fastq_qual_select: both outputs null");
    if (!ctx) return bg_refuse("bg_fastq_qual_select: null ctx");
    return BG_OK;
}

// ---- tables -------------------------------------------------------------------------------------------------------------
constexpr uint32_t kRowsLds = 160;
constexpr uint32_t kTabThreads = 512;  // 32 reads at a time share a block's counters
constexpr uint32_t kTabBlocksPerCu = 3;  // ... and three blocks' counters a compute unit's 160 KB of LDS
constexpr uint32_t kUnroll = 5;  // 80 symbols of a read a step: two steps for 150

__global__ __launch_bounds__(kTabThreads) void ql_tables_kernel(uint64_t m, uint64_t iters, uint64_t first, uint64_t step, uint32_t phred_offset,
                                                        uint32_t max_cycles, const uint8_t* __restrict__ seq,
                                                        const uint64_t* __restrict__ seq_off, const uint8_t* __restrict__ qual,
                                                        const uint64_t* __restrict__ qual_off, uint64_t* __restrict__ tables) {
    __shared__ uint32_t s_cnt[kRowsLds * 69];          // per row: base[5], qhist[64]
    __shared__ uint32_t s_len[BG_QC_MAX_CYCLES + 2];
    __shared__ uint32_t s_mq[64];
    __shared__ uint32_t s_reads;
    const uint32_t kept = max_cycles < kRowsLds ? max_cycles : kRowsLds;  // rows in LDS: never the collecting row max_cycles
    for (uint32_t c = threadIdx.x; c < kept * 69; c += kTabThreads) s_cnt[c] = 0;
    for (uint32_t c = threadIdx.x; c < max_cycles + 2; c += kTabThreads) s_len[c] = 0;
    if (threadIdx.x < 64) s_mq[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_reads = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x % QL_G;
    const uint64_t stride = (uint64_t)gridDim.x * (kTabThreads / QL_G);
    const uint64_t g_qhist = ql_tab_qhist(max_cycles);
    for (uint64_t it = 0; it < iters; it++) {
        const uint64_t k = it * stride + ((uint64_t)blockIdx.x * kTabThreads + threadIdx.x) / QL_G;
        if (k >= m) continue;  // the whole group
        const uint64_t r = first + k * step;
        const uint64_t s0 = seq_off[r], q0 = qual_off[r];
        const uint32_t sl = (uint32_t)(seq_off[r + 1] - s0), ql = (uint32_t)(qual_off[r + 1] - q0);
        // kUnroll loads in flight per lane and column: the counting that follows a load does not wait for the next one
        for (uint64_t i0 = lane; i0 < sl; i0 += kUnroll * QL_G) {
            uint8_t b[kUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; u++) b[u] = i0 + u * QL_G < sl ? seq[s0 + i0 + u * QL_G] : 0;
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; u++) {
                const uint64_t i = i0 + u * QL_G;
                if (i >= sl) break;
                const uint32_t row = ql_row(i, max_cycles), c = ql_base_class(b[u]);
                if (row < kept)
                    atomicAdd(&s_cnt[row * 69 + c], 1u);
                else
                    add64(tables + (uint64_t)row * 5 + c, 1);
            }
        }
        uint64_t sum = 0;
        for (uint64_t i0 = lane; i0 < ql; i0 += kUnroll * QL_G) {
            uint8_t b[kUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; u++) b[u] = i0 + u * QL_G < ql ? qual[q0 + i0 + u * QL_G] : 0;
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; u++) {
                const uint64_t i = i0 + u * QL_G;
                if (i >= ql) break;
                const uint32_t row = ql_row(i, max_cycles), v = ql_q(b[u], phred_offset), c = v < 63 ? v : 63u;
                sum += v;
                if (row < kept)
                    atomicAdd(&s_cnt[row * 69 + 5 + c], 1u);
                else
                    add64(tables + g_qhist + (uint64_t)row * 64 + c, 1);
            }
        }
        sum = grp_sum64(sum);
        if (lane == 0) {
            atomicAdd(&s_len[sl <= max_cycles ? sl : max_cycles + 1], 1u);
            if (ql) {
                const uint64_t mean = sum / ql;
                atomicAdd(&s_mq[mean < 63 ? mean : 63], 1u);
            }
            atomicAdd(&s_reads, 1u);
        }
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < kept * 69; c += kTabThreads) {
        const uint32_t v = s_cnt[c], row = c / 69, col = c % 69;
        if (v) add64(tables + (col < 5 ? (uint64_t)row * 5 + col : g_qhist + (uint64_t)row * 64 + (col - 5)), v);
    }
    for (uint32_t c = threadIdx.x; c < max_cycles + 2; c += kTabThreads)
        if (s_len[c]) add64(tables + ql_tab_len(max_cycles) + c, s_len[c]);
    if (threadIdx.x < 64 && s_mq[threadIdx.x]) add64(tables + ql_tab_meanq(max_cycles) + threadIdx.x, s_mq[threadIdx.x]);
    if (threadIdx.x == 0 && s_reads) add64(tables + ql_tab_reads(max_cycles), s_reads);
}

int tables_check(const bg_ctx* ctx, uint64_t n, uint64_t first, uint64_t step, uint32_t phred_offset, uint32_t max_cycles, const void* seq,
                 const void* seq_off, const void* qual, const void* qual_off, const void* tables) {
    if (step == 0) return bg_refuse("bg_fastq_qc_tables: step 0");
    if (max_cycles == 0 || max_cycles > BG_QC_MAX_CYCLES) return bg_refuse("bg_fastq_qc_tables: max_cycles outside 1 .. BG_QC_MAX_CYCLES");
    if (phred_offset > 255) return bg_refuse("bg_fastq_qc_tables: phred_offset above 255");
    if (!tables) return bg_refuse("bg_fastq_qc_tables: null tables");
    if (!seq_off || !qual_off) return bg_refuse("bg_fastq_qc_tables: null offsets");
    if (fq_strided_count(n, first, step) && (!seq || !qual)) return bg_refuse("bg_fastq_qc_tables: null seq or qual");
    if (!ctx) return bg_refuse("bg_fastq_qc_tables: null ctx");
    return BG_OK;
}

// blocks and rounds of a kernel that gives 16 lanes to each of `items` reads
void shape(uint64_t items, uint32_t max_blocks, uint32_t* blocks, uint64_t* iters, uint32_t per_block = kGroupsPerBlock) {
    const uint64_t need = (items + per_block - 1) / per_block;
    *blocks = (uint32_t)std::min<uint64_t>(need, max_blocks);
    *iters = (need + *blocks - 1) / *blocks;
}

}  // namespace

extern "C" uint64_t bg_qc_tables_words(uint32_t max_cycles) { return ql_tab_words(max_cycles); }

extern "C" int bg_fastq_qual_cut_dev(bg_ctx* ctx, uint64_t n, const bg_qual_cut_t* params, const uint8_t* d_qual, const uint64_t* d_qual_off,
                                     bg_alignment_t* d_cut_out, uint64_t* totals, void* stream) {
    if (int rc = cut_check(ctx, n, params, d_qual, d_qual_off, d_cut_out)) return rc;
    if (totals) totals[0] = totals[1] = 0;
    if (n == 0) return BG_OK;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);
    uint64_t* d_tot = nullptr;
    if (totals) {  // aux: the two sums
        if (int rc = bg_reserve(&ctx->aux, &ctx->aux_bytes, 16)) return rc;
        d_tot = (uint64_t*)ctx->aux;
        BG_HIP(hipMemsetAsync(d_tot, 0, 16, st));
    }
    uint32_t blocks;
    uint64_t iters;
    shape(n, kMaxBlocks, &blocks, &iters);
    ql_cut_kernel<<<dim3(blocks), dim3(256), 0, st>>>(n, iters, *params, d_qual, d_qual_off, d_cut_out, d_tot);
    BG_HIP(hipGetLastError());
    if (totals) {
        BG_HIP(hipMemcpyAsync(totals, d_tot, 16, hipMemcpyDeviceToHost, st));
        BG_HIP(hipStreamSynchronize(st));
    }
    return BG_OK;
}

extern "C" int bg_fastq_qual_cut(bg_ctx* ctx, uint64_t n, const bg_qual_cut_t* params, const uint8_t* qual, const uint64_t* qual_off,
                                 bg_alignment_t* cut_out, uint64_t* totals) {
    if (int rc = cut_check(ctx, n, params, qual, qual_off, cut_out)) return rc;
    if (totals) totals[0] = totals[1] = 0;
    if (n == 0) return BG_OK;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_qual = s.up(qual, qual_off[n]);
    const uint64_t* d_qo = s.up(qual_off, (size_t)n + 1);
    bg_alignment_t* d_cut = s.out<bg_alignment_t>(n);
    if (s.sync()) return s.rc;
    if (int rc = bg_fastq_qual_cut_dev(ctx, n, params, d_qual, d_qo, d_cut, totals, s.st)) return rc;
    s.down(cut_out, d_cut, n);
    return s.sync();
}

extern "C" int bg_fastq_qual_select_dev(bg_ctx* ctx, uint64_t n, const bg_qual_select_t* params, const uint32_t* weight, const uint8_t* d_qual,
                                        const uint64_t* d_qual_off, bg_qual_stats_t* d_stats_out, uint32_t* d_bin_out, uint64_t* totals,
                                        void* stream) {
    if (int rc = select_check(ctx, n, params, d_qual, d_qual_off, d_stats_out, d_bin_out)) return rc;
    if (totals) totals[0] = 0;
    if (n == 0) return BG_OK;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);
    uint64_t* d_tot = nullptr;
    if (totals) {  // aux: the sum
        if (int rc = bg_reserve(&ctx->aux, &ctx->aux_bytes, 8)) return rc;
        d_tot = (uint64_t*)ctx->aux;
        BG_HIP(hipMemsetAsync(d_tot, 0, 8, st));
    }
    ql_weights w;
    if (weight)
        std::copy(weight, weight + 256, w.w);
    else
        std::fill(w.w, w.w + 256, 0u);
    uint32_t blocks;
    uint64_t iters;
    shape(n, kMaxBlocks, &blocks, &iters);
    ql_select_kernel<<<dim3(blocks), dim3(256), 0, st>>>(n, iters, *params, weight != nullptr, w, d_qual, d_qual_off, d_stats_out, d_bin_out,
                                                         d_tot);
    BG_HIP(hipGetLastError());
    if (totals) {
        BG_HIP(hipMemcpyAsync(totals, d_tot, 8, hipMemcpyDeviceToHost, st));
        BG_HIP(hipStreamSynchronize(st));
    }
    return BG_OK;
}

extern "C" int bg_fastq_qual_select(bg_ctx* ctx, uint64_t n, const bg_qual_select_t* params, const uint32_t* weight, const uint8_t* qual,
                                    const uint64_t* qual_off, bg_qual_stats_t* stats_out, uint32_t* bin_out, uint64_t* totals) {
    if (int rc = select_check(ctx, n, params, qual, qual_off, stats_out, bin_out)) return rc;
    if (totals) totals[0] = 0;
    if (n == 0) return BG_OK;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_qual = s.up(qual, qual_off[n]);
    const uint64_t* d_qo = s.up(qual_off, (size_t)n + 1);
    bg_qual_stats_t* d_stats = stats_out ? s.out<bg_qual_stats_t>(n) : nullptr;
    uint32_t* d_bin = bin_out ? s.out<uint32_t>(n) : nullptr;
    if (s.sync()) return s.rc;
    if (int rc = bg_fastq_qual_select_dev(ctx, n, params, weight, d_qual, d_qo, d_stats, d_bin, totals, s.st)) return rc;
    if (stats_out) s.down(stats_out, d_stats, n);
    if (bin_out) s.down(bin_out, d_bin, n);
    return s.sync();
}

extern "C" int bg_fastq_qc_tables_dev(bg_ctx* ctx, uint64_t n, uint64_t first, uint64_t step, uint32_t phred_offset, uint32_t max_cycles,
                                      const uint8_t* d_seq, const uint64_t* d_seq_off, const uint8_t* d_qual, const uint64_t* d_qual_off,
                                      uint64_t* d_tables, void* stream) {
    if (int rc = tables_check(ctx, n, first, step, phred_offset, max_cycles, d_seq, d_seq_off, d_qual, d_qual_off, d_tables)) return rc;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    BG_HIP(hipMemsetAsync(d_tables, 0, ql_tab_words(max_cycles) * 8, st));
    const uint64_t m = fq_strided_count(n, first, step);
    if (m == 0) return BG_OK;
    uint32_t blocks;
    uint64_t iters;
    // as many blocks as the device holds at once, so that none waits for a second turn with half the device idle — and
    // never 2^31 reads or more to one of them (see the head of the file)
    int cus = 0;
    BG_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    shape(m, (uint32_t)std::max<uint64_t>((uint64_t)kTabBlocksPerCu * (cus > 0 ? cus : 1), m >> 31), &blocks, &iters, kTabThreads / QL_G);
    ql_tables_kernel<<<dim3(blocks), dim3(kTabThreads), 0, st>>>(m, iters, first, step, phred_offset, max_cycles, d_seq, d_seq_off, d_qual, d_qual_off,
                                                         d_tables);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

extern "C" int bg_fastq_qc_tables(bg_ctx* ctx, uint64_t n, uint64_t first, uint64_t step, uint32_t phred_offset, uint32_t max_cycles,
                                  const uint8_t* seq, const uint64_t* seq_off, const uint8_t* qual, const uint64_t* qual_off, uint64_t* tables) {
    if (int rc = tables_check(ctx, n, first, step, phred_offset, max_cycles, seq, seq_off, qual, qual_off, tables)) return rc;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_seq = s.up(seq, n ? seq_off[n] : 0);
    const uint64_t* d_so = s.up(seq_off, (size_t)n + 1);
    const uint8_t* d_qual = s.up(qual, n ? qual_off[n] : 0);
    const uint64_t* d_qo = s.up(qual_off, (size_t)n + 1);
    uint64_t* d_tab = s.out<uint64_t>(ql_tab_words(max_cycles));
    if (s.sync()) return s.rc;
    if (int rc = bg_fastq_qc_tables_dev(ctx, n, first, step, phred_offset, max_cycles, d_seq, d_so, d_qual, d_qo, d_tab, s.st)) return rc;
    s.down(tables, d_tab, ql_tab_words(max_cycles));
    return s.sync();
}
