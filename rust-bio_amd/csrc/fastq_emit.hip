// bg_fastq_filter[_dev] and bg_fastq_emit[_dev]: the way out of the FASTQ front of the pipeline (include/biogpu.h has both
// rules; rust-bio has fastq::Writer, io/fastq.rs:528-599, and no filter).  The per-record bodies are in fastq_emit_rule.h.
//
// Filter, 11 launches: the pass kernel (one lane per record, or 16 lanes per record where the 'N' bytes are counted; the pair
// rule is one shuffle with the neighbouring group, mates being neighbours) leaves keep[r] and three uint32 columns — 1, the
// sequence and the quality bytes of a kept record, 0 of a dropped one; three shared scans (scan.hip) turn them into the
// record's rank and its two byte offsets; the copy kernel (16 lanes per record, the trim's copy) moves the kept records.
//
// Emit: a length kernel (one lane per line), the scan, one read-back of the total, then the text pass: 16 lanes per line copy
// the four runs byte by byte to the line's place.  The measured default is this plain copy; fq_emit_mode = 2 (bg_set_option)
// selects the other flavour that was measured, sam_emit.hip's write pass: the group gathers the line into LDS at the offset
// inside a 16-byte granule that it has in the output and stores it with 16-byte stores between a byte head and a byte tail
// (a line longer than the staging area goes straight to global memory).  DESIGN.md 4.8 has the measurements.
#include <algorithm>

#include "bg_common.h"
#include "fastq_emit_rule.h"

namespace {

// ---- filter -------------------------------------------------------------------------------------------------------------
struct FqfArgs {
    uint64_t n;
    bg_fastq_filter_t f;
    const bg_alignment_t* hits;
    uint32_t n_pat;
    const bg_fastq_record_t* recs;
    const uint8_t* seq;
    const uint64_t* seq_off;
    const uint64_t* qual_off;
};

// G lanes per record: 1 where the sequence is not read, 16 where its 'N' bytes are counted.  No lane leaves before the
// shuffles; with BG_FQF_PAIRED n is even, so a record's mate is in range exactly when the record is.
template <int G>
__global__ __launch_bounds__(256) void fq_pass_kernel(const FqfArgs a, uint8_t* __restrict__ keep, uint32_t* __restrict__ k_out,
                                                      uint32_t* __restrict__ sl_out, uint32_t* __restrict__ ql_out) {
    const uint64_t r = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const uint32_t lane = threadIdx.x % G;
    const bool live = r < a.n;
    uint32_t sl = 0, ql = 0, nc = 0;
    if (live) {
        const uint64_t s0 = a.seq_off[r];
        sl = (uint32_t)(a.seq_off[r + 1] - s0);
        ql = (uint32_t)(a.qual_off[r + 1] - a.qual_off[r]);
        if (G > 1) nc = fq_count_n(a.seq + s0, sl, lane, G);
    }
#pragma unroll
    for (int o = G / 2; o; o >>= 1) nc += __shfl_xor(nc, o);
    bool pass = false;
    if (live) {
        const bool trimmed = (a.f.flags & (BG_FQF_DISCARD_UNTRIMMED | BG_FQF_DISCARD_TRIMMED)) && fq_trimmed(a.hits, r, a.n_pat);
        const int32_t check = (a.f.flags & BG_FQF_CHECK_OK) ? a.recs[r].check : BG_FQCHECK_OK;
        pass = fq_passes(a.f, sl, check, trimmed, nc);
    }
    const bool mate = __shfl_xor((int)pass, G) != 0;
    if (!live || lane) return;
    const bool kp = fq_keeps(a.f.flags, pass, mate);
    keep[r] = kp;
    k_out[r] = kp;
    sl_out[r] = kp ? sl : 0;
    ql_out[r] = kp ? ql : 0;
}

// 16 lanes per record; rank / so / qo: the scans' n + 1 entries.  The lanes of the last record also close the offsets.
__global__ __launch_bounds__(256) void fq_copy_kernel(uint64_t n, const uint8_t* __restrict__ keep, const uint64_t* __restrict__ rank,
                                                      const uint64_t* __restrict__ so, const uint64_t* __restrict__ qo,
                                                      const bg_fastq_record_t* __restrict__ recs, const uint8_t* __restrict__ seq,
                                                      const uint64_t* __restrict__ seq_off, const uint8_t* __restrict__ qual,
                                                      const uint64_t* __restrict__ qual_off, bg_fastq_record_t* __restrict__ recs_out,
                                                      uint8_t* __restrict__ seq_out, uint64_t* __restrict__ seq_off_out,
                                                      uint8_t* __restrict__ qual_out, uint64_t* __restrict__ qual_off_out) {
    const uint64_t r = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const uint32_t lane = threadIdx.x & 15;
    if (r >= n) return;
    if (r == n - 1 && lane == 0) {
        seq_off_out[rank[n]] = so[n];
        qual_off_out[rank[n]] = qo[n];
    }
    if (!keep[r]) return;
    const uint64_t s0 = seq_off[r], q0 = qual_off[r];
    fq_copy_record(recs[r], seq + s0, (uint32_t)(seq_off[r + 1] - s0), qual + q0, (uint32_t)(qual_off[r + 1] - q0), rank[r], so[r], qo[r],
                   recs_out, seq_out, seq_off_out, qual_out, qual_off_out, lane, 16);
}

// every refusal says why (bg_last_error), so that each can be told from the others where no device is present
int refuse(const char* why, int rc = BG_ERR_INVALID_ARG) {
    bg_tls_error = why;
    return rc;
}

int filter_check(const bg_ctx* ctx, uint64_t n, const bg_fastq_filter_t* f, const void* hits, uint32_t n_pat, const void* recs, const void* seq,
                 const void* seq_off, const void* qual, const void* qual_off, const void* recs_out, const void* seq_out,
                 const void* seq_off_out, const void* qual_out, const void* qual_off_out) {
    if (!f) return refuse("bg_fastq_filter: null filter");
    const uint32_t known = BG_FQF_PAIRED | BG_FQF_PAIR_BOTH | BG_FQF_DISCARD_UNTRIMMED | BG_FQF_DISCARD_TRIMMED | BG_FQF_CHECK_OK;
    const uint32_t discard = f->flags & (BG_FQF_DISCARD_UNTRIMMED | BG_FQF_DISCARD_TRIMMED);
    if (f->flags & ~known) return refuse("bg_fastq_filter: unknown flag bits");
    if (discard == (BG_FQF_DISCARD_UNTRIMMED | BG_FQF_DISCARD_TRIMMED)) return refuse("bg_fastq_filter: both DISCARD flags");
    if (n_pat > BG_MYERS_MAX_PATTERNS) return refuse("bg_fastq_filter: n_pat above BG_MYERS_MAX_PATTERNS", BG_ERR_TOO_LARGE);
    if (discard && (!hits || n_pat == 0)) return refuse("bg_fastq_filter: a DISCARD flag without hits");
    if ((f->flags & BG_FQF_PAIR_BOTH) && !(f->flags & BG_FQF_PAIRED)) return refuse("bg_fastq_filter: PAIR_BOTH without PAIRED");
    if ((f->flags & BG_FQF_PAIRED) && (n & 1)) return refuse("bg_fastq_filter: PAIRED with an odd record count");
    if (f->min_len > f->max_len) return refuse("bg_fastq_filter: min_len above max_len");
    if (!seq_off_out || !qual_off_out) return refuse("bg_fastq_filter: null output offsets");
    if (n && (!recs || !seq || !seq_off || !qual || !qual_off || !recs_out || !seq_out || !qual_out))
        return refuse("bg_fastq_filter: null column");
    if (!ctx) return refuse("bg_fastq_filter: null ctx");
    return BG_OK;
}

struct FqDev {
    void* p = nullptr;
    ~FqDev() { hipFree(p); }
    int alloc(size_t bytes) {
        BG_HIP(hipMalloc(&p, bytes ? bytes : 1));
        return BG_OK;
    }
};

// ---- emit ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t kStage = 1024;            // bytes of a staged line
constexpr uint32_t kStageBuf = kStage + 16;  // ... plus its offset inside the 16-byte granule of the output

// line j is record first + j * step
__global__ __launch_bounds__(256) void fq_length_kernel(uint64_t m, uint64_t first, uint64_t step, const bg_fastq_record_t* __restrict__ recs,
                                                        uint32_t* __restrict__ len) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < m) len[j] = fq_line_len(recs[first + j * step]);
}

// text pass: 16 lanes per line, 16 lines per block.  WIDE: staged in LDS and stored by fq_line_flush; otherwise (and for a line
// that does not fit the staging area) fq_line_write's bytes go straight to the output.  The two destinations are two calls, so
// that each compiles to stores of its own address space (LDS, global) and not to flat stores through a generic pointer
// (measured: 0.54 -> 0.42 ms per call of 1 M reads for the plain flavour).
constexpr uint32_t kLanes = 16;
template <bool WIDE>
__global__ __launch_bounds__(256) void fq_emit_kernel(uint64_t m, uint64_t first, uint64_t step, const uint8_t* __restrict__ text,
                                                      const bg_fastq_record_t* __restrict__ recs, const uint8_t* __restrict__ seq,
                                                      const uint8_t* __restrict__ qual, const uint64_t* __restrict__ off,
                                                      char* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) char s_stage[WIDE ? (256 / kLanes) * kStageBuf : 16];
    const uint32_t g = threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
    const uint64_t j = (uint64_t)blockIdx.x * (256 / kLanes) + g;
    uint64_t o0 = 0;
    uint32_t len = 0;
    if (j < m) {
        o0 = off[j];
        len = (uint32_t)(off[j + 1] - o0);
    }
    char* line = out + o0;
    const uint32_t mis = (uint32_t)((uintptr_t)line & 15);
    const bool staged = WIDE && len && mis + len <= kStageBuf;
    char* stage = s_stage + (WIDE ? g * kStageBuf + mis : 0);
    if (staged)
        fq_line_write(text, recs[first + j * step], seq, qual, stage, lane, kLanes);
    else if (len)
        fq_line_write(text, recs[first + j * step], seq, qual, line, lane, kLanes);
    if (!WIDE) return;
    __syncthreads();
    if (staged) fq_line_flush(stage, line, len, lane, kLanes);
}

uint64_t emit_lines(uint64_t n, uint64_t first, uint64_t step) { return first < n ? (n - first - 1) / step + 1 : 0; }

int emit_check(const bg_ctx* ctx, uint64_t n, uint64_t first, uint64_t step, const void* text, const void* recs, const void* seq,
               const void* qual, const void* out, uint64_t out_cap, const void* out_off, uint64_t* out_bytes) {
    if (!out_off || !out_bytes) return refuse("bg_fastq_emit: null out_off or out_bytes");
    *out_bytes = 0;
    if (step == 0) return refuse("bg_fastq_emit: step 0");
    if (!out && out_cap) return refuse("bg_fastq_emit: null out with a capacity");
    if (emit_lines(n, first, step) && (!text || !recs || !seq || !qual)) return refuse("bg_fastq_emit: null text, recs, seq or qual");
    if (!ctx) return refuse("bg_fastq_emit: null ctx");
    return BG_OK;
}

}  // namespace

extern "C" int bg_fastq_filter_dev(bg_ctx* ctx, uint64_t n, const bg_fastq_filter_t* flt, const bg_alignment_t* d_hits, uint32_t n_pat,
                                   const bg_fastq_record_t* d_recs, const uint8_t* d_seq, const uint64_t* d_seq_off, const uint8_t* d_qual,
                                   const uint64_t* d_qual_off, bg_fastq_record_t* d_recs_out, uint8_t* d_seq_out, uint64_t* d_seq_off_out,
                                   uint8_t* d_qual_out, uint64_t* d_qual_off_out, uint8_t* d_keep, uint64_t* totals, void* stream) {
    if (int rc = filter_check(ctx, n, flt, d_hits, n_pat, d_recs, d_seq, d_seq_off, d_qual, d_qual_off, d_recs_out, d_seq_out, d_seq_off_out,
                              d_qual_out, d_qual_off_out))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    if (totals) totals[0] = totals[1] = totals[2] = 0;
    if (n == 0) {
        BG_HIP(hipMemsetAsync(d_seq_off_out, 0, 8, st));
        BG_HIP(hipMemsetAsync(d_qual_off_out, 0, 8, st));
        if (totals) BG_HIP(hipStreamSynchronize(st));
        return BG_OK;
    }
    bg_scratch_guard guard(ctx, st);
    // aux: three scanned columns rank / so / qo (uint64[n + 1]) and the block sums of their scans, the three uint32 columns they
    // are scanned from, keep[n]
    const size_t col = (size_t)n + 1, sums = 2 * (size_t)(n / 2048 + 2), words = ((size_t)n * 3 + 1) / 2 * 2;
    if (int rc = bg_reserve(&ctx->aux, &ctx->aux_bytes, (3 * col + 3 * sums) * 8 + words * 4 + n)) return rc;
    uint64_t* d_rank = (uint64_t*)ctx->aux;
    uint64_t* d_so = d_rank + col;
    uint64_t* d_qo = d_so + col;
    uint64_t* d_sums = d_qo + col;
    uint32_t* d_k = (uint32_t*)(d_sums + 3 * sums);
    uint32_t* d_sl = d_k + n;
    uint32_t* d_ql = d_sl + n;
    uint8_t* keep = d_keep ? d_keep : (uint8_t*)(d_k + words);
    const FqfArgs a = {n, *flt, d_hits, n_pat, d_recs, d_seq, d_seq_off, d_qual_off};
    if (flt->max_n != 0xFFFFFFFFu)
        fq_pass_kernel<16><<<dim3((uint32_t)((n * 16 + 255) / 256)), dim3(256), 0, st>>>(a, keep, d_k, d_sl, d_ql);
    else
        fq_pass_kernel<1><<<dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st>>>(a, keep, d_k, d_sl, d_ql);
    BG_HIP(hipGetLastError());
    if (int rc = bg_scan_u32(d_k, n, d_rank, d_sums, st)) return rc;
    if (int rc = bg_scan_u32(d_sl, n, d_so, d_sums + sums, st)) return rc;
    if (int rc = bg_scan_u32(d_ql, n, d_qo, d_sums + 2 * sums, st)) return rc;
    fq_copy_kernel<<<dim3((uint32_t)((n * 16 + 255) / 256)), dim3(256), 0, st>>>(n, keep, d_rank, d_so, d_qo, d_recs, d_seq, d_seq_off, d_qual,
                                                                                 d_qual_off, d_recs_out, d_seq_out, d_seq_off_out, d_qual_out,
                                                                                 d_qual_off_out);
    BG_HIP(hipGetLastError());
    if (totals) {
        BG_HIP(hipMemcpyAsync(&totals[0], d_rank + n, 8, hipMemcpyDeviceToHost, st));
        BG_HIP(hipMemcpyAsync(&totals[1], d_so + n, 8, hipMemcpyDeviceToHost, st));
        BG_HIP(hipMemcpyAsync(&totals[2], d_qo + n, 8, hipMemcpyDeviceToHost, st));
        BG_HIP(hipStreamSynchronize(st));
    }
    return BG_OK;
}

extern "C" int bg_fastq_filter(bg_ctx* ctx, uint64_t n, const bg_fastq_filter_t* flt, const bg_alignment_t* hits, uint32_t n_pat,
                               const bg_fastq_record_t* recs, const uint8_t* seq, const uint64_t* seq_off, const uint8_t* qual,
                               const uint64_t* qual_off, bg_fastq_record_t* recs_out, uint8_t* seq_out, uint64_t* seq_off_out,
                               uint8_t* qual_out, uint64_t* qual_off_out, uint8_t* keep, uint64_t* totals) {
    if (int rc = filter_check(ctx, n, flt, hits, n_pat, recs, seq, seq_off, qual, qual_off, recs_out, seq_out, seq_off_out, qual_out,
                              qual_off_out))
        return rc;
    BG_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t sb = n ? seq_off[n] : 0, qb = n ? qual_off[n] : 0;
    FqDev d_hits, d_recs, d_seq, d_so, d_qual, d_qo, o_recs, o_seq, o_so, o_qual, o_qo, o_keep;
    const size_t hb = hits ? (size_t)n * n_pat * sizeof(bg_alignment_t) : 0, rb = (size_t)n * sizeof(bg_fastq_record_t),
                 ob = (size_t)(n + 1) * 8;
    for (auto pr : {std::pair<FqDev*, size_t>{&d_hits, hb}, {&d_recs, rb}, {&d_seq, sb}, {&d_so, ob}, {&d_qual, qb}, {&d_qo, ob},
                    {&o_recs, rb}, {&o_seq, sb}, {&o_so, ob}, {&o_qual, qb}, {&o_qo, ob}, {&o_keep, (size_t)n}})
        if (int rc = pr.first->alloc(pr.second)) return rc;
    if (n) {
        if (hb) BG_HIP(hipMemcpyAsync(d_hits.p, hits, hb, hipMemcpyHostToDevice, st));
        BG_HIP(hipMemcpyAsync(d_recs.p, recs, rb, hipMemcpyHostToDevice, st));
        if (sb) BG_HIP(hipMemcpyAsync(d_seq.p, seq, sb, hipMemcpyHostToDevice, st));
        if (qb) BG_HIP(hipMemcpyAsync(d_qual.p, qual, qb, hipMemcpyHostToDevice, st));
        BG_HIP(hipMemcpyAsync(d_so.p, seq_off, ob, hipMemcpyHostToDevice, st));
        BG_HIP(hipMemcpyAsync(d_qo.p, qual_off, ob, hipMemcpyHostToDevice, st));
        BG_HIP(hipStreamSynchronize(st));
    }
    uint64_t tot[3] = {0, 0, 0};
    if (int rc = bg_fastq_filter_dev(ctx, n, flt, hits ? (const bg_alignment_t*)d_hits.p : nullptr, n_pat, (const bg_fastq_record_t*)d_recs.p,
                                     (const uint8_t*)d_seq.p, (const uint64_t*)d_so.p, (const uint8_t*)d_qual.p, (const uint64_t*)d_qo.p,
                                     (bg_fastq_record_t*)o_recs.p, (uint8_t*)o_seq.p, (uint64_t*)o_so.p, (uint8_t*)o_qual.p,
                                     (uint64_t*)o_qo.p, (uint8_t*)o_keep.p, tot, st))
        return rc;
    if (tot[0]) BG_HIP(hipMemcpyAsync(recs_out, o_recs.p, (size_t)tot[0] * sizeof(bg_fastq_record_t), hipMemcpyDeviceToHost, st));
    if (tot[1]) BG_HIP(hipMemcpyAsync(seq_out, o_seq.p, tot[1], hipMemcpyDeviceToHost, st));
    if (tot[2]) BG_HIP(hipMemcpyAsync(qual_out, o_qual.p, tot[2], hipMemcpyDeviceToHost, st));
    BG_HIP(hipMemcpyAsync(seq_off_out, o_so.p, (size_t)(tot[0] + 1) * 8, hipMemcpyDeviceToHost, st));
    BG_HIP(hipMemcpyAsync(qual_off_out, o_qo.p, (size_t)(tot[0] + 1) * 8, hipMemcpyDeviceToHost, st));
    if (keep && n) BG_HIP(hipMemcpyAsync(keep, o_keep.p, n, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    if (totals) std::copy(tot, tot + 3, totals);
    return BG_OK;
}

extern "C" int bg_fastq_emit_dev(bg_ctx* ctx, uint64_t n, uint64_t first, uint64_t step, const uint8_t* d_fastq_text,
                                 const bg_fastq_record_t* d_recs, const uint8_t* d_seq, const uint8_t* d_qual, char* d_out, uint64_t out_cap,
                                 uint64_t* d_out_off, uint64_t* out_bytes, void* stream) {
    if (int rc = emit_check(ctx, n, first, step, d_fastq_text, d_recs, d_seq, d_qual, d_out, out_cap, d_out_off, out_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    const uint64_t m = emit_lines(n, first, step);
    if (m == 0) {
        BG_HIP(hipMemsetAsync(d_out_off, 0, 8, st));
        BG_HIP(hipStreamSynchronize(st));
        return BG_OK;
    }
    bg_scratch_guard guard(ctx, st);
    const size_t len_bytes = ((size_t)m * 4 + 15) & ~(size_t)15;
    if (int rc = bg_reserve(&ctx->aux, &ctx->aux_bytes, len_bytes + 2 * (size_t)(m / 2048 + 2) * 8)) return rc;
    uint32_t* d_len = (uint32_t*)ctx->aux;
    uint64_t* d_sums = (uint64_t*)((uint8_t*)ctx->aux + len_bytes);
    fq_length_kernel<<<dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st>>>(m, first, step, d_recs, d_len);
    BG_HIP(hipGetLastError());
    if (int rc = bg_scan_u32(d_len, m, d_out_off, d_sums, st)) return rc;
    uint64_t total = 0;
    BG_HIP(hipMemcpyAsync(&total, d_out_off + m, 8, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    *out_bytes = total;
    if (!d_out) return BG_OK;
    if (total > out_cap) return BG_ERR_OPS_CAP;
    const dim3 grid((uint32_t)((m + 15) / 16));
    if (ctx->fq_emit_mode == 2)
        fq_emit_kernel<true><<<grid, dim3(256), 0, st>>>(m, first, step, d_fastq_text, d_recs, d_seq, d_qual, d_out_off, d_out);
    else
        fq_emit_kernel<false><<<grid, dim3(256), 0, st>>>(m, first, step, d_fastq_text, d_recs, d_seq, d_qual, d_out_off, d_out);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

extern "C" int bg_fastq_emit(bg_ctx* ctx, uint64_t n, uint64_t first, uint64_t step, const uint8_t* fastq_text,
                             const bg_fastq_record_t* recs, const uint8_t* seq, const uint8_t* qual, char* out, uint64_t out_cap,
                             uint64_t* out_off, uint64_t* out_bytes) {
    if (int rc = emit_check(ctx, n, first, step, fastq_text, recs, seq, qual, out, out_cap, out_off, out_bytes)) return rc;
    out_off[0] = 0;
    const uint64_t m = emit_lines(n, first, step);
    if (m == 0) return BG_OK;
    BG_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // the buffers the written records point into end where the last of them ends
    uint64_t fq_bytes = 0, seq_bytes = 0, qual_bytes = 0;
    for (uint64_t r = first; r < n; r += step) {
        fq_bytes = std::max<uint64_t>(fq_bytes, recs[r].id_off + recs[r].id_len);
        if (recs[r].has_desc) fq_bytes = std::max<uint64_t>(fq_bytes, recs[r].desc_off + recs[r].desc_len);
        seq_bytes = std::max<uint64_t>(seq_bytes, recs[r].seq_off + recs[r].seq_len);
        qual_bytes = std::max<uint64_t>(qual_bytes, recs[r].qual_off + recs[r].qual_len);
        if (n - r <= step) break;  // r + step would pass n (or wrap)
    }
    FqDev d_fq, d_recs, d_seq, d_qual, d_off, d_out;
    const size_t rb = (size_t)n * sizeof(bg_fastq_record_t), ob = (size_t)(m + 1) * 8;
    for (auto pr : {std::pair<FqDev*, size_t>{&d_fq, fq_bytes}, {&d_recs, rb}, {&d_seq, seq_bytes}, {&d_qual, qual_bytes}, {&d_off, ob},
                    {&d_out, out ? (size_t)out_cap : 0}})
        if (int rc = pr.first->alloc(pr.second)) return rc;
    if (fq_bytes) BG_HIP(hipMemcpyAsync(d_fq.p, fastq_text, fq_bytes, hipMemcpyHostToDevice, st));
    BG_HIP(hipMemcpyAsync(d_recs.p, recs, rb, hipMemcpyHostToDevice, st));
    if (seq_bytes) BG_HIP(hipMemcpyAsync(d_seq.p, seq, seq_bytes, hipMemcpyHostToDevice, st));
    if (qual_bytes) BG_HIP(hipMemcpyAsync(d_qual.p, qual, qual_bytes, hipMemcpyHostToDevice, st));
    const int rc = bg_fastq_emit_dev(ctx, n, first, step, (const uint8_t*)d_fq.p, (const bg_fastq_record_t*)d_recs.p, (const uint8_t*)d_seq.p,
                                     (const uint8_t*)d_qual.p, out ? (char*)d_out.p : nullptr, out_cap, (uint64_t*)d_off.p, out_bytes, st);
    if (rc && rc != BG_ERR_OPS_CAP) return rc;
    BG_HIP(hipMemcpyAsync(out_off, d_off.p, ob, hipMemcpyDeviceToHost, st));
    if (!rc && out && *out_bytes) BG_HIP(hipMemcpyAsync(out, d_out.p, *out_bytes, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    return rc;
}
