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
//
// The host flavours stage their arrays through a bg_stage: the filter its columns by fastq_cols.h, the writer as much of the
// text and of the two byte columns as the written records reach into (fq_record_extents).
#include "fastq_cols.h"
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

// every refusal says why (bg_refuse); device or host pointers alike
int filter_check(const bg_ctx* ctx, uint64_t n, const bg_fastq_filter_t* f, const void* hits, uint32_t n_pat, const fq_cols_in& in,
                 const fq_cols_out& out) {
    if (!f) return bg_refuse("bg_fastq_filter: null filter");
    const uint32_t known = BG_FQF_PAIRED | BG_FQF_PAIR_BOTH | BG_FQF_DISCARD_UNTRIMMED | BG_FQF_DISCARD_TRIMMED | BG_FQF_CHECK_OK;
    const uint32_t discard = f->flags & (BG_FQF_DISCARD_UNTRIMMED | BG_FQF_DISCARD_TRIMMED);
    if (f->flags & ~known) return bg_refuse("bg_fastq_filter: unknown flag bits");
    if (discard == (BG_FQF_DISCARD_UNTRIMMED | BG_FQF_DISCARD_TRIMMED)) return bg_refuse("bg_fastq_filter: both DISCARD flags");
    if (n_pat > BG_MYERS_MAX_PATTERNS) return bg_refuse("bg_fastq_filter: n_pat above BG_MYERS_MAX_PATTERNS", BG_ERR_TOO_LARGE);
    if (discard && (!hits || n_pat == 0)) return bg_refuse("bg_fastq_filter: a DISCARD flag without hits");
    if ((f->flags & BG_FQF_PAIR_BOTH) && !(f->flags & BG_FQF_PAIRED)) return bg_refuse("bg_fastq_filter: PAIR_BOTH without PAIRED");
    if ((f->flags & BG_FQF_PAIRED) && (n & 1)) return bg_refuse("bg_fastq_filter: PAIRED with an odd record count");
    if (f->min_len > f->max_len) return bg_refuse("bg_fastq_filter: min_len above max_len");
    if (!out.offsets()) return bg_refuse("bg_fastq_filter: null output offsets");
    if (n && (!in.complete() || !out.data())) return bg_refuse("bg_fastq_filter: null column");
    if (!ctx) return bg_refuse("bg_fastq_filter: null ctx");
    return BG_OK;
}

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

int emit_check(const bg_ctx* ctx, uint64_t n, uint64_t first, uint64_t step, const void* text, const void* recs, const void* seq,
               const void* qual, const void* out, uint64_t out_cap, const void* out_off, uint64_t* out_bytes) {
    if (!out_off || !out_bytes) return bg_refuse("bg_fastq_emit: null out_off or out_bytes");
    *out_bytes = 0;
    if (step == 0) return bg_refuse("bg_fastq_emit: step 0");
    if (!out && out_cap) return bg_refuse("bg_fastq_emit: null out with a capacity");
    if (fq_strided_count(n, first, step) && (!text || !recs || !seq || !qual)) return bg_refuse("bg_fastq_emit: null text, recs, seq or qual");
    if (!ctx) return bg_refuse("bg_fastq_emit: null ctx");
    return BG_OK;
}

}  // namespace

extern "C" int bg_fastq_filter_dev(bg_ctx* ctx, uint64_t n, const bg_fastq_filter_t* flt, const bg_alignment_t* d_hits, uint32_t n_pat,
                                   const bg_fastq_record_t* d_recs, const uint8_t* d_seq, const uint64_t* d_seq_off, const uint8_t* d_qual,
                                   const uint64_t* d_qual_off, bg_fastq_record_t* d_recs_out, uint8_t* d_seq_out, uint64_t* d_seq_off_out,
                                   uint8_t* d_qual_out, uint64_t* d_qual_off_out, uint8_t* d_keep, uint64_t* totals, void* stream) {
    if (int rc = filter_check(ctx, n, flt, d_hits, n_pat, {d_recs, d_seq, d_seq_off, d_qual, d_qual_off},
                              {d_recs_out, d_seq_out, d_seq_off_out, d_qual_out, d_qual_off_out}))
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
    // aux: three scanned columns rank / so / qo and the block sums of their scans, the three columns they are scanned from, keep
    const size_t sums = bg_scan_sums_words(n);
    uint64_t *d_rank, *d_so, *d_qo, *d_sums;
    uint32_t *d_k, *d_sl, *d_ql;
    uint8_t* keep;
    if (int rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_rank = cv.take<uint64_t>(n + 1), d_so = cv.take<uint64_t>(n + 1), d_qo = cv.take<uint64_t>(n + 1);
        d_sums = cv.take<uint64_t>(3 * sums);  // one piece: scan k has d_sums + k * sums
        d_k = cv.take<uint32_t>(n), d_sl = cv.take<uint32_t>(n), d_ql = cv.take<uint32_t>(n);
        keep = d_keep ? d_keep : cv.take<uint8_t>(n);
    })) return rc;
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
    const fq_cols_in in = {recs, seq, seq_off, qual, qual_off};
    const fq_cols_out out = {recs_out, seq_out, seq_off_out, qual_out, qual_off_out};
    if (int rc = filter_check(ctx, n, flt, hits, n_pat, in, out)) return rc;
    bg_stage s(ctx, ctx->stream);
    const bg_alignment_t* d_hits = hits ? s.up(hits, (size_t)n * n_pat) : nullptr;
    const fq_cols_in d = fq_cols_upload(s, n, in);
    const fq_cols_out o = fq_cols_alloc(s, n, n ? seq_off[n] : 0, n ? qual_off[n] : 0);
    uint8_t* d_keep = s.out<uint8_t>(n);
    if (s.sync()) return s.rc;
    uint64_t tot[3] = {0, 0, 0};
    if (int rc = bg_fastq_filter_dev(ctx, n, flt, d_hits, n_pat, d.recs, d.seq, d.seq_off, d.qual, d.qual_off, o.recs, o.seq, o.seq_off, o.qual,
                                     o.qual_off, d_keep, tot, s.st))
        return rc;
    fq_cols_download(s, out, o, tot[0], tot[1], tot[2]);
    if (keep) s.down(keep, d_keep, n);
    if (s.sync()) return s.rc;
    if (totals) std::copy(tot, tot + 3, totals);
    return BG_OK;
}

extern "C" int bg_fastq_emit_dev(bg_ctx* ctx, uint64_t n, uint64_t first, uint64_t step, const uint8_t* d_fastq_text,
                                 const bg_fastq_record_t* d_recs, const uint8_t* d_seq, const uint8_t* d_qual, char* d_out, uint64_t out_cap,
                                 uint64_t* d_out_off, uint64_t* out_bytes, void* stream) {
    if (int rc = emit_check(ctx, n, first, step, d_fastq_text, d_recs, d_seq, d_qual, d_out, out_cap, d_out_off, out_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    const uint64_t m = fq_strided_count(n, first, step);
    if (m == 0) {
        BG_HIP(hipMemsetAsync(d_out_off, 0, 8, st));
        BG_HIP(hipStreamSynchronize(st));
        return BG_OK;
    }
    bg_scratch_guard guard(ctx, st);
    uint32_t* d_len;
    uint64_t* d_sums;
    if (int rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_len = cv.take<uint32_t>(m);
        d_sums = cv.take<uint64_t>(bg_scan_sums_words(m));
    })) return rc;
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
    const uint64_t m = fq_strided_count(n, first, step);
    if (m == 0) return BG_OK;
    const fq_extents e = fq_record_extents(recs, n, first, step);  // as much of the three buffers as the written records reach into
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_fq = s.up(fastq_text, std::max(e.id, e.desc));
    const bg_fastq_record_t* d_recs = s.up(recs, n);
    const uint8_t* d_seq = s.up(seq, e.seq);
    const uint8_t* d_qual = s.up(qual, e.qual);
    uint64_t* d_off = s.out<uint64_t>(m + 1);
    char* d_out = out ? s.out<char>(out_cap) : nullptr;
    if (s.rc) return s.rc;
    const int rc = bg_fastq_emit_dev(ctx, n, first, step, d_fq, d_recs, d_seq, d_qual, d_out, out_cap, d_off, out_bytes, s.st);
    if (rc && rc != BG_ERR_OPS_CAP) return rc;
    s.down(out_off, d_off, m + 1);
    if (!rc && out) s.down(out, d_out, *out_bytes);
    return s.sync() ? s.rc : rc;
}
