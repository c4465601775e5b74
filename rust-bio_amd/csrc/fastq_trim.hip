// bg_fastq_trim[_dev]: cut adapters off parsed FASTQ records by the hits of bg_myers_best_batch[_dev] without a host
// round trip (include/biogpu.h has the rule; rust-bio has no trimmer).  Three steps on the stream: the kept range and
// the two lengths of every read (one lane per read), the shared exclusive scan (scan.hip) of the sequence and of the
// quality lengths into the output offsets, and the copy (16 lanes per read; lane 0 writes the record).  The host flavour
// stages its columns through fastq_cols.h.
#include "fastq_cols.h"

namespace {

__global__ __launch_bounds__(256) void trim_lengths_kernel(uint64_t n, int mode, const bg_alignment_t* __restrict__ hits, uint32_t n_pat,
                                                           const uint64_t* __restrict__ seq_off, const uint64_t* __restrict__ qual_off,
                                                           uint32_t* __restrict__ lo_out, uint32_t* __restrict__ seq_len_out,
                                                           uint32_t* __restrict__ qual_len_out) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint32_t sl = (uint32_t)(seq_off[r + 1] - seq_off[r]), ql = (uint32_t)(qual_off[r + 1] - qual_off[r]);
    uint32_t lo = 0, hi = sl;
    bool any = false;
    uint32_t e = 0xFFFFFFFFu, b = 0;
    for (uint32_t p = 0; p < n_pat; p++) {
        const bg_alignment_t* h = hits + r * n_pat + p;
        if (h->score == BG_MIN_SCORE) continue;
        any = true;
        e = min(e, h->ystart);
        b = max(b, h->yend);
    }
    if (any) {
        if (mode == BG_TRIM_3P)
            hi = min(sl, e);
        else
            lo = min(sl, b);
    }
    lo_out[r] = lo;
    seq_len_out[r] = hi - lo;
    qual_len_out[r] = min(hi, ql) - min(lo, ql);
}

__global__ __launch_bounds__(256) void trim_copy_kernel(uint64_t n, const bg_fastq_record_t* __restrict__ recs, const uint8_t* __restrict__ seq,
                                                        const uint64_t* __restrict__ seq_off, const uint8_t* __restrict__ qual,
                                                        const uint64_t* __restrict__ qual_off, const uint32_t* __restrict__ lo_in,
                                                        bg_fastq_record_t* __restrict__ recs_out, uint8_t* __restrict__ seq_out,
                                                        const uint64_t* __restrict__ seq_off_out, uint8_t* __restrict__ qual_out,
                                                        const uint64_t* __restrict__ qual_off_out) {
    const uint64_t r = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15;
    if (r >= n) return;
    const uint32_t lo = lo_in[r];
    const uint64_t so = seq_off_out[r], qo = qual_off_out[r];
    const uint32_t sl = (uint32_t)(seq_off_out[r + 1] - so), ql = (uint32_t)(qual_off_out[r + 1] - qo);
    const uint32_t src_ql = (uint32_t)(qual_off[r + 1] - qual_off[r]);
    const uint8_t* s = seq + seq_off[r] + lo;
    const uint8_t* q = qual + qual_off[r] + min(lo, src_ql);
    for (uint32_t i = sub; i < sl; i += 16) seq_out[so + i] = s[i];
    for (uint32_t i = sub; i < ql; i += 16) qual_out[qo + i] = q[i];
    if (sub == 0) {
        bg_fastq_record_t o = recs[r];
        o.seq_off = so;
        o.qual_off = qo;
        o.seq_len = sl;
        o.qual_len = ql;
        recs_out[r] = o;
    }
}

// what both entry points refuse, device or host pointers alike; the codes carry no message
int trim_check(const bg_ctx* ctx, uint64_t n, int mode, const void* hits, uint32_t n_pat, const fq_cols_in& in, const fq_cols_out& out) {
    if (mode != BG_TRIM_3P && mode != BG_TRIM_5P) return BG_ERR_INVALID_ARG;
    if (n_pat == 0 || n_pat > BG_MYERS_MAX_PATTERNS) return n_pat ? BG_ERR_TOO_LARGE : BG_ERR_INVALID_ARG;
    if (!ctx || !out.offsets()) return BG_ERR_INVALID_ARG;
    if (n && (!hits || !in.complete() || !out.data())) return BG_ERR_INVALID_ARG;
    return BG_OK;
}

}  // namespace

extern "C" int bg_fastq_trim_dev(bg_ctx* ctx, uint64_t n, int mode, const bg_alignment_t* d_hits, uint32_t n_pat,
                                 const bg_fastq_record_t* d_recs, const uint8_t* d_seq, const uint64_t* d_seq_off,
                                 const uint8_t* d_qual, const uint64_t* d_qual_off, bg_fastq_record_t* d_recs_out,
                                 uint8_t* d_seq_out, uint64_t* d_seq_off_out, uint8_t* d_qual_out, uint64_t* d_qual_off_out,
                                 uint64_t* totals, void* stream) {
    if (int rc = trim_check(ctx, n, mode, d_hits, n_pat, {d_recs, d_seq, d_seq_off, d_qual, d_qual_off},
                            {d_recs_out, d_seq_out, d_seq_off_out, d_qual_out, d_qual_off_out}))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);
    const size_t sums = bg_scan_sums_words(n);
    uint32_t *d_lo, *d_sl, *d_ql;
    uint64_t* d_sums;
    if (int rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_lo = cv.take<uint32_t>(n), d_sl = cv.take<uint32_t>(n), d_ql = cv.take<uint32_t>(n);
        d_sums = cv.take<uint64_t>(2 * sums);  // the block sums of the two scans
    })) return rc;
    if (n) {
        trim_lengths_kernel<<<dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st>>>(n, mode, d_hits, n_pat, d_seq_off, d_qual_off, d_lo,
                                                                                     d_sl, d_ql);
        BG_HIP(hipGetLastError());
    }
    if (int rc = bg_scan_u32(d_sl, n, d_seq_off_out, d_sums, st)) return rc;
    if (int rc = bg_scan_u32(d_ql, n, d_qual_off_out, d_sums + sums, st)) return rc;
    if (n) {
        trim_copy_kernel<<<dim3((uint32_t)((n * 16 + 255) / 256)), dim3(256), 0, st>>>(n, d_recs, d_seq, d_seq_off, d_qual, d_qual_off, d_lo,
                                                                                       d_recs_out, d_seq_out, d_seq_off_out, d_qual_out,
                                                                                       d_qual_off_out);
        BG_HIP(hipGetLastError());
    }
    if (totals) {
        BG_HIP(hipMemcpyAsync(&totals[0], d_seq_off_out + n, 8, hipMemcpyDeviceToHost, st));
        BG_HIP(hipMemcpyAsync(&totals[1], d_qual_off_out + n, 8, hipMemcpyDeviceToHost, st));
        BG_HIP(hipStreamSynchronize(st));
    }
    return BG_OK;
}

extern "C" int bg_fastq_trim(bg_ctx* ctx, uint64_t n, int mode, const bg_alignment_t* hits, uint32_t n_pat,
                             const bg_fastq_record_t* recs, const uint8_t* seq, const uint64_t* seq_off, const uint8_t* qual,
                             const uint64_t* qual_off, bg_fastq_record_t* recs_out, uint8_t* seq_out, uint64_t* seq_off_out,
                             uint8_t* qual_out, uint64_t* qual_off_out, uint64_t* totals) {
    const fq_cols_in in = {recs, seq, seq_off, qual, qual_off};
    const fq_cols_out out = {recs_out, seq_out, seq_off_out, qual_out, qual_off_out};
    if (int rc = trim_check(ctx, n, mode, hits, n_pat, in, out)) return rc;
    bg_stage s(ctx, ctx->stream);
    const bg_alignment_t* d_hits = s.up(hits, (size_t)n * n_pat);
    const fq_cols_in d = fq_cols_upload(s, n, in);
    const fq_cols_out o = fq_cols_alloc(s, n, n ? seq_off[n] : 0, n ? qual_off[n] : 0);
    if (s.sync()) return s.rc;
    uint64_t tot[2] = {0, 0};
    if (int rc = bg_fastq_trim_dev(ctx, n, mode, d_hits, n_pat, d.recs, d.seq, d.seq_off, d.qual, d.qual_off, o.recs, o.seq, o.seq_off, o.qual,
                                   o.qual_off, tot, s.st))
        return rc;
    fq_cols_download(s, out, o, n, tot[0], tot[1]);
    if (s.sync()) return s.rc;
    if (totals) {
        totals[0] = tot[0];
        totals[1] = tot[1];
    }
    return BG_OK;
}
