// bg_fastq_trim[_dev]: cut adapters off parsed FASTQ records by the hits of bg_myers_best_batch[_dev] without a host
// round trip (include/biogpu.h has the rule; rust-bio has no trimmer).  Three steps on the stream: the kept range and
// the two lengths of every read (one lane per read), the shared exclusive scan (scan.hip) of the sequence and of the
// quality lengths into the output offsets, and the copy (16 lanes per read; lane 0 writes the record).
#include "bg_common.h"

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

struct TrimDev {
    void* p = nullptr;
    ~TrimDev() { hipFree(p); }
    int alloc(size_t bytes) {
        BG_HIP(hipMalloc(&p, bytes ? bytes : 1));
        return BG_OK;
    }
};

}  // namespace

extern "C" int bg_fastq_trim_dev(bg_ctx* ctx, uint64_t n, int mode, const bg_alignment_t* d_hits, uint32_t n_pat,
                                 const bg_fastq_record_t* d_recs, const uint8_t* d_seq, const uint64_t* d_seq_off,
                                 const uint8_t* d_qual, const uint64_t* d_qual_off, bg_fastq_record_t* d_recs_out,
                                 uint8_t* d_seq_out, uint64_t* d_seq_off_out, uint8_t* d_qual_out, uint64_t* d_qual_off_out,
                                 uint64_t* totals, void* stream) {
    if (mode != BG_TRIM_3P && mode != BG_TRIM_5P) return BG_ERR_INVALID_ARG;
    if (n_pat == 0 || n_pat > BG_MYERS_MAX_PATTERNS) return n_pat ? BG_ERR_TOO_LARGE : BG_ERR_INVALID_ARG;
    if (!ctx || !d_seq_off_out || !d_qual_off_out) return BG_ERR_INVALID_ARG;
    if (n && (!d_hits || !d_recs || !d_seq || !d_seq_off || !d_qual || !d_qual_off || !d_recs_out || !d_seq_out || !d_qual_out))
        return BG_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);
    // aux: lo[n], seq_len[n], qual_len[n] (uint32), then the block sums of the two scans
    const size_t words = ((size_t)n * 3 + 1) / 2 * 2, sums = 2 * (size_t)(n / 2048 + 2);
    if (int rc = bg_reserve(&ctx->aux, &ctx->aux_bytes, words * 4 + 2 * sums * 8)) return rc;
    uint32_t* d_lo = (uint32_t*)ctx->aux;
    uint32_t* d_sl = d_lo + n;
    uint32_t* d_ql = d_sl + n;
    uint64_t* d_sums = (uint64_t*)(d_lo + words);
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
    if (mode != BG_TRIM_3P && mode != BG_TRIM_5P) return BG_ERR_INVALID_ARG;
    if (n_pat == 0 || n_pat > BG_MYERS_MAX_PATTERNS) return n_pat ? BG_ERR_TOO_LARGE : BG_ERR_INVALID_ARG;
    if (!ctx || !seq_off_out || !qual_off_out) return BG_ERR_INVALID_ARG;
    if (n && (!hits || !recs || !seq || !seq_off || !qual || !qual_off || !recs_out || !seq_out || !qual_out)) return BG_ERR_INVALID_ARG;
    BG_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t sb = n ? seq_off[n] : 0, qb = n ? qual_off[n] : 0;
    TrimDev d_hits, d_recs, d_seq, d_so, d_qual, d_qo, o_recs, o_seq, o_so, o_qual, o_qo;
    const size_t hb = (size_t)n * n_pat * sizeof(bg_alignment_t), rb = (size_t)n * sizeof(bg_fastq_record_t), ob = (size_t)(n + 1) * 8;
    for (auto pr : {std::pair<TrimDev*, size_t>{&d_hits, hb}, {&d_recs, rb}, {&d_seq, sb}, {&d_so, ob}, {&d_qual, qb}, {&d_qo, ob},
                    {&o_recs, rb}, {&o_seq, sb}, {&o_so, ob}, {&o_qual, qb}, {&o_qo, ob}})
        if (int rc = pr.first->alloc(pr.second)) return rc;
    if (n) {
        BG_HIP(hipMemcpyAsync(d_hits.p, hits, hb, hipMemcpyHostToDevice, st));
        BG_HIP(hipMemcpyAsync(d_recs.p, recs, rb, hipMemcpyHostToDevice, st));
        if (sb) BG_HIP(hipMemcpyAsync(d_seq.p, seq, sb, hipMemcpyHostToDevice, st));
        if (qb) BG_HIP(hipMemcpyAsync(d_qual.p, qual, qb, hipMemcpyHostToDevice, st));
        BG_HIP(hipMemcpyAsync(d_so.p, seq_off, ob, hipMemcpyHostToDevice, st));
        BG_HIP(hipMemcpyAsync(d_qo.p, qual_off, ob, hipMemcpyHostToDevice, st));
        BG_HIP(hipStreamSynchronize(st));
    }
    uint64_t tot[2] = {0, 0};
    if (int rc = bg_fastq_trim_dev(ctx, n, mode, (const bg_alignment_t*)d_hits.p, n_pat, (const bg_fastq_record_t*)d_recs.p,
                                   (const uint8_t*)d_seq.p, (const uint64_t*)d_so.p, (const uint8_t*)d_qual.p, (const uint64_t*)d_qo.p,
                                   (bg_fastq_record_t*)o_recs.p, (uint8_t*)o_seq.p, (uint64_t*)o_so.p, (uint8_t*)o_qual.p,
                                   (uint64_t*)o_qo.p, tot, st))
        return rc;
    if (n) BG_HIP(hipMemcpyAsync(recs_out, o_recs.p, rb, hipMemcpyDeviceToHost, st));
    if (tot[0]) BG_HIP(hipMemcpyAsync(seq_out, o_seq.p, tot[0], hipMemcpyDeviceToHost, st));
    if (tot[1]) BG_HIP(hipMemcpyAsync(qual_out, o_qual.p, tot[1], hipMemcpyDeviceToHost, st));
    BG_HIP(hipMemcpyAsync(seq_off_out, o_so.p, ob, hipMemcpyDeviceToHost, st));
    BG_HIP(hipMemcpyAsync(qual_off_out, o_qo.p, ob, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    if (totals) {
        totals[0] = tot[0];
        totals[1] = tot[1];
    }
    return BG_OK;
}
