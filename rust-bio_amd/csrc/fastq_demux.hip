// bg_fastq_demux_assign[_dev] and bg_fastq_demux_split[_dev]: which sample a read belongs to, by the records of a Myers best
// call, and the stable grouping of parsed, trimmed or filtered records by sample (include/biogpu.h has both rules; rust-bio
// has no demultiplexer).  The per-record bodies are in fastq_demux_rule.h.
//
// Assign, 1 launch: a read's records are 64 bytes apart, so a group of lanes takes a read (1 lane below 16 patterns, 16
// otherwise) and strides over its patterns; the group reduces (winner's score, pattern, bin; best score of any other bin) by
// shuffles, the pair rule is one more shuffle with the neighbouring group, and the group's lanes write the 16 words of
// hit_out.  No lane leaves before the shuffles.  pat_bin travels by value, 16 bits an entry: nothing is staged, nothing of
// the caller's is read after the call returns.
//
// Split, 13 launches — one wide radix pass over up to 1026 groups: a histogram per tile of 2048 records and per group in LDS
// (atomics only count), written group-major; the shared scan (scan.hip) over that table gives every (group, tile) its base
// rank; the rank kernel gives every record its stable rank inside its tile's group — per-wavefront counts in LDS turned
// into bases in wavefront order, then, step by step in input order, the earlier lanes of the same group by ballots over the
// bits of the group number — and writes perm[k] and the two lengths at k; two more scans give the byte offsets; the copy
// kernel (16 lanes per output record, the filter's fq_copy_record) moves the bytes.  No atomic decides an order.
//
// The host flavours stage their arrays through a bg_stage, the split its columns by fastq_cols.h.
#include "fastq_cols.h"
#include "fastq_demux_rule.h"

namespace {

// ---- assign -------------------------------------------------------------------------------------------------------------
// G lanes per read.  With BG_DMX_PAIRED n is even and 256 / G is, so a read's mate is in the same wavefront and in range
// exactly when the read is.
template <int G>
__global__ __launch_bounds__(256) void dmx_assign_kernel(uint64_t n, const bg_demux_params_t prm, const bg_alignment_t* __restrict__ hits,
                                                         uint32_t n_pat, const dmx_bins bins, uint32_t* __restrict__ bin_out,
                                                         bg_alignment_t* __restrict__ hit_out, uint32_t* __restrict__ pat_out) {
    const uint64_t r = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const uint32_t lane = threadIdx.x % G, mate = (uint32_t)(r & 1);
    const bool live = r < n;
    const bg_alignment_t* mine = hits + r * n_pat;
    dmx_state s = dmx_empty();
    if (live && dmx_mate_counts(prm.flags, mate)) s = dmx_lane_share(mine, n_pat, bins.b, prm.flags, prm.max_offset, lane, G);
    auto from = [&](const dmx_state& v, int o) {
        return dmx_state{__shfl_xor(v.s1, o), (uint32_t)__shfl_xor((int)v.p1, o), (uint32_t)__shfl_xor((int)v.bin1, o), __shfl_xor(v.s2, o),
                         (uint32_t)__shfl_xor((int)v.has2, o)};
    };
#pragma unroll
    for (int o = G / 2; o; o >>= 1) s = dmx_merge(s, from(s, o));
    bool holds = !dmx_is_empty(s);
    const dmx_state other = from(s, G);
    if (prm.flags & BG_DMX_PAIRED) s = dmx_pair(s, other, mate, &holds);
    if (!live) return;
    const uint32_t bin = dmx_verdict(s, prm.n_bins, prm.min_margin);
    const bool carries = bin < prm.n_bins && holds;
    dmx_write_hit(hit_out + r, mine, carries ? mine + s.p1 : nullptr, lane, G);
    if (lane == 0) {
        bin_out[r] = bin;
        if (pat_out) pat_out[r] = carries ? s.p1 : BG_DMX_IGNORE;
    }
}

int assign_check(const bg_ctx* ctx, uint64_t n, const bg_demux_params_t* p, const void* hits, uint32_t n_pat, const uint32_t* pat_bin,
                 const void* bin, const void* hit_out) {
    if (!p) return bg_refuse("bg_fastq_demux_assign: null params");
    const uint32_t known = BG_DMX_ANCHOR_5P | BG_DMX_ANCHOR_3P | BG_DMX_PAIRED | BG_DMX_MATE1 | BG_DMX_MATE2;
    if (p->flags & ~known) return bg_refuse("bg_fastq_demux_assign: unknown flag bits");
    if ((p->flags & BG_DMX_ANCHOR_5P) && (p->flags & BG_DMX_ANCHOR_3P)) return bg_refuse("bg_fastq_demux_assign: both ANCHOR flags");
    if ((p->flags & (BG_DMX_MATE1 | BG_DMX_MATE2)) && !(p->flags & BG_DMX_PAIRED)) return bg_refuse("bg_fastq_demux_assign: a MATE flag without PAIRED");
    if ((p->flags & BG_DMX_PAIRED) && (n & 1)) return bg_refuse("bg_fastq_demux_assign: PAIRED with an odd record count");
    if (p->n_bins == 0) return bg_refuse("bg_fastq_demux_assign: n_bins 0");
    if (p->n_bins > BG_DMX_MAX_BINS) return bg_refuse("bg_fastq_demux_assign: n_bins above BG_DMX_MAX_BINS", BG_ERR_TOO_LARGE);
    if (n_pat == 0) return bg_refuse("bg_fastq_demux_assign: n_pat 0");
    if (n_pat > BG_MYERS_MAX_PATTERNS) return bg_refuse("bg_fastq_demux_assign: n_pat above BG_MYERS_MAX_PATTERNS", BG_ERR_TOO_LARGE);
    if (!pat_bin) return bg_refuse("bg_fastq_demux_assign: null pat_bin");
    for (uint32_t q = 0; q < n_pat; q++)
        if (pat_bin[q] >= p->n_bins && pat_bin[q] != BG_DMX_IGNORE) return bg_refuse("bg_fastq_demux_assign: a pat_bin entry names no bin");
    if (n && (!hits || !bin || !hit_out)) return bg_refuse("bg_fastq_demux_assign: null hits, bin or hit_out");
    if (!ctx) return bg_refuse("bg_fastq_demux_assign: null ctx");
    return BG_OK;
}

// ---- split --------------------------------------------------------------------------------------------------------------
constexpr uint32_t kGroups = BG_DMX_MAX_BINS + 2;

// count[g * n_tiles + t]: records of tile t in group g
__global__ __launch_bounds__(256) void dmx_hist_kernel(uint64_t n, uint32_t n_bins, uint32_t n_tiles, const uint32_t* __restrict__ bin,
                                                       uint32_t* __restrict__ count) {
    __shared__ uint32_t s_cnt[kGroups];
    const uint32_t ng = n_bins + 2;
    for (uint32_t g = threadIdx.x; g < ng; g += 256) s_cnt[g] = 0;
    __syncthreads();
    for (uint32_t i = 0; i < DMX_TILE / 256; i++) {
        const uint64_t r = (uint64_t)blockIdx.x * DMX_TILE + i * 256 + threadIdx.x;
        if (r < n) atomicAdd(&s_cnt[dmx_group(bin[r], n_bins)], 1u);
    }
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < ng; g += 256) count[(uint64_t)g * n_tiles + blockIdx.x] = s_cnt[g];
}

// base[g * n_tiles + t]: the scanned table.  A record's place is its (group, tile) base, plus the records of its group in the
// wavefronts before its own, plus those in the earlier steps of its own wavefront, plus the earlier lanes of its step.
__global__ __launch_bounds__(256) void dmx_rank_kernel(uint64_t n, uint32_t n_bins, uint32_t n_bits, uint32_t n_tiles,
                                                       const uint32_t* __restrict__ bin, const uint64_t* __restrict__ base,
                                                       const uint64_t* __restrict__ seq_off, const uint64_t* __restrict__ qual_off,
                                                       uint64_t* __restrict__ perm, uint32_t* __restrict__ sl_out, uint32_t* __restrict__ ql_out) {
    __shared__ uint32_t s_w[DMX_WAVES][kGroups];
    const uint32_t ng = n_bins + 2, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t g = threadIdx.x; g < ng; g += 256)
        for (uint32_t w = 0; w < DMX_WAVES; w++) s_w[w][g] = 0;
    __syncthreads();
    uint32_t grp[DMX_STEPS];
#pragma unroll
    for (uint32_t i = 0; i < DMX_STEPS; i++) {
        const uint64_t r = dmx_item(blockIdx.x, wave, i, lane);
        grp[i] = r < n ? dmx_group(bin[r], n_bins) : 0;
        if (r < n) atomicAdd(&s_w[wave][grp[i]], 1u);
    }
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < ng; g += 256) {
        uint32_t run = 0;
        for (uint32_t w = 0; w < DMX_WAVES; w++) {
            const uint32_t c = s_w[w][g];
            s_w[w][g] = run;
            run += c;
        }
    }
    __syncthreads();
    volatile uint32_t* mine = s_w[wave];
#pragma unroll
    for (uint32_t i = 0; i < DMX_STEPS; i++) {
        const uint64_t r = dmx_item(blockIdx.x, wave, i, lane);
        const bool live = r < n;
        const uint32_t g = grp[i];
        uint64_t peers = __ballot(live);
        for (uint32_t b = 0; b < n_bits; b++) {
            const uint32_t bit = live ? (g >> b) & 1u : 0u;
            peers = dmx_narrow(peers, __ballot(bit), bit);
        }
        const uint32_t below = dmx_rank_below(peers, lane);
        const uint32_t before = live ? mine[g] : 0;
        __builtin_amdgcn_wave_barrier();
        if (live && below == 0) mine[g] = before + dmx_peer_count(peers);
        __builtin_amdgcn_wave_barrier();
        if (live) {
            const uint64_t k = base[(uint64_t)g * n_tiles + blockIdx.x] + before + below;
            perm[k] = r;
            sl_out[k] = (uint32_t)(seq_off[r + 1] - seq_off[r]);
            ql_out[k] = (uint32_t)(qual_off[r + 1] - qual_off[r]);
        }
    }
}

// bin_off[g] = base[g * n_tiles] for the n_bins + 2 groups, and the closing n (the scan's total)
__global__ __launch_bounds__(256) void dmx_bin_off_kernel(uint32_t ng, uint32_t n_tiles, const uint64_t* __restrict__ base,
                                                          uint64_t* __restrict__ bin_off) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g <= ng) bin_off[g] = base[(uint64_t)g * n_tiles];
}

// 16 lanes per output record k = perm's index.  seq_off_out / qual_off_out hold the scans' n + 1 offsets; fq_copy_record
// writes entry k again, with the value it was given from there.
__global__ __launch_bounds__(256) void dmx_copy_kernel(uint64_t n, const uint64_t* __restrict__ perm, const bg_fastq_record_t* __restrict__ recs,
                                                       const uint8_t* __restrict__ seq, const uint64_t* __restrict__ seq_off,
                                                       const uint8_t* __restrict__ qual, const uint64_t* __restrict__ qual_off,
                                                       const bg_alignment_t* __restrict__ hit, bg_fastq_record_t* __restrict__ recs_out,
                                                       uint8_t* __restrict__ seq_out, uint64_t* seq_off_out, uint8_t* __restrict__ qual_out,
                                                       uint64_t* qual_off_out, bg_alignment_t* __restrict__ hit_out) {
    const uint64_t k = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const uint32_t lane = threadIdx.x & 15;
    if (k >= n) return;
    const uint64_t r = perm[k];
    const uint64_t s0 = seq_off[r], q0 = qual_off[r];
    fq_copy_record(recs[r], seq + s0, (uint32_t)(seq_off[r + 1] - s0), qual + q0, (uint32_t)(qual_off[r + 1] - q0), k, seq_off_out[k],
                   qual_off_out[k], recs_out, seq_out, seq_off_out, qual_out, qual_off_out, lane, 16);
    if (hit_out) ((uint32_t*)(hit_out + k))[lane] = ((const uint32_t*)(hit + r))[lane];
}

int split_check(const bg_ctx* ctx, uint64_t n, uint32_t n_bins, const void* bin, const void* hit, const fq_cols_in& in, const fq_cols_out& out,
                const void* hit_out, const void* bin_off) {
    if (n_bins == 0) return bg_refuse("bg_fastq_demux_split: n_bins 0");
    if (n_bins > BG_DMX_MAX_BINS) return bg_refuse("bg_fastq_demux_split: n_bins above BG_DMX_MAX_BINS", BG_ERR_TOO_LARGE);
    if (!bin_off) return bg_refuse("bg_fastq_demux_split: null bin_off");
    if (!out.offsets()) return bg_refuse("bg_fastq_demux_split: null output offsets");
    if (hit_out && !hit) return bg_refuse("bg_fastq_demux_split: hit_out without hit");
    if (n && (!bin || !in.complete() || !out.data())) return bg_refuse("bg_fastq_demux_split: null bin or column");
    if (!ctx) return bg_refuse("bg_fastq_demux_split: null ctx");
    return BG_OK;
}

}  // namespace

extern "C" int bg_fastq_demux_assign_dev(bg_ctx* ctx, uint64_t n, const bg_demux_params_t* params, const bg_alignment_t* d_hits, uint32_t n_pat,
                                         const uint32_t* pat_bin, uint32_t* d_bin, bg_alignment_t* d_hit_out, uint32_t* d_pat_out,
                                         void* stream) {
    if (int rc = assign_check(ctx, n, params, d_hits, n_pat, pat_bin, d_bin, d_hit_out)) return rc;
    if (n == 0) return BG_OK;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    dmx_bins bins;
    for (uint32_t p = 0; p < n_pat; p++) bins.b[p] = pat_bin[p] == BG_DMX_IGNORE ? (uint16_t)DMX_BIN_IGNORE : (uint16_t)pat_bin[p];
    std::fill(bins.b + n_pat, bins.b + BG_MYERS_MAX_PATTERNS, (uint16_t)DMX_BIN_IGNORE);
    if (n_pat >= 16)
        dmx_assign_kernel<16><<<dim3((uint32_t)((n * 16 + 255) / 256)), dim3(256), 0, st>>>(n, *params, d_hits, n_pat, bins, d_bin, d_hit_out,
                                                                                            d_pat_out);
    else
        dmx_assign_kernel<1><<<dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st>>>(n, *params, d_hits, n_pat, bins, d_bin, d_hit_out, d_pat_out);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

extern "C" int bg_fastq_demux_assign(bg_ctx* ctx, uint64_t n, const bg_demux_params_t* params, const bg_alignment_t* hits, uint32_t n_pat,
                                     const uint32_t* pat_bin, uint32_t* bin, bg_alignment_t* hit_out, uint32_t* pat_out) {
    if (int rc = assign_check(ctx, n, params, hits, n_pat, pat_bin, bin, hit_out)) return rc;
    if (n == 0) return BG_OK;
    bg_stage s(ctx, ctx->stream);
    const bg_alignment_t* d_hits = s.up(hits, (size_t)n * n_pat);
    uint32_t* d_bin = s.out<uint32_t>(n);
    bg_alignment_t* d_hit_out = s.out<bg_alignment_t>(n);
    uint32_t* d_pat = pat_out ? s.out<uint32_t>(n) : nullptr;
    if (s.sync()) return s.rc;
    if (int rc = bg_fastq_demux_assign_dev(ctx, n, params, d_hits, n_pat, pat_bin, d_bin, d_hit_out, d_pat, s.st)) return rc;
    s.down(bin, d_bin, n);
    s.down(hit_out, d_hit_out, n);
    if (pat_out) s.down(pat_out, d_pat, n);
    return s.sync();
}

extern "C" int bg_fastq_demux_split_dev(bg_ctx* ctx, uint64_t n, uint32_t n_bins, const uint32_t* d_bin, const bg_alignment_t* d_hit,
                                        const bg_fastq_record_t* d_recs, const uint8_t* d_seq, const uint64_t* d_seq_off, const uint8_t* d_qual,
                                        const uint64_t* d_qual_off, bg_fastq_record_t* d_recs_out, uint8_t* d_seq_out, uint64_t* d_seq_off_out,
                                        uint8_t* d_qual_out, uint64_t* d_qual_off_out, bg_alignment_t* d_hit_out, uint64_t* d_perm,
                                        uint64_t* d_bin_off, uint64_t* bin_off_host, void* stream) {
    if (int rc = split_check(ctx, n, n_bins, d_bin, d_hit, {d_recs, d_seq, d_seq_off, d_qual, d_qual_off},
                             {d_recs_out, d_seq_out, d_seq_off_out, d_qual_out, d_qual_off_out}, d_hit_out, d_bin_off))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    const uint32_t ng = n_bins + 2;
    if (n == 0) {
        BG_HIP(hipMemsetAsync(d_bin_off, 0, (size_t)(ng + 1) * 8, st));
        BG_HIP(hipMemsetAsync(d_seq_off_out, 0, 8, st));
        BG_HIP(hipMemsetAsync(d_qual_off_out, 0, 8, st));
        if (bin_off_host) std::fill(bin_off_host, bin_off_host + ng + 1, (uint64_t)0);
        return BG_OK;
    }
    bg_scratch_guard guard(ctx, st);
    // aux: the scanned (group, tile) table and perm (unless the caller takes it), the block sums of the three scans, then the
    // table's counts and the two length columns at their places
    const uint32_t n_tiles = (uint32_t)((n + DMX_TILE - 1) / DMX_TILE);
    const size_t cells = (size_t)ng * n_tiles, t_sums = bg_scan_sums_words(cells), r_sums = bg_scan_sums_words(n);
    uint64_t *d_base, *perm, *d_sums;
    uint32_t *d_count, *d_sl, *d_ql;
    if (int rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_base = cv.take<uint64_t>(cells + 1);
        perm = d_perm ? d_perm : cv.take<uint64_t>(n);
        d_sums = cv.take<uint64_t>(t_sums + 2 * r_sums);
        d_count = cv.take<uint32_t>(cells), d_sl = cv.take<uint32_t>(n), d_ql = cv.take<uint32_t>(n);
    })) return rc;
    dmx_hist_kernel<<<dim3(n_tiles), dim3(256), 0, st>>>(n, n_bins, n_tiles, d_bin, d_count);
    BG_HIP(hipGetLastError());
    if (int rc = bg_scan_u32(d_count, cells, d_base, d_sums, st)) return rc;
    dmx_rank_kernel<<<dim3(n_tiles), dim3(256), 0, st>>>(n, n_bins, dmx_group_bits(n_bins), n_tiles, d_bin, d_base, d_seq_off, d_qual_off, perm,
                                                         d_sl, d_ql);
    dmx_bin_off_kernel<<<dim3((ng + 256) / 256), dim3(256), 0, st>>>(ng, n_tiles, d_base, d_bin_off);
    BG_HIP(hipGetLastError());
    if (int rc = bg_scan_u32(d_sl, n, d_seq_off_out, d_sums + t_sums, st)) return rc;
    if (int rc = bg_scan_u32(d_ql, n, d_qual_off_out, d_sums + t_sums + r_sums, st)) return rc;
    dmx_copy_kernel<<<dim3((uint32_t)((n * 16 + 255) / 256)), dim3(256), 0, st>>>(n, perm, d_recs, d_seq, d_seq_off, d_qual, d_qual_off, d_hit,
                                                                                  d_recs_out, d_seq_out, d_seq_off_out, d_qual_out,
                                                                                  d_qual_off_out, d_hit_out);
    BG_HIP(hipGetLastError());
    if (bin_off_host) {
        BG_HIP(hipMemcpyAsync(bin_off_host, d_bin_off, (size_t)(ng + 1) * 8, hipMemcpyDeviceToHost, st));
        BG_HIP(hipStreamSynchronize(st));
    }
    return BG_OK;
}

extern "C" int bg_fastq_demux_split(bg_ctx* ctx, uint64_t n, uint32_t n_bins, const uint32_t* bin, const bg_alignment_t* hit,
                                    const bg_fastq_record_t* recs, const uint8_t* seq, const uint64_t* seq_off, const uint8_t* qual,
                                    const uint64_t* qual_off, bg_fastq_record_t* recs_out, uint8_t* seq_out, uint64_t* seq_off_out,
                                    uint8_t* qual_out, uint64_t* qual_off_out, bg_alignment_t* hit_out, uint64_t* perm, uint64_t* bin_off) {
    const fq_cols_in in = {recs, seq, seq_off, qual, qual_off};
    const fq_cols_out out = {recs_out, seq_out, seq_off_out, qual_out, qual_off_out};
    if (int rc = split_check(ctx, n, n_bins, bin, hit, in, out, hit_out, bin_off)) return rc;
    const uint64_t sb = n ? seq_off[n] : 0, qb = n ? qual_off[n] : 0;
    bg_stage s(ctx, ctx->stream);
    const uint32_t* d_bin = s.up(bin, n);
    const bg_alignment_t* d_hit = hit ? s.up(hit, n) : nullptr;
    const fq_cols_in d = fq_cols_upload(s, n, in);
    const fq_cols_out o = fq_cols_alloc(s, n, sb, qb);
    bg_alignment_t* d_hit_out = hit_out ? s.out<bg_alignment_t>(n) : nullptr;
    uint64_t* d_perm = s.out<uint64_t>(n);
    uint64_t* d_bin_off = s.out<uint64_t>((size_t)n_bins + 3);
    if (s.sync()) return s.rc;
    if (int rc = bg_fastq_demux_split_dev(ctx, n, n_bins, d_bin, d_hit, d.recs, d.seq, d.seq_off, d.qual, d.qual_off, o.recs, o.seq, o.seq_off,
                                          o.qual, o.qual_off, d_hit_out, d_perm, d_bin_off, bin_off, s.st))
        return rc;
    fq_cols_download(s, out, o, n, sb, qb);
    if (hit_out) s.down(hit_out, d_hit_out, n);
    if (perm) s.down(perm, d_perm, n);
    return s.sync();
}
