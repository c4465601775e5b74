// Coordinate-sorted SAM and duplicate marking (bg_sam_markdup[_dev], bg_sam_sort_keys[_dev], bg_sam_sort[_dev]; the rules are in
// include/biogpu.h, their bodies in sam_rule.h).
//
// markdup.  A score per read (16 lanes a read sum its qualities), then one 48-byte entry per read and, with pairs, one per pair
// (md_end_entry, md_pair_entry).  The entries are ordered by md_less, which is a TOTAL order — group, then score descending,
// then index — so a group's winner is simply the first entry of its run and nothing depends on how the sort treats equal
// elements: there are none.  rocPRIM's merge sort orders indices with md_less as its comparison; the entries are gathered
// into that order and one pass flags every entry whose predecessor is of its group.  In the sort over ends the ends of
// both-ended pairs stand in front of the fragments of the same end, so a fragment behind one is flagged by the same test.
//
// sort.  rocPRIM's stable radix sort of (key, index) gives perm; the permuted lengths are scanned into out_off; the copy
// gives every line of up to kLongLine bytes a group of 16 lanes and every longer one (a 65 535-base read makes a line of more
// than 130 KB) a column of blocks that take 4 KB of it at a time.  Either way the line leaves in 16-byte stores aligned to
// the DESTINATION; a store's 16 bytes are put together from the two source granules they straddle (sam_copy_vec), and only
// a line's first and last vectors fall back to byte loads, so that no byte outside the line is read.
#include <algorithm>

#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "fastq_cols.h"
#include "sam_rule.h"

namespace {

constexpr uint64_t kLongLine = SAM_LONG_LINE;    // bytes: a longer line goes to the block kernel
constexpr uint32_t kChunkVecs = SAM_CHUNK_VECS;  // 16-byte vectors of a long line a block takes at a time
constexpr uint32_t kLongCols = 32, kLongRows = 256;  // the block kernel's grid: chunks of a line x lines

__device__ __forceinline__ void count_votes(bool vote, uint64_t* cell, uint64_t weight) {
    const uint64_t m = __ballot(vote);
    if (m && (threadIdx.x & 63) == (uint32_t)(__ffsll((unsigned long long)m) - 1)) atomicAdd((unsigned long long*)cell, (unsigned long long)(__popcll(m) * weight));
}

// ---- markdup --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void md_score_kernel(uint64_t n, const bg_fastq_record_t* __restrict__ recs, const uint8_t* __restrict__ qual,
                                                       uint32_t phred_offset, uint32_t min_qual, uint32_t* __restrict__ score) {
    const uint64_t r = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / MD_G;
    const uint32_t lane = threadIdx.x % MD_G;
    uint32_t s = 0;
    if (r < n) s = md_score_share(qual + recs[r].qual_off, recs[r].qual_len, phred_offset, min_qual, lane, MD_G);
    for (uint32_t o = MD_G / 2; o; o >>= 1) s += __shfl_xor(s, o, MD_G);
    if (r < n && lane == 0) score[r] = s;
}

__global__ __launch_bounds__(256) void md_entry_kernel(uint64_t n, uint32_t K, bool paired, const bg_sam_contig_t* __restrict__ contigs,
                                                       uint64_t n_contigs, const bg_seed_hit_t* __restrict__ hits, const uint8_t* __restrict__ strand,
                                                       const uint32_t* __restrict__ score, md_entry_t* __restrict__ ends,
                                                       md_entry_t* __restrict__ pairs, uint64_t* __restrict__ counts) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool has_end = false;
    if (r < n) {
        const md_end_t e = md_end(contigs, n_contigs, hits[r * K], strand[r * K]);
        has_end = e.contig >= 0;
        uint32_t kind = MD_KIND_FRAGMENT;
        if (paired) {  // K == 1
            const uint64_t m = r ^ 1;
            const md_end_t em = md_end(contigs, n_contigs, hits[m], strand[m]);
            if (has_end && em.contig >= 0) kind = MD_KIND_PAIR_END;
            if (!(r & 1)) pairs[r >> 1] = md_pair_entry(e, em, score[r], score[m], r >> 1);
        }
        ends[r] = md_end_entry(e, kind, score[r], r);
    }
    count_votes(has_end, counts + 0, 1);
}

struct MdOrder {
    const md_entry_t* e;
    __device__ bool operator()(uint64_t a, uint64_t b) const { return md_less(e[a], e[b]); }
};

__global__ __launch_bounds__(256) void md_gather_kernel(uint64_t n, const md_entry_t* __restrict__ e, const uint64_t* __restrict__ order,
                                                        md_entry_t* __restrict__ sorted) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) sorted[i] = e[order[i]];
}

// the pass over runs; words = 4: the entries are pairs, words = 2: ends
__global__ __launch_bounds__(256) void md_run_kernel(uint64_t n, const md_entry_t* __restrict__ sorted, int words, bool paired,
                                                     uint8_t* __restrict__ dup, uint64_t* __restrict__ counts) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool flagged = i < n && md_flagged(sorted, i, words);
    bool by_pair = false;
    if (flagged) {
        const uint64_t idx = sorted[i].idx;
        if (words == 4) {
            dup[2 * idx] = 1;
            dup[2 * idx + 1] = 1;
        } else {
            dup[idx] = 1;
            by_pair = paired && md_group_has_pair_end(sorted, i);
        }
    }
    count_votes(flagged, counts + 1, words == 4 ? 2 : 1);
    if (words == 4) count_votes(flagged, counts + 2, 1);
    else count_votes(by_pair, counts + 3, 1);
}

// ---- keys -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sam_key_kernel(uint64_t n_slots, uint32_t flags, uint32_t K, const bg_sam_contig_t* __restrict__ contigs,
                                                      uint64_t n_contigs, const bg_seed_hit_t* __restrict__ hits, const uint8_t* __restrict__ strand,
                                                      uint64_t* __restrict__ key) {
    const uint64_t slot = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (slot < n_slots) key[slot] = sam_rule_key(flags, K, contigs, n_contigs, hits, strand, slot);
}

// ---- sort -----------------------------------------------------------------------------------------------------------------
// len[j] = length of record perm[j] (len[n] = 0: the scan's last entry is the total); the long lines are listed
__global__ __launch_bounds__(256) void sort_len_kernel(uint64_t n, const uint64_t* __restrict__ perm, const uint64_t* __restrict__ in_off,
                                                       uint64_t* __restrict__ len, uint64_t* __restrict__ long_list, uint64_t* __restrict__ n_long) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j > n) return;
    uint64_t l = 0;
    if (j < n) {
        const uint64_t i = perm[j];
        l = in_off[i + 1] - in_off[i];
        if (l > kLongLine) long_list[atomicAdd((unsigned long long*)n_long, 1ull)] = j;
    }
    len[j] = l;
}

// 16 lanes a line, 16 lines a block
__global__ __launch_bounds__(256) void sort_copy_kernel(uint64_t n, const uint64_t* __restrict__ perm, const uint64_t* __restrict__ in_off,
                                                        const uint64_t* __restrict__ out_off, const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * (256 / SAM_COPY_G) + threadIdx.x / SAM_COPY_G;
    if (j >= n) return;
    const uint64_t i = perm[j], s = in_off[i], len = in_off[i + 1] - s;
    if (len == 0 || len > kLongLine) return;
    sam_copy_line(in + s, out + out_off[j], len, threadIdx.x % SAM_COPY_G, SAM_COPY_G, 0, UINT64_MAX, true);
}

// long lines: block (c, y) takes chunks c, c + kLongCols, ... of the listed lines y, y + kLongRows, ...
__global__ __launch_bounds__(256) void sort_copy_long_kernel(const uint64_t* __restrict__ long_list, const uint64_t* __restrict__ n_long,
                                                             const uint64_t* __restrict__ perm, const uint64_t* __restrict__ in_off,
                                                             const uint64_t* __restrict__ out_off, const uint8_t* __restrict__ in,
                                                             uint8_t* __restrict__ out) {
    const uint64_t count = *n_long;
    for (uint64_t y = blockIdx.y; y < count; y += kLongRows) {
        const uint64_t j = long_list[y], i = perm[j], s = in_off[i], len = in_off[i + 1] - s;
        const uint64_t vecs = len >> 4;  // at least the plan's body
        for (uint64_t c = blockIdx.x; c * kChunkVecs <= vecs; c += kLongCols)
            sam_copy_line(in + s, out + out_off[j], len, threadIdx.x, 256, c * kChunkVecs, (c + 1) * kChunkVecs, c == 0);
    }
}

int md_check(const bg_ctx* ctx, const bg_markdup_params_t* mp, uint64_t n_reads, uint64_t n_contigs) {
    if (!ctx || !mp) return BG_ERR_INVALID_ARG;
    if (mp->flags & ~(uint32_t)BG_SAM_PAIRED) return BG_ERR_INVALID_ARG;
    if (mp->max_hits == 0 || mp->max_hits > BG_SEED_MAX_HITS || n_contigs == 0) return BG_ERR_INVALID_ARG;
    if ((mp->flags & BG_SAM_PAIRED) && ((n_reads & 1) || mp->max_hits != 1)) return BG_ERR_INVALID_ARG;
    return BG_OK;
}

int key_check(const bg_ctx* ctx, const bg_sam_params_t* sp, uint64_t n_reads, uint64_t n_contigs) {
    if (!ctx || !sp) return BG_ERR_INVALID_ARG;
    if (sp->flags & ~(uint32_t)(BG_SAM_PAIRED | BG_SAM_SECONDARY | BG_SAM_TAG_NM | BG_SAM_TAG_MD)) return BG_ERR_INVALID_ARG;
    if (sp->max_hits == 0 || sp->max_hits > BG_SEED_MAX_HITS || n_contigs == 0) return BG_ERR_INVALID_ARG;
    if ((sp->flags & BG_SAM_PAIRED) && ((n_reads & 1) || sp->max_hits != 1)) return BG_ERR_INVALID_ARG;
    return BG_OK;
}

int sort_check(const bg_ctx* ctx, uint64_t n_slots, const void* key, const void* in, const void* in_off, uint64_t in_bytes, const void* out,
               uint64_t out_cap, const void* out_off, const void* perm) {
    if (!ctx || !out_off || !perm) return BG_ERR_INVALID_ARG;
    if (n_slots && (!key || !in_off)) return BG_ERR_INVALID_ARG;
    if (in_bytes && (!in || !out)) return BG_ERR_INVALID_ARG;
    if (out_cap < in_bytes) return BG_ERR_OPS_CAP;
    return BG_OK;
}

inline uint32_t blocks_of(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

}  // namespace

extern "C" int bg_sam_markdup_dev(bg_ctx* ctx, const bg_markdup_params_t* mp, uint64_t n_reads, const bg_sam_contig_t* d_contigs,
                                  uint64_t n_contigs, const bg_seed_hit_t* d_hits, const uint8_t* d_strand, const bg_fastq_record_t* d_recs,
                                  const uint8_t* d_qual, uint8_t* d_dup, uint64_t* counts, void* stream) {
    if (!counts) return BG_ERR_INVALID_ARG;
    int rc = md_check(ctx, mp, n_reads, n_contigs);
    if (rc) return rc;
    if (n_reads && (!d_contigs || !d_hits || !d_strand || !d_recs || !d_qual || !d_dup)) return BG_ERR_INVALID_ARG;
    for (int i = 0; i < 4; i++) counts[i] = 0;
    if (n_reads == 0) return BG_OK;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);
    const bool paired = (mp->flags & BG_SAM_PAIRED) != 0;
    const uint64_t n = n_reads, np = paired ? n / 2 : 0;
    size_t t_ends = 0, t_pairs = 0;
    const rocprim::counting_iterator<uint64_t> iota(0);
    BG_HIP(rocprim::merge_sort(nullptr, t_ends, iota, (uint64_t*)nullptr, n, MdOrder{nullptr}, st));
    if (np) BG_HIP(rocprim::merge_sort(nullptr, t_pairs, iota, (uint64_t*)nullptr, np, MdOrder{nullptr}, st));
    uint64_t *d_counts, *d_order;
    uint32_t* d_score;
    md_entry_t *d_ends, *d_pairs, *d_sorted;
    uint8_t* d_tmp;
    if ((rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_counts = cv.take<uint64_t>(4);
        d_score = cv.take<uint32_t>(n);
        d_ends = cv.take<md_entry_t>(n), d_pairs = cv.take<md_entry_t>(np);
        d_order = cv.take<uint64_t>(n), d_sorted = cv.take<md_entry_t>(n);
        d_tmp = cv.take<uint8_t>(std::max(t_ends, t_pairs));
    }))) return rc;
    BG_HIP(hipMemsetAsync(d_counts, 0, 4 * 8, st));
    BG_HIP(hipMemsetAsync(d_dup, 0, n, st));
    md_score_kernel<<<dim3(blocks_of(n, 256 / MD_G)), dim3(256), 0, st>>>(n, d_recs, d_qual, mp->phred_offset, mp->min_qual, d_score);
    md_entry_kernel<<<dim3(blocks_of(n, 256)), dim3(256), 0, st>>>(n, mp->max_hits, paired, d_contigs, n_contigs, d_hits, d_strand, d_score, d_ends,
                                                                   d_pairs, d_counts);
    BG_HIP(hipGetLastError());
    if (np) {
        size_t t = t_pairs;
        BG_HIP(rocprim::merge_sort(d_tmp, t, iota, d_order, np, MdOrder{d_pairs}, st));
        md_gather_kernel<<<dim3(blocks_of(np, 256)), dim3(256), 0, st>>>(np, d_pairs, d_order, d_sorted);
        md_run_kernel<<<dim3(blocks_of(np, 256)), dim3(256), 0, st>>>(np, d_sorted, 4, paired, d_dup, d_counts);
        BG_HIP(hipGetLastError());
    }
    size_t t = t_ends;
    BG_HIP(rocprim::merge_sort(d_tmp, t, iota, d_order, n, MdOrder{d_ends}, st));
    md_gather_kernel<<<dim3(blocks_of(n, 256)), dim3(256), 0, st>>>(n, d_ends, d_order, d_sorted);
    md_run_kernel<<<dim3(blocks_of(n, 256)), dim3(256), 0, st>>>(n, d_sorted, 2, paired, d_dup, d_counts);
    BG_HIP(hipGetLastError());
    BG_HIP(hipMemcpyAsync(counts, d_counts, 4 * 8, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    return BG_OK;
}

extern "C" int bg_sam_markdup(bg_ctx* ctx, const bg_markdup_params_t* mp, uint64_t n_reads, const bg_sam_contig_t* contigs, uint64_t n_contigs,
                              const bg_seed_hit_t* hits, const uint8_t* strand, const bg_fastq_record_t* recs, const uint8_t* qual, uint8_t* dup,
                              uint64_t* counts) {
    if (!counts) return BG_ERR_INVALID_ARG;
    int rc = md_check(ctx, mp, n_reads, n_contigs);
    if (rc) return rc;
    if (n_reads && (!contigs || !hits || !strand || !recs || !qual || !dup)) return BG_ERR_INVALID_ARG;
    for (int i = 0; i < 4; i++) counts[i] = 0;
    if (n_reads == 0) return BG_OK;
    const uint64_t n_slots = n_reads * mp->max_hits;
    bg_stage s(ctx, ctx->stream);
    const bg_sam_contig_t* d_contigs = s.up(contigs, n_contigs);
    const bg_seed_hit_t* d_hits = s.up(hits, n_slots);
    const uint8_t* d_strand = s.up(strand, n_slots);
    const bg_fastq_record_t* d_recs = s.up(recs, n_reads);
    const uint8_t* d_qual = s.up(qual, fq_record_extents(recs, n_reads).qual);  // of the records' buffers only the qualities are read
    uint8_t* d_dup = s.out<uint8_t>(n_reads);
    if (s.rc) return s.rc;
    if ((rc = bg_sam_markdup_dev(ctx, mp, n_reads, d_contigs, n_contigs, d_hits, d_strand, d_recs, d_qual, d_dup, counts, s.st))) return rc;
    s.down(dup, d_dup, n_reads);
    return s.sync();
}

extern "C" int bg_sam_sort_keys_dev(bg_ctx* ctx, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* d_contigs, uint64_t n_contigs,
                                    const bg_seed_hit_t* d_hits, const uint8_t* d_strand, uint64_t* d_key, void* stream) {
    int rc = key_check(ctx, sp, n_reads, n_contigs);
    if (rc) return rc;
    if (n_reads && (!d_contigs || !d_hits || !d_strand || !d_key)) return BG_ERR_INVALID_ARG;
    if (n_reads == 0) return BG_OK;
    BG_HIP(hipSetDevice(ctx->device));
    const uint64_t n_slots = n_reads * sp->max_hits;
    sam_key_kernel<<<dim3(blocks_of(n_slots, 256)), dim3(256), 0, (hipStream_t)stream>>>(n_slots, sp->flags, sp->max_hits, d_contigs, n_contigs, d_hits,
                                                                                        d_strand, d_key);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

extern "C" int bg_sam_sort_keys(bg_ctx* ctx, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* contigs, uint64_t n_contigs,
                                const bg_seed_hit_t* hits, const uint8_t* strand, uint64_t* key) {
    int rc = key_check(ctx, sp, n_reads, n_contigs);
    if (rc) return rc;
    if (n_reads && (!contigs || !hits || !strand || !key)) return BG_ERR_INVALID_ARG;
    if (n_reads == 0) return BG_OK;
    const uint64_t n_slots = n_reads * sp->max_hits;
    bg_stage s(ctx, ctx->stream);
    const bg_sam_contig_t* d_contigs = s.up(contigs, n_contigs);
    const bg_seed_hit_t* d_hits = s.up(hits, n_slots);
    const uint8_t* d_strand = s.up(strand, n_slots);
    uint64_t* d_key = s.out<uint64_t>(n_slots);
    if (s.rc) return s.rc;
    if ((rc = bg_sam_sort_keys_dev(ctx, sp, n_reads, d_contigs, n_contigs, d_hits, d_strand, d_key, s.st))) return rc;
    s.down(key, d_key, n_slots);
    return s.sync();
}

extern "C" int bg_sam_sort_dev(bg_ctx* ctx, uint64_t n_slots, const uint64_t* d_key, const char* d_in, const uint64_t* d_in_off, uint64_t in_bytes,
                               char* d_out, uint64_t out_cap, uint64_t* d_out_off, uint64_t* d_perm, void* stream) {
    int rc = sort_check(ctx, n_slots, d_key, d_in, d_in_off, in_bytes, d_out, out_cap, d_out_off, d_perm);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    if (n_slots == 0) {
        BG_HIP(hipMemsetAsync(d_out_off, 0, 8, st));
        return BG_OK;
    }
    bg_scratch_guard guard(ctx, st);
    const uint64_t n = n_slots;
    const rocprim::counting_iterator<uint64_t> iota(0);
    size_t t_sort = 0, t_scan = 0;
    BG_HIP(rocprim::radix_sort_pairs(nullptr, t_sort, d_key, (uint64_t*)nullptr, iota, d_perm, n, 0, 64, st));
    BG_HIP(rocprim::exclusive_scan(nullptr, t_scan, (uint64_t*)nullptr, d_out_off, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), st));
    uint64_t *d_keys_out, *d_len, *d_list, *d_count;
    uint8_t* d_tmp;
    if ((rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_keys_out = cv.take<uint64_t>(n), d_len = cv.take<uint64_t>(n + 1), d_list = cv.take<uint64_t>(n), d_count = cv.take<uint64_t>(1);
        d_tmp = cv.take<uint8_t>(std::max(t_sort, t_scan));
    }))) return rc;
    hipEvent_t ev[3] = {};
    if (ctx->timing) {
        for (hipEvent_t& e : ev) BG_HIP(hipEventCreate(&e));
        BG_HIP(hipEventRecord(ev[0], st));
    }
    BG_HIP(rocprim::radix_sort_pairs(d_tmp, t_sort, d_key, d_keys_out, iota, d_perm, n, 0, 64, st));
    if (ctx->timing) BG_HIP(hipEventRecord(ev[1], st));
    BG_HIP(hipMemsetAsync(d_count, 0, 8, st));
    sort_len_kernel<<<dim3(blocks_of(n + 1, 256)), dim3(256), 0, st>>>(n, d_perm, d_in_off, d_len, d_list, d_count);
    BG_HIP(hipGetLastError());
    BG_HIP(rocprim::exclusive_scan(d_tmp, t_scan, d_len, d_out_off, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), st));
    if (in_bytes) {
        sort_copy_kernel<<<dim3(blocks_of(n, 256 / SAM_COPY_G)), dim3(256), 0, st>>>(n, d_perm, d_in_off, d_out_off, (const uint8_t*)d_in, (uint8_t*)d_out);
        sort_copy_long_kernel<<<dim3(kLongCols, kLongRows), dim3(256), 0, st>>>(d_list, d_count, d_perm, d_in_off, d_out_off, (const uint8_t*)d_in,
                                                                               (uint8_t*)d_out);
        BG_HIP(hipGetLastError());
    }
    if (ctx->timing) {
        BG_HIP(hipEventRecord(ev[2], st));
        BG_HIP(hipEventSynchronize(ev[2]));
        float sort_ms = 0, copy_ms = 0;
        BG_HIP(hipEventElapsedTime(&sort_ms, ev[0], ev[1]));
        BG_HIP(hipEventElapsedTime(&copy_ms, ev[1], ev[2]));
        ctx->last.fm_ms += sort_ms;
        ctx->last.fm_launches += 1;
        ctx->last.fill_ms += copy_ms;
        ctx->last.fill_launches += 1;
        for (hipEvent_t e : ev) hipEventDestroy(e);
    }
    return BG_OK;
}

extern "C" int bg_sam_sort(bg_ctx* ctx, uint64_t n_slots, const uint64_t* key, const char* in, const uint64_t* in_off, uint64_t in_bytes, char* out,
                           uint64_t out_cap, uint64_t* out_off, uint64_t* perm) {
    int rc = sort_check(ctx, n_slots, key, in, in_off, in_bytes, out, out_cap, out_off, perm);
    if (rc) return rc;
    out_off[0] = 0;
    if (n_slots == 0) return BG_OK;
    bg_stage s(ctx, ctx->stream);
    const uint64_t* d_key = s.up(key, n_slots);
    const char* d_in = s.up(in, in_bytes);
    const uint64_t* d_in_off = s.up(in_off, n_slots + 1);
    char* d_out = s.out<char>(in_bytes);
    uint64_t* d_out_off = s.out<uint64_t>(n_slots + 1);
    uint64_t* d_perm = s.out<uint64_t>(n_slots);
    if (s.rc) return s.rc;
    if ((rc = bg_sam_sort_dev(ctx, n_slots, d_key, d_in, d_in_off, in_bytes, d_out, in_bytes, d_out_off, d_perm, s.st))) return rc;
    s.down(out_off, d_out_off, n_slots + 1);
    s.down(perm, d_perm, n_slots);
    s.down(out, d_out, in_bytes);
    return s.sync();
}
