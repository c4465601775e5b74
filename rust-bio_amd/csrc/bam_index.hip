// The BAI index of a coordinate-sorted stream of BAM records (bg_bam_index[_dev]; THE RULE is in include/biogpu.h, the bodies
// in bam_index_rule.h).  Everything is a pass with one lane per element, a scan or one stable radix sort (rocPRIM):
//   1. the non-empty slots are ranked (a scan), and one lane per slot decodes its record — fixed fields by byte loads, the
//      CIGAR walk for `end`, the checks — into entry rank[slot] of a dense list: the predecessor of record j is j - 1;
//   2. one lane per record compares it with its predecessor: the order check, the head of a run of one (ref, bin), the first
//      and last record of a reference (the sorted input makes references segments).  A scan of the head flags numbers the
//      chunks (the unmapped flags ride in its upper half), a running maximum of (ref, end) is the prefix maximum of `end`
//      inside every reference;
//   3. the chunk list is sorted stably by (ref, bin) — the number of chunks is only known on the device, so the list is
//      padded to n_slots with a key above all others —; bin heads are scanned, the sorted list gives every reference its
//      bins and chunks, a scan over the references' byte counts places them;
//   4. the first error (the minimum over slot << 2 | kind, by an ordinary atomic minimum) and the total are read back once;
//      then the bytes are stored: one lane per chunk, and per reference a row of 8 blocks whose lanes take its windows, each a
//      binary search in the running maximum.  The output is small and may lie anywhere: byte stores.
// Every kernel behind the checks returns at once when an error is recorded, so that nothing indexes with what an unsorted or
// broken input left in the lists.  Scratch is the ctx's: 17 words of 8 bytes a slot and 6 a contig; the linear index goes
// straight to the output, so nothing is proportional to windows, let alone to n_contigs x 37 450.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "bg_common.h"
#include "bam_index_rule.h"

namespace {

struct BaiArgs {
    uint64_t n;  // slots
    const uint8_t* recs;
    const uint64_t* off;
    const bg_sam_contig_t* contigs;
    uint64_t n_contigs;
    const uint64_t* block_off;
    uint64_t base;
    uint64_t n_blocks;        // bg_bam_index_blocks: the rows of block_off and out_off (bg_bgzf_blocks' tables) ...
    const uint64_t* out_off;  // ... null for the two framings of our own
};
struct BaiWork {
    unsigned long long* bad;  // slot << 2 | kind of the first offending slot, BAI_NONE without one
    uint64_t* n_indexed;      // records with refID >= 0: a prefix of the sorted records
    uint64_t* flag;           // [n + 1] input of the scan at hand
    uint64_t* rank;           // [n + 1] non-empty slots in front of a slot; rank[n]: records
    bai_rec_t* rec;           // [n]
    uint64_t* hu;             // [n + 1] scanned: chunk heads in front of a record (low half), unmapped records (high half)
    uint64_t* end_key;        // [n + 1]
    uint64_t* end_max;        // [n + 1] running maximum of end_key
    uint64_t* key;            // [n] (ref, bin) of chunk c
    uint64_t* head_pos;       // [n + 1] the record chunk c starts at; behind the last chunk: n_indexed
    uint64_t* key_sorted;     // [n]
    uint64_t* perm;           // [n] the chunk at place k of the sorted list
    uint64_t* bins_before;    // [n + 1] scanned: bin heads in front of place k
    uint64_t* bin_start;      // [n + 1] the place bin b starts at; behind the last bin: the number of chunks
    uint64_t* ref_first;      // [n_contigs] records [ref_first, ref_end) ...
    uint64_t* ref_end;
    uint64_t* chunk_first;    // ... and places [chunk_first, chunk_end) of the sorted chunk list are a reference's
    uint64_t* chunk_end;
    uint64_t* ref_bytes;      // [n_contigs + 1]
    uint64_t* ref_base;       // [n_contigs + 1] scanned
};

__device__ __forceinline__ void bai_report(const BaiWork& w, uint64_t slot, int kind) { atomicMin(w.bad, (unsigned long long)((slot << 2) | (uint64_t)kind)); }
__device__ __forceinline__ bool bai_failed(const BaiWork& w) { return *w.bad != BAI_NONE; }
__device__ __forceinline__ uint64_t bai_chunks(const BaiWork& w, uint64_t n) { return w.hu[w.rank[n]] & 0xFFFFFFFFull; }

__global__ __launch_bounds__(256) void bai_flag_kernel(const BaiArgs a, const BaiWork w) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > a.n) return;
    uint64_t f = 0;
    if (i < a.n) {
        if (a.off[i + 1] < a.off[i]) bai_report(w, i, BAI_INVALID);
        f = a.off[i + 1] > a.off[i];
    }
    w.flag[i] = f;
}

__global__ __launch_bounds__(256) void bai_decode_kernel(const BaiArgs a, const BaiWork w) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n || !w.flag[i]) return;
    bai_rec_t r;
    r.slot = i;
    const int kind = bai_decode(a.recs + a.off[i], a.off[i + 1] - a.off[i], a.contigs, a.n_contigs, &r);
    if (kind) bai_report(w, i, kind);
    w.rec[w.rank[i]] = r;
}

// one lane per record (and the entries behind the last one, which the scans read)
__global__ __launch_bounds__(256) void bai_link_kernel(const BaiArgs a, const BaiWork w) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j > a.n) return;
    const uint64_t m = w.rank[a.n];
    uint64_t hu = 0, ek = 0;
    if (j < m) {
        const bai_rec_t e = w.rec[j];
        bai_rec_t p = e;
        if (j) p = w.rec[j - 1];
        if (j && bai_before(e, p)) bai_report(w, e.slot, BAI_INVALID);
        const bool placed = e.ref >= 0, last = j + 1 == m;
        const int32_t next_ref = last ? -1 : w.rec[j + 1].ref;
        const bool ref_head = placed && (j == 0 || p.ref != e.ref);
        if (ref_head) w.ref_first[e.ref] = j;
        if (placed && (last || next_ref != e.ref)) w.ref_end[e.ref] = j + 1;
        if (placed && (last || next_ref < 0)) *w.n_indexed = j + 1;
        if (ref_head || (placed && ((p.binf ^ e.binf) & 0xFFFFu))) hu = 1;
        if (placed && (e.binf & BAI_UNMAPPED_BIT)) hu |= 1ull << 32;
        ek = bai_end_key(e);
    }
    w.flag[j] = hu;
    w.end_key[j] = ek;
}

// the chunk list: a key and the first record of every chunk, the padding keys behind them
__global__ __launch_bounds__(256) void bai_chunk_kernel(const BaiArgs a, const BaiWork w) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n || bai_failed(w)) return;
    const uint64_t m = w.rank[a.n], n_chunks = bai_chunks(w, a.n);
    if (j < m && (w.flag[j] & 1)) {
        const uint64_t c = w.hu[j] & 0xFFFFFFFFull;
        w.key[c] = bai_chunk_key(w.rec[j].ref, w.rec[j].binf);
        w.head_pos[c] = j;
    }
    if (j >= n_chunks) w.key[j] = BAI_KEY_PAD;
    if (j == 0) w.head_pos[n_chunks] = *w.n_indexed;
}

// one lane per place of the sorted chunk list: bin heads, and the places of a reference
__global__ __launch_bounds__(256) void bai_bin_kernel(const BaiArgs a, const BaiWork w) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > a.n) return;
    uint64_t head = 0;
    if (!bai_failed(w)) {
        const uint64_t n_chunks = bai_chunks(w, a.n);
        if (k < n_chunks) {
            const uint64_t key = w.key_sorted[k], ref = key >> 16;
            const uint64_t prev = k ? w.key_sorted[k - 1] : 0, next = k + 1 < n_chunks ? w.key_sorted[k + 1] : 0;
            head = k == 0 || prev != key;
            if (k == 0 || prev >> 16 != ref) w.chunk_first[ref] = k;
            if (k + 1 == n_chunks || next >> 16 != ref) w.chunk_end[ref] = k + 1;
        }
    }
    w.flag[k] = head;
}

__global__ __launch_bounds__(256) void bai_bin_start_kernel(const BaiArgs a, const BaiWork w) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > a.n || bai_failed(w)) return;
    const uint64_t n_chunks = bai_chunks(w, a.n);
    if (k < n_chunks ? w.flag[k] != 0 : k == n_chunks) w.bin_start[w.bins_before[k]] = k;
}

struct BaiRef {  // a reference's records, bins, chunks and windows
    uint64_t first, end, chunk_first, n_bins, n_chunks, n_intv;
};
__device__ BaiRef bai_ref(const BaiWork& w, uint64_t r) {
    BaiRef f = {};
    f.first = w.ref_first[r];
    f.end = w.ref_end[r];
    if (f.end <= f.first) return f;
    f.chunk_first = w.chunk_first[r];
    const uint64_t ce = w.chunk_end[r];
    f.n_chunks = ce - f.chunk_first;
    f.n_bins = w.bins_before[ce] - w.bins_before[f.chunk_first];
    f.n_intv = bai_n_intv((uint32_t)w.end_max[f.end - 1]);
    return f;
}

__global__ __launch_bounds__(256) void bai_ref_bytes_kernel(const BaiArgs a, const BaiWork w) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > a.n_contigs) return;
    uint64_t bytes = 0;
    if (r < a.n_contigs && !bai_failed(w)) {
        const BaiRef f = bai_ref(w, r);
        bytes = bai_ref_bytes(f.end > f.first, f.n_bins, f.n_chunks, f.n_intv);
    }
    w.ref_bytes[r] = bytes;
}

// the first error and the total side by side, for one read-back
__global__ void bai_tail_kernel(const BaiArgs a, const BaiWork w, unsigned long long* __restrict__ tail) {
    tail[0] = *w.bad;
    tail[1] = bai_total(w.ref_base[a.n_contigs]);
}

// ---- the bytes ----------------------------------------------------------------------------------------------------------
__global__ void bai_ends_kernel(const BaiArgs a, const BaiWork w, uint8_t* __restrict__ out) {
    bai_put_head(out, a.n_contigs);
    bai_put64(out + 8 + w.ref_base[a.n_contigs], w.rank[a.n] - *w.n_indexed);
}

// one lane per place of the sorted chunk list
__global__ __launch_bounds__(256) void bai_write_chunk_kernel(const BaiArgs a, const BaiWork w, uint8_t* __restrict__ out) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.n || k >= bai_chunks(w, a.n)) return;
    const uint64_t c = w.perm[k], j0 = w.head_pos[c], j1 = w.head_pos[c + 1];
    const uint64_t key = w.key_sorted[k], ref = key >> 16;
    const bool head = w.flag[k] != 0;
    const uint64_t b = w.bins_before[k] + (head ? 1 : 0) - 1, at = w.bin_start[b], first = w.chunk_first[ref];
    uint8_t* bin = out + 8 + w.ref_base[ref] + bai_bin_at(b - w.bins_before[first], at - first);
    if (head) bai_put_bin(bin, (uint32_t)(key & 0xFFFFu), w.bin_start[b + 1] - at);
    bai_put_chunk(bin + 8 + 16 * (k - at), bai_voff_any(a.off[w.rec[j0].slot], a.block_off, a.base, a.n_blocks, a.out_off),
                  bai_voff_any(a.off[w.rec[j1 - 1].slot + 1], a.block_off, a.base, a.n_blocks, a.out_off));
}

constexpr uint32_t kRefRows = 8;  // blocks that share a reference's windows
// block (r, y): lane 0 of row 0 the reference's counts and its pseudo-bin, all lanes its windows y * 256 + lane, + 2048, ...
__global__ __launch_bounds__(256) void bai_write_ref_kernel(const BaiArgs a, const BaiWork w, uint8_t* __restrict__ out) {
    const uint64_t r = blockIdx.x;
    const BaiRef f = bai_ref(w, r);
    uint8_t* ref = out + 8 + w.ref_base[r];
    const bool lead = blockIdx.y == 0 && threadIdx.x == 0;
    if (f.end <= f.first) {
        if (lead) bai_put_empty_ref(ref);
        return;
    }
    if (lead) {
        const uint64_t unmapped = (w.hu[f.end] >> 32) - (w.hu[f.first] >> 32);
        bai_put32(ref, (uint32_t)(f.n_bins + 1));
        bai_put_pseudo(ref + bai_pseudo_at(f.n_bins, f.n_chunks), bai_voff_any(a.off[w.rec[f.first].slot], a.block_off, a.base, a.n_blocks, a.out_off),
                       bai_voff_any(a.off[w.rec[f.end - 1].slot + 1], a.block_off, a.base, a.n_blocks, a.out_off), f.end - f.first - unmapped, unmapped, f.n_intv);
    }
    uint8_t* intv = ref + bai_intv_at(f.n_bins, f.n_chunks) + 4;
    for (uint64_t x = (uint64_t)blockIdx.y * 256 + threadIdx.x; x < f.n_intv; x += kRefRows * 256) {
        const uint64_t j = bai_window_first(w.end_max, f.first, f.end, (uint32_t)r, x);
        bai_put64(intv + 8 * x, bai_voff_any(a.off[w.rec[j].slot], a.block_off, a.base, a.n_blocks, a.out_off));
    }
}

int bai_check(const bg_ctx* ctx, uint64_t n_slots, const void* recs, const void* off, const void* contigs, uint64_t n_contigs, const void* out,
              uint64_t out_cap, uint64_t* out_bytes, uint64_t* first_bad) {
    if (first_bad) *first_bad = UINT64_MAX;
    if (!ctx || !out_bytes || (!out && out_cap) || (n_slots && (!recs || !off)) || (n_contigs && !contigs)) return BG_ERR_INVALID_ARG;
    *out_bytes = 0;
    if (n_slots >= 0xFFFFFFFFull || n_contigs > BAM_MAX_REF) return BG_ERR_TOO_LARGE;
    return BG_OK;
}

// bg_bam_index_dev (d_out_off null) and bg_bam_index_blocks_dev
int index_dev(bg_ctx* ctx, uint64_t n_slots, const uint8_t* d_recs, const uint64_t* d_off, const bg_sam_contig_t* d_contigs, uint64_t n_contigs,
              const uint64_t* d_block_off, uint64_t base, uint64_t n_blocks, const uint64_t* d_out_off, uint8_t* d_out, uint64_t out_cap,
              uint64_t* out_bytes, uint64_t* first_bad, void* stream) {
    int rc = bai_check(ctx, n_slots, d_recs, d_off, d_contigs, n_contigs, d_out, out_cap, out_bytes, first_bad);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);
    const uint64_t n = n_slots, n1 = n + 1, c1 = n_contigs + 1;
    const rocprim::counting_iterator<uint64_t> iota(0);
    const rocprim::plus<uint64_t> plus;
    const rocprim::maximum<uint64_t> maxi;
    size_t t_sum = 0, t_max = 0, t_ref = 0, t_sort = 0;
    BG_HIP(rocprim::exclusive_scan(nullptr, t_sum, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, n1, plus, st));
    BG_HIP(rocprim::inclusive_scan(nullptr, t_max, (uint64_t*)nullptr, (uint64_t*)nullptr, n1, maxi, st));
    BG_HIP(rocprim::exclusive_scan(nullptr, t_ref, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, c1, plus, st));
    if (n) BG_HIP(rocprim::radix_sort_pairs(nullptr, t_sort, (uint64_t*)nullptr, (uint64_t*)nullptr, iota, (uint64_t*)nullptr, n, 0, BAI_KEY_BITS, st));
    unsigned long long* d_cells;  // the first error, n_indexed, then the two words read back
    uint8_t* d_tmp;
    BaiWork w;
    if ((rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_cells = cv.take<unsigned long long>(4);
        w.flag = cv.take<uint64_t>(n1), w.rank = cv.take<uint64_t>(n1);
        w.rec = cv.take<bai_rec_t>(n1);
        w.hu = cv.take<uint64_t>(n1), w.end_key = cv.take<uint64_t>(n1), w.end_max = cv.take<uint64_t>(n1);
        w.key = cv.take<uint64_t>(n1), w.head_pos = cv.take<uint64_t>(n1);
        w.key_sorted = cv.take<uint64_t>(n1), w.perm = cv.take<uint64_t>(n1);
        w.bins_before = cv.take<uint64_t>(n1), w.bin_start = cv.take<uint64_t>(n1);
        w.ref_first = cv.take<uint64_t>(4 * c1);  // one piece: ref_end, chunk_first and chunk_end follow it
        w.ref_bytes = cv.take<uint64_t>(c1), w.ref_base = cv.take<uint64_t>(c1);
        d_tmp = cv.take<uint8_t>(std::max(std::max(t_sum, t_max), std::max(t_ref, t_sort)));
    }))) return rc;
    w.bad = d_cells;
    w.n_indexed = (uint64_t*)(d_cells + 1);
    w.ref_end = w.ref_first + c1;
    w.chunk_first = w.ref_end + c1;
    w.chunk_end = w.chunk_first + c1;
    const BaiArgs a = {n, d_recs, d_off, d_contigs, n_contigs, d_block_off, base, n_blocks, d_out_off};
    BG_HIP(hipMemsetAsync(d_cells, 0xFF, 8, st));
    BG_HIP(hipMemsetAsync(d_cells + 1, 0, 8, st));
    BG_HIP(hipMemsetAsync(w.ref_first, 0, 4 * c1 * 8, st));
    size_t t = 0;
    // 1. records
    bai_flag_kernel<<<lanes(n1), dim3(256), 0, st>>>(a, w);
    BG_HIP(rocprim::exclusive_scan(d_tmp, t = t_sum, w.flag, w.rank, (uint64_t)0, n1, plus, st));
    if (n) bai_decode_kernel<<<lanes(n), dim3(256), 0, st>>>(a, w);
    // 2. neighbours
    bai_link_kernel<<<lanes(n1), dim3(256), 0, st>>>(a, w);
    BG_HIP(hipGetLastError());
    BG_HIP(rocprim::exclusive_scan(d_tmp, t = t_sum, w.flag, w.hu, (uint64_t)0, n1, plus, st));
    BG_HIP(rocprim::inclusive_scan(d_tmp, t = t_max, w.end_key, w.end_max, n1, maxi, st));
    // 3. chunks, bins, references
    if (n) {
        bai_chunk_kernel<<<lanes(n), dim3(256), 0, st>>>(a, w);
        BG_HIP(rocprim::radix_sort_pairs(d_tmp, t = t_sort, w.key, w.key_sorted, iota, w.perm, n, 0, BAI_KEY_BITS, st));
    }
    bai_bin_kernel<<<lanes(n1), dim3(256), 0, st>>>(a, w);
    BG_HIP(rocprim::exclusive_scan(d_tmp, t = t_sum, w.flag, w.bins_before, (uint64_t)0, n1, plus, st));
    bai_bin_start_kernel<<<lanes(n1), dim3(256), 0, st>>>(a, w);
    bai_ref_bytes_kernel<<<lanes(c1), dim3(256), 0, st>>>(a, w);
    BG_HIP(hipGetLastError());
    BG_HIP(rocprim::exclusive_scan(d_tmp, t = t_ref, w.ref_bytes, w.ref_base, (uint64_t)0, c1, plus, st));
    // 4. one read-back, then the bytes
    bai_tail_kernel<<<dim3(1), dim3(1), 0, st>>>(a, w, d_cells + 2);
    unsigned long long tail[2] = {0, 0};
    BG_HIP(hipMemcpyAsync(tail, d_cells + 2, 16, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    if (tail[0] != BAI_NONE) {
        const uint64_t slot = tail[0] >> 2;
        if (first_bad) *first_bad = slot;
        if ((tail[0] & 3) == BAI_UNSUPPORTED) return bg_refuse(("slot " + std::to_string(slot) + " ends beyond 2^29: BAI has no bin for it").c_str(), BG_ERR_UNSUPPORTED);
        return bg_refuse(("slot " + std::to_string(slot) + " is no BAM record of this contig table, or sorts before its predecessor").c_str());
    }
    *out_bytes = tail[1];
    if (!d_out) return BG_OK;
    if (tail[1] > out_cap) return BG_ERR_OPS_CAP;
    bai_ends_kernel<<<dim3(1), dim3(1), 0, st>>>(a, w, d_out);
    if (n) bai_write_chunk_kernel<<<lanes(n), dim3(256), 0, st>>>(a, w, d_out);
    if (n_contigs) bai_write_ref_kernel<<<dim3((uint32_t)n_contigs, kRefRows), dim3(256), 0, st>>>(a, w, d_out);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

// what no index of these inputs exceeds: at most a bin and a chunk a slot, and every window of every contig
uint64_t bai_bound(uint64_t n_slots, const bg_sam_contig_t* contigs, uint64_t n_contigs) {
    uint64_t bound = bai_total(0) + 24 * n_slots;
    for (uint64_t c = 0; c < n_contigs; c++) bound += bai_ref_bytes(true, 0, 0, (contigs[c].len >> BAI_LINEAR_SHIFT) + 1);
    return bound;
}

}  // namespace

extern "C" int bg_bam_index_dev(bg_ctx* ctx, uint64_t n_slots, const uint8_t* d_recs, const uint64_t* d_off, const bg_sam_contig_t* d_contigs,
                                uint64_t n_contigs, const uint64_t* d_block_off, uint64_t base, uint8_t* d_out, uint64_t out_cap,
                                uint64_t* out_bytes, uint64_t* first_bad, void* stream) {
    return index_dev(ctx, n_slots, d_recs, d_off, d_contigs, n_contigs, d_block_off, base, 0, nullptr, d_out, out_cap, out_bytes, first_bad, stream);
}

extern "C" int bg_bam_index_blocks_dev(bg_ctx* ctx, uint64_t n_slots, const uint8_t* d_recs, const uint64_t* d_off, const bg_sam_contig_t* d_contigs,
                                       uint64_t n_contigs, uint64_t n_blocks, const uint64_t* d_block_off, const uint64_t* d_out_off, uint8_t* d_out,
                                       uint64_t out_cap, uint64_t* out_bytes, uint64_t* first_bad, void* stream) {
    if (!d_block_off || !d_out_off) {
        if (first_bad) *first_bad = UINT64_MAX;
        return BG_ERR_INVALID_ARG;
    }
    return index_dev(ctx, n_slots, d_recs, d_off, d_contigs, n_contigs, d_block_off, 0, n_blocks, d_out_off, d_out, out_cap, out_bytes, first_bad, stream);
}

extern "C" int bg_bam_index_blocks(bg_ctx* ctx, uint64_t n_slots, const uint8_t* recs, const uint64_t* off, const bg_sam_contig_t* contigs,
                                   uint64_t n_contigs, uint64_t n_blocks, const uint64_t* block_off, const uint64_t* out_off, uint8_t* out,
                                   uint64_t out_cap, uint64_t* out_bytes, uint64_t* first_bad) {
    int rc = bai_check(ctx, n_slots, recs, off, contigs, n_contigs, out, out_cap, out_bytes, first_bad);
    if (rc) return rc;
    if (!block_off || !out_off) return BG_ERR_INVALID_ARG;
    const uint64_t total = n_slots ? off[n_slots] : 0;
    const uint64_t cap = out ? std::min(out_cap, bai_bound(n_slots, contigs, n_contigs)) : 0;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_recs = s.up(recs, total);
    const uint64_t* d_off = s.up(off, n_slots ? n_slots + 1 : 0);
    const bg_sam_contig_t* d_contigs = s.up(contigs, n_contigs);
    const uint64_t* d_block_off = s.up(block_off, n_blocks + 1);
    const uint64_t* d_out_off = s.up(out_off, n_blocks + 1);
    uint8_t* d_out = out ? s.out<uint8_t>(cap) : nullptr;
    if (s.rc) return s.rc;
    if ((rc = bg_bam_index_blocks_dev(ctx, n_slots, d_recs, d_off, d_contigs, n_contigs, n_blocks, d_block_off, d_out_off, d_out, cap, out_bytes, first_bad, s.st))) return rc;
    if (out) s.down(out, d_out, *out_bytes);
    return s.sync();
}

extern "C" int bg_bam_index(bg_ctx* ctx, uint64_t n_slots, const uint8_t* recs, const uint64_t* off, const bg_sam_contig_t* contigs,
                            uint64_t n_contigs, const uint64_t* block_off, uint64_t base, uint8_t* out, uint64_t out_cap, uint64_t* out_bytes,
                            uint64_t* first_bad) {
    int rc = bai_check(ctx, n_slots, recs, off, contigs, n_contigs, out, out_cap, out_bytes, first_bad);
    if (rc) return rc;
    const uint64_t total = n_slots ? off[n_slots] : 0, n_blocks = (total + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD;
    const uint64_t cap = out ? std::min(out_cap, bai_bound(n_slots, contigs, n_contigs)) : 0;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_recs = s.up(recs, total);
    const uint64_t* d_off = s.up(off, n_slots ? n_slots + 1 : 0);
    const bg_sam_contig_t* d_contigs = s.up(contigs, n_contigs);
    const uint64_t* d_block_off = block_off ? s.up(block_off, n_blocks + 1) : nullptr;
    uint8_t* d_out = out ? s.out<uint8_t>(cap) : nullptr;
    if (s.rc) return s.rc;
    if ((rc = bg_bam_index_dev(ctx, n_slots, d_recs, d_off, d_contigs, n_contigs, d_block_off, base, d_out, cap, out_bytes, first_bad, s.st))) return rc;
    if (out) s.down(out, d_out, *out_bytes);
    return s.sync();
}
