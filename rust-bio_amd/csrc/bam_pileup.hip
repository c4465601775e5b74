// Pileup: one row of counters for each reference position of a batch of regions, from a coordinate-sorted run of BAM records
// (bg_bam_pileup[_dev]; THE RULE is in include/biogpu.h, the bodies in bam_pileup_rule.h).  Integer scatter-add work, tiled in
// LDS; no counter is ever added to in global memory, so the rows are plain stores and an exact function of the inputs.
//   1. one lane per slot: bai_decode, the pileup's own checks, the kept verdict, the keys ((ref, pos + 1) and (ref, end); an
//      empty slot gets 0 for both, an unplaced record sorts last by its refID), the first error by an ordinary atomic minimum;
//   2. the running maxima of both keys (rocPRIM, as bam_index.hip): that of (ref, end) is inside a reference the prefix
//      maximum of `end`; that of (ref, pos + 1) equals a slot's own key exactly where the slot does not sort before a
//      predecessor, which is the order check, and carries a record's key over the empty slots behind it;
//   3. one lane per region: the check, its length and its tiles (BG_PILEUP_TILE positions, never across regions); two scans
//      (bg_scan_u32) place the regions' rows and number the tiles.  The first error, the rows and the tiles are read back once;
//   4. one workgroup per tile: its region by binary search in the tile numbers, its candidate slots [lo, hi) by two binary
//      searches in the running maxima (lo: the first slot whose end maximum exceeds (ref, t0); hi: the first whose key is
//      >= (ref, t1)), LDS counters zeroed, a group of 16 lanes per candidate record walking its operations uniformly and
//      striding over the positions of an operation inside the tile (LDS adds whose value is not used: ds_add_u32), a barrier,
//      then the rows out, transposed, 16 bytes wide where d_rows is 16-byte aligned and as dwords otherwise.
// Known costs: a tile under a pile of extreme depth is one workgroup's work; a record of many operations is walked again by
// every tile it spans; the transposing read of the counters (4 or 8 columns apart in adjacent lanes) conflicts 2- or 4-way
// in LDS, and W-way in the dword form.  Scratch is the ctx's: 33 bytes a slot and 24 a region.
// Steps 1 to 3 are plp_front, which bam_sites.hip and bam_indels.hip call as well (bam_pileup_front.h declares it and holds the
// counting of step 4, which their tile kernels share); its kernels are compiled here and nowhere else.
#include <algorithm>

#include <rocprim/device/device_scan.hpp>

#include "bam_pileup_front.h"
#include "bam_sites_rule.h"

static_assert(sizeof(bg_bam_region_t) == 12 && sizeof(bg_bam_pileup_t) == 12, "the boundary's structs");
static_assert(2 * BG_PILEUP_COLS * BG_PILEUP_TILE * 4 * 2 <= 160 * 1024, "two workgroups of the 16-column form must fit a CU's LDS");

namespace {

__device__ __forceinline__ void plp_report(const PlpWork& w, uint64_t slot, int kind) { atomicMin(w.bad, (unsigned long long)((slot << 2) | (uint64_t)kind)); }

__global__ __launch_bounds__(256) void plp_slot_kernel(const PlpArgs a, const PlpWork w) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    plp_slot_t s = {0, 0, 0};
    const uint64_t o0 = a.off[i], o1 = a.off[i + 1];
    if (o1 < o0) plp_report(w, i, BAI_INVALID);
    if (o1 > o0) {
        const int kind = plp_slot(a.recs + o0, o1 - o0, a.contigs, a.n_contigs, a.prm, &s);
        if (kind) plp_report(w, i, kind);
    }
    w.pos_key[i] = s.pos_key;
    w.end_key[i] = s.end_key;
    w.kept[i] = s.kept;
}

// a non-empty slot whose key is below the running maximum sorts before a predecessor
__global__ __launch_bounds__(256) void plp_order_kernel(const PlpArgs a, const PlpWork w) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    if (a.off[i + 1] > a.off[i] && w.pos_max[i] != w.pos_key[i]) plp_report(w, i, BAI_INVALID);
}

__global__ __launch_bounds__(256) void plp_region_kernel(const PlpArgs a, const PlpWork w) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n_regions) return;
    const bg_bam_region_t g = a.regions[r];
    uint32_t len = 0;
    if (a.in_text ? sit_region_ok(g, a.contigs, a.n_contigs, a.n_text) : plp_region_ok(g, a.contigs, a.n_contigs)) len = (uint32_t)(g.end - g.beg);
    else *w.region_bad = 1;
    w.region_len[r] = len;
    w.region_tiles[r] = plp_tiles(len);
}

// the first error, the regions' verdict, the rows and the tiles side by side, for one read-back
__global__ void plp_tail_kernel(const PlpArgs a, const PlpWork w, unsigned long long* __restrict__ tail) {
    tail[0] = *w.bad;
    tail[1] = *w.region_bad;
    tail[2] = a.n_regions ? w.row_off[a.n_regions] : 0;
    tail[3] = a.n_regions ? w.tile_off[a.n_regions] : 0;
}

// one workgroup per tile; W: the uint32 of a row
template <uint32_t W>
__global__ __launch_bounds__(kThreads) void plp_tile_kernel(const PlpArgs a, const PlpWork w, uint32_t* __restrict__ rows, bool wide) {
    __shared__ uint32_t cnt[W * BG_PILEUP_TILE];
    __shared__ uint64_t range[2];
    const plp_tile_t t = plp_tile(blockIdx.x, a.regions, a.n_regions, w.tile_off, w.row_off);  // the same loads in every lane
    plp_count_tile<W>(cnt, range, a, w, t);
    plp_store_rows(cnt, W, (uint32_t)(t.t1 - t.t0), rows + t.row * W, wide, threadIdx.x, kThreads);
}

int plp_check(const bg_ctx* ctx, const bg_bam_pileup_t* prm, uint64_t n_slots, const void* recs, const void* off, const void* contigs, uint64_t n_contigs,
              const void* regions, uint64_t n_regions, const void* rows, uint64_t rows_cap, uint64_t* n_rows, uint64_t* first_bad) {
    return plp_check_args(ctx, prm, n_slots, recs, off, contigs, n_contigs, regions, n_regions, first_bad, n_rows && (rows || !rows_cap), [&] {
        *n_rows = 0;
        if ((prm->flags & ~(uint32_t)BG_PILEUP_STRANDS) || prm->reserved) return bg_refuse("bg_bam_pileup: unknown flag bits, or reserved is not 0");
        return (int)BG_OK;
    });
}

}  // namespace

// steps 1 to 3 (bam_pileup_front.h)
int plp_front(bg_ctx* ctx, hipStream_t st, const PlpArgs& a, PlpFront* f, uint64_t* first_bad) {
    int rc;
    const uint64_t n = a.n, nr = a.n_regions;
    const rocprim::maximum<uint64_t> maxi;
    size_t t_max = 0;
    if (n) BG_HIP(rocprim::inclusive_scan(nullptr, t_max, (uint64_t*)nullptr, (uint64_t*)nullptr, n, maxi, st));
    unsigned long long* d_cells;  // the first error, the regions' verdict, then the four words read back
    uint64_t* d_sums;
    uint8_t* d_tmp;
    PlpWork& w = f->w;
    if ((rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_cells = cv.take<unsigned long long>(6);
        w.pos_key = cv.take<uint64_t>(n), w.end_key = cv.take<uint64_t>(n);
        w.pos_max = cv.take<uint64_t>(n), w.end_max = cv.take<uint64_t>(n);
        w.kept = cv.take<uint8_t>(n);
        w.region_len = cv.take<uint32_t>(nr), w.region_tiles = cv.take<uint32_t>(nr);
        w.row_off = cv.take<uint64_t>(nr + 1), w.tile_off = cv.take<uint64_t>(nr + 1);
        d_sums = cv.take<uint64_t>(bg_scan_sums_words(nr));
        d_tmp = cv.take<uint8_t>(t_max);
    }))) return rc;
    w.bad = d_cells;
    w.region_bad = (uint64_t*)(d_cells + 1);
    BG_HIP(hipMemsetAsync(d_cells, 0xFF, 8, st));
    BG_HIP(hipMemsetAsync(d_cells + 1, 0, 8, st));
    // 1., 2. slots
    if (n) {
        size_t t = 0;
        plp_slot_kernel<<<lanes(n), dim3(256), 0, st>>>(a, w);
        BG_HIP(hipGetLastError());
        BG_HIP(rocprim::inclusive_scan(d_tmp, t = t_max, w.pos_key, w.pos_max, n, maxi, st));
        BG_HIP(rocprim::inclusive_scan(d_tmp, t = t_max, w.end_key, w.end_max, n, maxi, st));
        plp_order_kernel<<<lanes(n), dim3(256), 0, st>>>(a, w);
    }
    // 3. regions
    if (nr) {
        plp_region_kernel<<<lanes(nr), dim3(256), 0, st>>>(a, w);
        BG_HIP(hipGetLastError());
        if ((rc = bg_scan_u32(w.region_len, nr, w.row_off, d_sums, st))) return rc;
        if ((rc = bg_scan_u32(w.region_tiles, nr, w.tile_off, d_sums, st))) return rc;
    }
    plp_tail_kernel<<<dim3(1), dim3(1), 0, st>>>(a, w, d_cells + 2);
    unsigned long long tail[4] = {0, 0, 0, 0};
    BG_HIP(hipMemcpyAsync(tail, d_cells + 2, sizeof tail, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    if (tail[1])
        return bg_refuse(a.in_text ? "bg_bam_sites: a region lies outside its contig, names none, has beg > end, or its contig lies outside the text"
                                   : "bg_bam_pileup: a region lies outside its contig, names none, or has beg > end");
    if (tail[0] != BAI_NONE) {
        const uint64_t slot = tail[0] >> 2;
        if (first_bad) *first_bad = slot;
        if ((tail[0] & 3) == BAI_UNSUPPORTED)
            return bg_refuse(("slot " + std::to_string(slot) + " ends beyond 2^29, or holds the placeholder of a CG tag").c_str(), BG_ERR_UNSUPPORTED);
        return bg_refuse(("slot " + std::to_string(slot) + " is no BAM record of this contig table, has a CIGAR that does not fit its bases, or sorts before its predecessor").c_str());
    }
    if (tail[2] >= (1ull << 32)) return BG_ERR_TOO_LARGE;
    f->n_rows = tail[2];
    f->tiles = tail[3];
    return BG_OK;
}

extern "C" int bg_bam_pileup_dev(bg_ctx* ctx, const bg_bam_pileup_t* prm, uint64_t n_slots, const uint8_t* d_recs, const uint64_t* d_off,
                                 const bg_sam_contig_t* d_contigs, uint64_t n_contigs, const bg_bam_region_t* d_regions, uint64_t n_regions,
                                 uint32_t* d_rows, uint64_t rows_cap, uint64_t* d_row_off, uint64_t* n_rows, uint64_t* first_bad, void* stream) {
    int rc = plp_check(ctx, prm, n_slots, d_recs, d_off, d_contigs, n_contigs, d_regions, n_regions, d_rows, rows_cap, n_rows, first_bad);
    if (rc) return rc;
    if ((uintptr_t)d_rows & 3u) return bg_refuse("bg_bam_pileup_dev: d_rows is not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);
    const uint64_t nr = n_regions;
    const PlpArgs a = {n_slots, d_recs, d_off, d_contigs, n_contigs, d_regions, nr, *prm, false, 0};
    PlpFront f;
    if ((rc = plp_front(ctx, st, a, &f, first_bad))) return rc;
    const PlpWork& w = f.w;
    *n_rows = f.n_rows;
    if (!d_rows) return BG_OK;
    if (f.n_rows > rows_cap) return BG_ERR_OPS_CAP;
    if (d_row_off && nr) BG_HIP(hipMemcpyAsync(d_row_off, w.row_off, (nr + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (d_row_off && !nr) BG_HIP(hipMemsetAsync(d_row_off, 0, 8, st));
    // 4. tiles
    if (f.tiles) {
        const bool wide = ((uintptr_t)d_rows & 15u) == 0;
        if (prm->flags & BG_PILEUP_STRANDS) plp_tile_kernel<2 * BG_PILEUP_COLS><<<dim3((uint32_t)f.tiles), dim3(kThreads), 0, st>>>(a, w, d_rows, wide);
        else plp_tile_kernel<BG_PILEUP_COLS><<<dim3((uint32_t)f.tiles), dim3(kThreads), 0, st>>>(a, w, d_rows, wide);
        BG_HIP(hipGetLastError());
    }
    return BG_OK;
}

extern "C" int bg_bam_pileup(bg_ctx* ctx, const bg_bam_pileup_t* prm, uint64_t n_slots, const uint8_t* recs, const uint64_t* off,
                             const bg_sam_contig_t* contigs, uint64_t n_contigs, const bg_bam_region_t* regions, uint64_t n_regions, uint32_t* rows,
                             uint64_t rows_cap, uint64_t* row_off, uint64_t* n_rows, uint64_t* first_bad) {
    int rc = plp_check(ctx, prm, n_slots, recs, off, contigs, n_contigs, regions, n_regions, rows, rows_cap, n_rows, first_bad);
    if (rc) return rc;
    const uint64_t W = prm->flags & BG_PILEUP_STRANDS ? 2 * BG_PILEUP_COLS : BG_PILEUP_COLS;
    uint64_t bound = 0;  // what no call on these regions exceeds
    for (uint64_t r = 0; r < n_regions; r++) bound += regions[r].end > regions[r].beg ? (uint64_t)((int64_t)regions[r].end - regions[r].beg) : 0;
    const uint64_t cap = rows ? std::min(rows_cap, bound) : 0;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_recs = s.up(recs, n_slots ? off[n_slots] : 0);
    const uint64_t* d_off = s.up(off, n_slots ? n_slots + 1 : 0);
    const bg_sam_contig_t* d_contigs = s.up(contigs, n_contigs);
    const bg_bam_region_t* d_regions = s.up(regions, n_regions);
    uint32_t* d_rows = rows ? s.out<uint32_t>(cap * W) : nullptr;
    uint64_t* d_row_off = rows && row_off ? s.out<uint64_t>(n_regions + 1) : nullptr;
    if (s.rc) return s.rc;
    if ((rc = bg_bam_pileup_dev(ctx, prm, n_slots, d_recs, d_off, d_contigs, n_contigs, d_regions, n_regions, d_rows, cap, d_row_off, n_rows, first_bad, s.st)))
        return rc;
    if (rows) {
        s.down(rows, d_rows, *n_rows * W);
        if (row_off) s.down(row_off, d_row_off, n_regions + 1);
    }
    return s.sync();
}
