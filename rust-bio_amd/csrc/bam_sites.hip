// Candidate variant sites and region summaries: the pileup held against the reference (bg_bam_sites[_dev]; THE RULE is in
// include/biogpu.h, the bodies in bam_sites_rule.h).  It shares steps 1 to 3 of the pileup (plp_front, bam_pileup.hip) and the
// counting of step 4 (plp_count_tile, bam_pileup_front.h)
// and judges the counters against the reference text in LDS instead of storing them: a count pass, a scan of the tiles' site
// counts, an emit pass over the tiles that have sites.  A tile's share of its region's summary is parked in scratch, 48 bytes a
// tile, and a pass of its own sums a region's tiles (global atomics into one summary were measured first: 58 594 tiles of one
// region queue on one cache line for 1.7 ms).
#include <algorithm>

#include "bam_pileup_front.h"
#include "bam_sites_rule.h"

namespace {

struct SitArgs {
    bg_bam_sites_t prm;
    const uint8_t* text;
    uint32_t* tile_sites;            // [tiles]: the count pass writes it
    const uint64_t* tile_site_off;   // [tiles + 1] scanned: the emit pass reads it
    bg_bam_region_summary_t* tile_share;  // [tiles] in scratch: the count pass parks a tile's share of its region's summary; null: not wanted
    bg_bam_site_t* sites;
    bool wide;
};
static_assert(2 * kThreads == BG_PILEUP_TILE, "a thread takes positions tid and tid + 256; the scan's pairs are 2 t and 2 t + 1");
static_assert(4 * (SIT_W * BG_PILEUP_TILE * 4 + BG_PILEUP_TILE * 4 + 512) <= 160 * 1024, "four workgroups of the sites kernels must fit a CU's LDS");

__device__ __forceinline__ sit_share_t sit_wave_share(sit_share_t s) {
    for (int d = 32; d; d >>= 1) {
        sit_share_t o;
        o.sum_depth = __shfl_xor((unsigned long long)s.sum_depth, d, 64);
        o.match = __shfl_xor((unsigned long long)s.match, d, 64);
        o.mismatch = __shfl_xor((unsigned long long)s.mismatch, d, 64);
        o.packed = __shfl_xor((unsigned long long)s.packed, d, 64);
        o.max_depth = __shfl_xor(s.max_depth, d, 64);
        sit_share_join(s, o);
    }
    return s;
}

// One workgroup per tile: the counters of plp_tile_kernel<16>, then each thread judges positions tid and tid + 256 against the
// reference bytes (adjacent lanes read adjacent banks of a column and adjacent bytes of the text).  The count pass (EMIT false)
// leaves the tile's number of sites and parks its share of its region's summary in scratch; the emit pass counts again in the
// tiles that have sites, scans the 512 per-position counts in LDS and stores the records.
template <bool EMIT>
__global__ __launch_bounds__(kThreads) void sit_tile_kernel(const PlpArgs a, const PlpWork w, const SitArgs s) {
    __shared__ uint32_t cnt[SIT_W * BG_PILEUP_TILE];
    __shared__ uint64_t range[2];
    __shared__ uint32_t scan[EMIT ? BG_PILEUP_TILE : 1];
    __shared__ sit_share_t wave_share[kWaves];
    __shared__ uint32_t wave_sum[kWaves];
    uint64_t first = 0;
    if (EMIT) {
        first = s.tile_site_off[blockIdx.x];
        if (s.tile_site_off[blockIdx.x + 1] == first) return;  // (uniform)
    }
    const plp_tile_t t = plp_tile(blockIdx.x, a.regions, a.n_regions, w.tile_off, w.row_off);
    plp_count_tile<SIT_W>(cnt, range, a, w, t);
    const uint32_t n_pos = (uint32_t)(t.t1 - t.t0), tid = threadIdx.x, wave = tid / 64;
    const uint8_t* ref = s.text + a.contigs[t.ref].start + (uint64_t)t.t0;
    sit_pos_t v[2];
    sit_share_t share = sit_share_zero();
    for (uint32_t h = 0; h < 2; h++) {
        const uint32_t i = tid + h * kThreads;
        v[h].n_sites = 0;
        v[h].mask = 0;
        if (i < n_pos) {
            v[h] = sit_judge(cnt, i, ref[i], s.prm);
            if (!EMIT) sit_share_pos(share, v[h], s.prm);
        }
    }
    if (!EMIT) {
        share = sit_wave_share(share);
        if (tid % 64 == 0) wave_share[wave] = share;
        __syncthreads();
        if (tid == 0) {
            sit_share_t all = wave_share[0];
            for (uint32_t k = 1; k < kWaves; k++) sit_share_join(all, wave_share[k]);
            s.tile_sites[blockIdx.x] = sit_share_sites(all);
            if (s.tile_share) s.tile_share[blockIdx.x] = sit_share_summary(all);
        }
        return;
    }
    scan[tid] = v[0].n_sites;
    scan[tid + kThreads] = v[1].n_sites;
    __syncthreads();
    const uint32_t pair = sit_scan_pair(scan, tid);
    uint32_t incl = pair;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (tid % 64 >= d) incl += up;
    }
    if (tid % 64 == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t ex = incl - pair;
    for (uint32_t k = 0; k < wave; k++) ex += wave_sum[k];
    sit_scan_place(scan, tid, ex);
    __syncthreads();
    for (uint32_t h = 0; h < 2; h++) {
        const uint32_t i = tid + h * kThreads;
        if (!v[h].n_sites) continue;
        bg_bam_site_t* dst = s.sites + first + scan[i];
        for (uint32_t k = 0; k < 5; k++)
            if (v[h].mask >> k & 1u) sit_store(sit_site(cnt, i, v[h], k, t.ref, t.t0 + i, t.region), dst++, s.wide);
    }
}

// One workgroup per region: the shares of its tiles, which are adjacent, summed — threads stride over them, six shuffle steps
// join a wave, LDS joins the four waves — and the summary out as dwords (zeros for a region without a tile).
__global__ __launch_bounds__(kThreads) void sit_region_sum_kernel(const uint64_t* __restrict__ tile_off, const bg_bam_region_summary_t* __restrict__ tile_share,
                                                                  bg_bam_region_summary_t* __restrict__ summary) {
    __shared__ bg_bam_region_summary_t wave_sum[kWaves];
    const uint64_t r = blockIdx.x;
    bg_bam_region_summary_t a = sit_summary_stride(tile_share, tile_off[r], tile_off[r + 1], threadIdx.x, kThreads);
    for (int d = 32; d; d >>= 1) {
        bg_bam_region_summary_t o;
        o.sum_depth = __shfl_xor((unsigned long long)a.sum_depth, d, 64);
        o.match = __shfl_xor((unsigned long long)a.match, d, 64);
        o.mismatch = __shfl_xor((unsigned long long)a.mismatch, d, 64);
        for (uint32_t k = 0; k < 4; k++) o.covered[k] = __shfl_xor(a.covered[k], d, 64);
        o.max_depth = __shfl_xor(a.max_depth, d, 64);
        o.n_ref_other = __shfl_xor(a.n_ref_other, d, 64);
        sit_summary_join(a, o);
    }
    if (threadIdx.x % 64 == 0) wave_sum[threadIdx.x / 64] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t k = 1; k < kWaves; k++) sit_summary_join(a, wave_sum[k]);
        sit_summary_store(a, summary + r);
    }
}

// site_off[r] = the sites in front of region r's first tile; tiles == 0: no region has a position
__global__ __launch_bounds__(256) void sit_region_off_kernel(uint64_t n_regions, const uint64_t* __restrict__ tile_off, const uint64_t* __restrict__ tile_site_off,
                                                             uint64_t tiles, uint64_t* __restrict__ site_off) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n_regions) return;
    site_off[r] = tiles ? tile_site_off[tile_off[r]] : 0;
}

int sit_check(const bg_ctx* ctx, const bg_bam_sites_t* prm, uint64_t n_slots, const void* recs, const void* off, const void* contigs, uint64_t n_contigs,
              const void* text, uint64_t n_text, const void* regions, uint64_t n_regions, const void* sites, uint64_t sites_cap, uint64_t* n_sites,
              uint64_t* first_bad) {
    const bool own_ok = n_sites && (sites || !sites_cap) && (text || !n_text);
    return plp_check_args(ctx, prm, n_slots, recs, off, contigs, n_contigs, regions, n_regions, first_bad, own_ok, [&] {
        *n_sites = 0;
        if (prm->flags || prm->reserved) return bg_refuse("bg_bam_sites: flags or reserved is not 0");
        if (prm->min_alt_permille > 1000) return bg_refuse("bg_bam_sites: min_alt_permille is above 1000");
        return (int)BG_OK;
    });
}

}  // namespace

// bg_bam_sites_dev: the front (steps 1 to 3 of the pileup, with the regions' contigs held against the text), then
//   4. the count pass, one workgroup per tile: the tile's number of sites, its share of its region's summary (both in scratch);
//   5. a scan of the tile counts places the tiles; the SECOND read-back gives n_sites, and the sizing call ends here;
//   6. one workgroup per region sums its tiles' shares into d_summary; the regions' offsets out; the emit pass over the tiles
//      that have sites.
// Scratch behind the front's is ctx->tb (the front's lies in ctx->aux and must survive): 12 bytes a tile, and 48 more where the
// summaries are asked for.
extern "C" int bg_bam_sites_dev(bg_ctx* ctx, const bg_bam_sites_t* prm, uint64_t n_slots, const uint8_t* d_recs, const uint64_t* d_off,
                                const bg_sam_contig_t* d_contigs, uint64_t n_contigs, const uint8_t* d_text, uint64_t n_text,
                                const bg_bam_region_t* d_regions, uint64_t n_regions, bg_bam_site_t* d_sites, uint64_t sites_cap, uint64_t* d_site_off,
                                bg_bam_region_summary_t* d_summary, uint64_t* n_sites, uint64_t* first_bad, void* stream) {
    int rc = sit_check(ctx, prm, n_slots, d_recs, d_off, d_contigs, n_contigs, d_text, n_text, d_regions, n_regions, d_sites, sites_cap, n_sites, first_bad);
    if (rc) return rc;
    if (((uintptr_t)d_sites | (uintptr_t)d_summary) & 3u) return bg_refuse("bg_bam_sites_dev: d_sites or d_summary is not 4-byte aligned");
    if ((uintptr_t)d_site_off & 7u) return bg_refuse("bg_bam_sites_dev: d_site_off is not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);
    const uint64_t nr = n_regions;
    const PlpArgs a = {n_slots, d_recs, d_off, d_contigs, n_contigs, d_regions, nr, sit_pileup_params(*prm), true, n_text};
    PlpFront f;
    if ((rc = plp_front(ctx, st, a, &f, first_bad))) return rc;
    const uint64_t tiles = f.tiles;
    const bool sizing = !d_sites;
    SitArgs sa;
    uint64_t *d_soff, *d_sums;
    if ((rc = bg_reserve_carved(&ctx->tb, &ctx->tb_bytes, [&](bg_carve& cv) {
        sa.tile_sites = cv.take<uint32_t>(tiles);
        sa.tile_site_off = d_soff = cv.take<uint64_t>(tiles + 1);
        d_sums = cv.take<uint64_t>(bg_scan_sums_words(tiles));
        sa.tile_share = sizing || !d_summary ? nullptr : cv.take<bg_bam_region_summary_t>(tiles);
    }))) return rc;
    sa.prm = *prm;
    sa.text = d_text;
    sa.sites = d_sites;
    sa.wide = ((uintptr_t)d_sites & 15u) == 0;
    uint64_t total = 0;
    if (tiles) {
        // 4. the count pass
        sit_tile_kernel<false><<<dim3((uint32_t)tiles), dim3(kThreads), 0, st>>>(a, f.w, sa);
        BG_HIP(hipGetLastError());
        // 5. the tiles placed
        if ((rc = bg_scan_u32(sa.tile_sites, tiles, d_soff, d_sums, st))) return rc;
        BG_HIP(hipMemcpyAsync(&total, sa.tile_site_off + tiles, 8, hipMemcpyDeviceToHost, st));
        BG_HIP(hipStreamSynchronize(st));
    }
    if (total >= (1ull << 32)) return BG_ERR_TOO_LARGE;
    *n_sites = total;
    if (sizing) return BG_OK;
    if (total > sites_cap) return BG_ERR_OPS_CAP;
    // 6. out
    if (d_summary && nr) {
        if (!tiles) BG_HIP(hipMemsetAsync(d_summary, 0, nr * sizeof(bg_bam_region_summary_t), st));
        else sit_region_sum_kernel<<<dim3((uint32_t)nr), dim3(kThreads), 0, st>>>(f.w.tile_off, sa.tile_share, d_summary);
        BG_HIP(hipGetLastError());
    }
    if (d_site_off) {
        sit_region_off_kernel<<<lanes(nr + 1), dim3(256), 0, st>>>(nr, f.w.tile_off, sa.tile_site_off, tiles, d_site_off);
        BG_HIP(hipGetLastError());
    }
    if (total) {
        sit_tile_kernel<true><<<dim3((uint32_t)tiles), dim3(kThreads), 0, st>>>(a, f.w, sa);
        BG_HIP(hipGetLastError());
    }
    return BG_OK;
}

extern "C" int bg_bam_sites(bg_ctx* ctx, const bg_bam_sites_t* prm, uint64_t n_slots, const uint8_t* recs, const uint64_t* off, const bg_sam_contig_t* contigs,
                            uint64_t n_contigs, const uint8_t* text, uint64_t n_text, const bg_bam_region_t* regions, uint64_t n_regions, bg_bam_site_t* sites,
                            uint64_t sites_cap, uint64_t* site_off, bg_bam_region_summary_t* summary, uint64_t* n_sites, uint64_t* first_bad) {
    int rc = sit_check(ctx, prm, n_slots, recs, off, contigs, n_contigs, text, n_text, regions, n_regions, sites, sites_cap, n_sites, first_bad);
    if (rc) return rc;
    uint64_t bound = 0;  // what no call on these regions exceeds: five sites a position
    for (uint64_t r = 0; r < n_regions; r++) bound += regions[r].end > regions[r].beg ? 5 * (uint64_t)((int64_t)regions[r].end - regions[r].beg) : 0;
    const uint64_t cap = sites ? std::min(sites_cap, bound) : 0;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_recs = s.up(recs, n_slots ? off[n_slots] : 0);
    const uint64_t* d_off = s.up(off, n_slots ? n_slots + 1 : 0);
    const bg_sam_contig_t* d_contigs = s.up(contigs, n_contigs);
    const uint8_t* d_text = s.up(text, n_text);
    const bg_bam_region_t* d_regions = s.up(regions, n_regions);
    bg_bam_site_t* d_sites = sites ? s.out<bg_bam_site_t>(cap) : nullptr;
    uint64_t* d_site_off = sites && site_off ? s.out<uint64_t>(n_regions + 1) : nullptr;
    bg_bam_region_summary_t* d_summary = sites && summary ? s.out<bg_bam_region_summary_t>(n_regions) : nullptr;
    if (s.rc) return s.rc;
    if ((rc = bg_bam_sites_dev(ctx, prm, n_slots, d_recs, d_off, d_contigs, n_contigs, d_text, n_text, d_regions, n_regions, d_sites, cap, d_site_off, d_summary,
                               n_sites, first_bad, s.st)))
        return rc;
    if (sites) {
        s.down(sites, d_sites, *n_sites);
        if (site_off) s.down(site_off, d_site_off, n_regions + 1);
        if (summary) s.down(summary, d_summary, n_regions);
    }
    return s.sync();
}
