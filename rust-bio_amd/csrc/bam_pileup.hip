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
// bg_bam_sites[_dev] (the bodies in bam_sites_rule.h) shares steps 1 to 3 (plp_front) and the counting of step 4 (plp_count_tile)
// and judges the counters against the reference text in LDS instead of storing them: a count pass, a scan of the tiles' site
// counts, an emit pass over the tiles that have sites.  A tile's share of its region's summary is parked in scratch, 48 bytes a
// tile, and a pass of its own sums a region's tiles (global atomics into one summary were measured first: 58 594 tiles of one
// region queue on one cache line for 1.7 ms).
// bg_bam_indels[_dev] (the bodies in bam_indels_rule.h) shares steps 1 to 3 and plp_count_tile as well and keeps what the walk
// reads and drops, an operation's length and the inserted bases: a count pass and an emit pass over the tiles leave the raw
// events in scratch, a merge sort orders them by the full key, heads of runs and prefix sums of the strand bits make them events
// (the steps are listed at the entry point).
// bg_bam_indels_left[_dev] (the bodies in bam_indels_left_rule.h) is that call with a shift of every raw event against the
// reference text between the walk and the window (inl_tile_kernel), the sort and the placement through the shifted codes; its
// merge sort is instantiated in bam_indels_left_sort.hip.
#include <algorithm>

#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "bg_common.h"
#include "bam_pileup_rule.h"
#include "bam_sites_rule.h"
#include "bam_indels_rule.h"
#include "bam_indels_left_rule.h"

static_assert(sizeof(bg_bam_region_t) == 12 && sizeof(bg_bam_pileup_t) == 12, "the boundary's structs");
static_assert(2 * BG_PILEUP_COLS * BG_PILEUP_TILE * 4 * 2 <= 160 * 1024, "two workgroups of the 16-column form must fit a CU's LDS");

// bam_indels_left_sort.hip: the merge sort of the left-aligned raw events by inl_cmp, kept out of this file so that the kernels of
// bg_bam_indels_dev's sort are compiled as they were (the reason is written there)
int inl_sort_raw(void* d_tmp, size_t tmp_bytes, const ind_raw_t* raw, const uint8_t* recs, const uint64_t* off, uint32_t* order, uint64_t n, hipStream_t st);

namespace {

constexpr uint32_t kThreads = 256;

struct PlpArgs {
    uint64_t n;  // slots
    const uint8_t* recs;
    const uint64_t* off;
    const bg_sam_contig_t* contigs;
    uint64_t n_contigs;
    const bg_bam_region_t* regions;
    uint64_t n_regions;
    bg_bam_pileup_t prm;
    bool in_text;     // bg_bam_sites: a region's contig must lie inside [0, n_text)
    uint64_t n_text;
};
struct PlpWork {
    unsigned long long* bad;  // slot << 2 | kind of the first offending slot, BAI_NONE without one
    uint64_t* region_bad;     // non-zero: some region fails plp_region_ok
    uint64_t* pos_key;        // [n]
    uint64_t* end_key;        // [n]
    uint64_t* pos_max;        // [n] running maxima
    uint64_t* end_max;        // [n]
    uint8_t* kept;            // [n]
    uint32_t* region_len;     // [n_regions]
    uint32_t* region_tiles;   // [n_regions]
    uint64_t* row_off;        // [n_regions + 1] scanned
    uint64_t* tile_off;       // [n_regions + 1] scanned
};

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

// A tile's counters, by all the threads of its workgroup: cnt zeroed, the candidate slots [lo, hi) by the two searches, every
// kept one walked by a group of PLP_G lanes, a barrier.  W: the columns counted (SIT_W under BG_PILEUP_STRANDS)
template <uint32_t W>
__device__ __forceinline__ void plp_count_tile(uint32_t* cnt, uint64_t* range, const PlpArgs& a, const PlpWork& w, const plp_tile_t& t) {
    for (uint32_t i = threadIdx.x; i < W * BG_PILEUP_TILE; i += kThreads) cnt[i] = 0;
    if (threadIdx.x == 0) range[0] = plp_lo(w.end_max, a.n, t);
    if (threadIdx.x == 64) range[1] = plp_hi(w.pos_max, a.n, t);
    __syncthreads();
    const uint64_t lo = range[0], hi = range[1];
    const uint32_t group = threadIdx.x / PLP_G, lane = threadIdx.x % PLP_G;
    for (uint64_t s = lo + group; s < hi; s += kThreads / PLP_G) {
        if (!w.kept[s]) continue;
        plp_walk_lane(a.recs + a.off[s], a.prm, t.ref, t.t0, t.t1, lane, [&](uint32_t i) { atomicAdd(&cnt[i], 1u); });
    }
    __syncthreads();
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

// ---- sites ------------------------------------------------------------------------------------------------------------------
struct SitArgs {
    bg_bam_sites_t prm;
    const uint8_t* text;
    uint32_t* tile_sites;            // [tiles]: the count pass writes it
    const uint64_t* tile_site_off;   // [tiles + 1] scanned: the emit pass reads it
    bg_bam_region_summary_t* tile_share;  // [tiles] in scratch: the count pass parks a tile's share of its region's summary; null: not wanted
    bg_bam_site_t* sites;
    bool wide;
};
constexpr uint32_t kWaves = kThreads / 64;
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

// ---- indel events -----------------------------------------------------------------------------------------------------------
struct IndWork {
    uint32_t* tile_raw;             // [tiles]: the count pass writes it
    const uint64_t* tile_raw_off;   // [tiles + 1] scanned
    ind_raw_t* raw;                 // [n_raw]: the emit pass fills a tile's range, in any order inside it
    uint32_t* order;                // [n_raw]: the raw events by the full key
    uint32_t* head;                 // [n_raw]: 1 where a run of equal raw events begins (sorted order)
    uint32_t* rev;                  // [n_raw]: the strand bit (sorted order)
    uint64_t* head_off;             // [n_raw + 1] scanned: head_off[i] of a head is its run's number; head_off[n_raw] the runs
    uint64_t* rev_off;              // [n_raw + 1] scanned
    uint32_t* run_start;            // [n_raw + 1]: the sorted index a run begins at; n_raw behind the last run
    uint32_t* keep;                 // [n_raw]: by run, 1 for a kept event (0 behind the last run)
    uint32_t* seq_len;              // [n_raw]: by run, the bytes of a kept insertion
    uint64_t* keep_off;             // [n_raw + 1] scanned
    uint64_t* seq_off;              // [n_raw + 1] scanned
};
struct IndOrder {  // the comparator of the merge sort: indices into raw
    const ind_raw_t* raw;
    const uint8_t* recs;
    const uint64_t* off;
    __device__ bool operator()(uint32_t a, uint32_t b) const { return ind_cmp(raw[a], raw[b], recs, off) < 0; }
};

// One workgroup per tile, one thread per candidate record.  The count pass (EMIT false) leaves the tile's number of raw events.
// The emit pass runs in the tiles that have some: the 8-column counters of the tile for the depth of the anchors, then the same
// walk again; a raw event takes the next place of the tile's range of scratch from a counter in LDS, so the order inside the
// range is that of arrival and everything behind this pass is independent of it.
template <bool EMIT>
__global__ __launch_bounds__(kThreads) void ind_tile_kernel(const PlpArgs a, const PlpWork w, const IndWork x) {
    __shared__ uint32_t cnt[EMIT ? BG_PILEUP_COLS * BG_PILEUP_TILE : 1];
    __shared__ uint64_t range[2];
    __shared__ uint32_t wave_sum[kWaves];
    __shared__ uint32_t next;
    uint64_t first = 0;
    uint32_t room = 0;
    if (EMIT) {
        first = x.tile_raw_off[blockIdx.x];
        room = (uint32_t)(x.tile_raw_off[blockIdx.x + 1] - first);
        if (!room) return;  // (uniform)
    }
    const plp_tile_t t = plp_tile(blockIdx.x, a.regions, a.n_regions, w.tile_off, w.row_off);
    if (EMIT) {
        plp_count_tile<BG_PILEUP_COLS>(cnt, range, a, w, t);
        if (threadIdx.x == 0) next = 0;
    } else {
        if (threadIdx.x == 0) range[0] = plp_lo(w.end_max, a.n, t);
        if (threadIdx.x == 64) range[1] = plp_hi(w.pos_max, a.n, t);
    }
    __syncthreads();
    const uint64_t lo = range[0], hi = range[1];
    uint32_t mine = 0;
    for (uint64_t s = lo + threadIdx.x; s < hi; s += kThreads) {
        if (!w.kept[s]) continue;
        const uint8_t* rec = a.recs + a.off[s];
        const uint32_t flag = bai_get16(rec + 18);
        ind_walk(rec, t.ref, t.t0, t.t1, [&](uint32_t kind, uint32_t anchor, uint32_t len, uint32_t q) {
            if (EMIT) {
                const uint32_t place = atomicAdd(&next, 1u);
                if (place < room) x.raw[first + place] = ind_raw(blockIdx.x, kind, anchor, len, q, flag, ind_depth(cnt, anchor - (uint32_t)t.t0), s);
            } else {
                mine++;
            }
        });
    }
    if (EMIT) return;
    for (int d = 32; d; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if (threadIdx.x % 64 == 0) wave_sum[threadIdx.x / 64] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (uint32_t k = 0; k < kWaves; k++) all += wave_sum[k];
        x.tile_raw[blockIdx.x] = all;
    }
}

// sorted index i: does a run begin here, and the strand bit
__global__ __launch_bounds__(256) void ind_head_kernel(uint64_t n_raw, const PlpArgs a, const IndWork x) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_raw) return;
    const ind_raw_t e = x.raw[x.order[i]];
    x.head[i] = i == 0 || ind_cmp(x.raw[x.order[i - 1]], e, a.recs, a.off) != 0;
    x.rev[i] = ind_rev(e);
}
// a head's sorted index at its run's number; n_raw behind the last run
__global__ __launch_bounds__(256) void ind_run_kernel(uint64_t n_raw, const IndWork x) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n_raw) return;
    if (i == n_raw) x.run_start[x.head_off[n_raw]] = (uint32_t)n_raw;
    else if (x.head[i]) x.run_start[x.head_off[i]] = (uint32_t)i;
}
// run k: its counts as differences, the verdict, the bytes it adds to the sequences
__global__ __launch_bounds__(256) void ind_judge_kernel(uint64_t n_raw, const bg_bam_indels_t prm, const IndWork x) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_raw) return;
    uint32_t keep = 0, bytes = 0;
    if (k < x.head_off[n_raw]) {
        const uint32_t s = x.run_start[k], e = x.run_start[k + 1];
        const uint32_t rev = (uint32_t)(x.rev_off[e] - x.rev_off[s]);
        const ind_raw_t v = x.raw[x.order[s]];
        keep = ind_is_kept(e - s - rev, rev, v.depth, prm);
        bytes = keep && ind_kind(v) == BG_SITE_INS ? v.len : 0;
    }
    x.keep[k] = keep;
    x.seq_len[k] = bytes;
}
// PLP_G lanes a run: a kept event's record, and the bytes of a kept insertion
__global__ __launch_bounds__(256) void ind_place_kernel(uint64_t n_raw, const PlpArgs a, const PlpWork w, const IndWork x, bg_bam_indel_t* __restrict__ events,
                                                        uint8_t* __restrict__ seq) {
    const uint64_t k = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / PLP_G;
    const uint32_t lane = threadIdx.x % PLP_G;
    if (k >= n_raw || !x.keep[k]) return;
    const uint32_t s = x.run_start[k], e = x.run_start[k + 1];
    const uint32_t rev = (uint32_t)(x.rev_off[e] - x.rev_off[s]);
    const ind_raw_t v = x.raw[x.order[s]];
    if (lane == 0) {
        const plp_tile_t t = plp_tile(v.tile, a.regions, a.n_regions, w.tile_off, w.row_off);
        ind_store(ind_event(v, t.ref, t.region, e - s - rev, rev, x.seq_off[k]), events + x.keep_off[k]);
    }
    if (ind_kind(v) == BG_SITE_INS) ind_seq_lane(v, a.recs, a.off, seq + x.seq_off[k], lane, PLP_G);
}
// event_off[r] = the events in front of region r's first tile: that tile's first raw event in sorted order is a head
__global__ __launch_bounds__(256) void ind_region_off_kernel(uint64_t n_regions, const uint64_t* __restrict__ tile_off, uint64_t tiles, uint64_t n_raw,
                                                             const IndWork x, uint64_t* __restrict__ event_off) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n_regions) return;
    uint64_t v = 0;
    if (tiles && n_raw) {
        const uint64_t i = x.tile_raw_off[tile_off[r]];
        v = x.keep_off[i < n_raw ? x.head_off[i] : x.head_off[n_raw]];
    }
    event_off[r] = v;
}

// ---- indel events, left-aligned --------------------------------------------------------------------------------------------
struct InlArgs {
    const uint8_t* text;
    uint32_t max_shift;
};

// ind_tile_kernel with the shift between the walk and the window: one workgroup per tile, one thread per candidate record.
// A thread walks its record's operations from t0 on (inl_walk: not only up to t1, an event anchored behind the tile may land in
// it), shifts every raw event against the contig's text and keeps the one whose SHIFTED anchor a' lies in [t0, t1).  The
// candidate range [lo, hi) of the tile is still complete, and that is what the rule's bound a' >= pos is for: a record whose
// event lands in the tile has pos <= a' < t1 and end > a >= a' >= t0, so it overlaps the tile and lies in front of hi and not in
// front of lo.  The first step fails for most events, and it is the first thing the shift tests (two byte loads).  The emit pass
// takes the depth of a' from the tile's counters; k rides in the raw event's reserved word.
template <bool EMIT>
__global__ __launch_bounds__(kThreads) void inl_tile_kernel(const PlpArgs a, const PlpWork w, const IndWork x, const InlArgs L) {
    __shared__ uint32_t cnt[EMIT ? BG_PILEUP_COLS * BG_PILEUP_TILE : 1];
    __shared__ uint64_t range[2];
    __shared__ uint32_t wave_sum[kWaves];
    __shared__ uint32_t next;
    uint64_t first = 0;
    uint32_t room = 0;
    if (EMIT) {
        first = x.tile_raw_off[blockIdx.x];
        room = (uint32_t)(x.tile_raw_off[blockIdx.x + 1] - first);
        if (!room) return;  // (uniform)
    }
    const plp_tile_t t = plp_tile(blockIdx.x, a.regions, a.n_regions, w.tile_off, w.row_off);
    if (EMIT) {
        plp_count_tile<BG_PILEUP_COLS>(cnt, range, a, w, t);
        if (threadIdx.x == 0) next = 0;
    } else {
        if (threadIdx.x == 0) range[0] = plp_lo(w.end_max, a.n, t);
        if (threadIdx.x == 64) range[1] = plp_hi(w.pos_max, a.n, t);
    }
    __syncthreads();
    const uint64_t lo = range[0], hi = range[1];
    const bg_sam_contig_t contig = a.contigs[t.ref];
    const uint8_t* text = L.text + contig.start;
    uint32_t mine = 0;
    for (uint64_t s = lo + threadIdx.x; s < hi; s += kThreads) {
        if (!w.kept[s]) continue;
        const uint8_t* rec = a.recs + a.off[s];
        const uint32_t flag = bai_get16(rec + 18);
        inl_walk(rec, t.ref, t.t0, t.t1, L.max_shift, [&](uint32_t kind, uint32_t anchor, uint32_t len, uint32_t q, int64_t pos) {
            const uint32_t k = kind == BG_SITE_DEL ? inl_shift_del(text, (int64_t)contig.len, pos, anchor, len, L.max_shift)
                                                   : inl_shift_ins(text, pos, anchor, len, ind_seq_of(rec), q, L.max_shift);
            const int64_t at = (int64_t)anchor - k;
            if (at < t.t0 || at >= t.t1) return;
            if (EMIT) {
                const uint32_t place = atomicAdd(&next, 1u);
                if (place < room) {
                    ind_raw_t e = ind_raw(blockIdx.x, kind, (uint32_t)at, len, q, flag, ind_depth(cnt, (uint32_t)(at - t.t0)), s);
                    e.reserved = k;
                    x.raw[first + place] = e;
                }
            } else {
                mine++;
            }
        });
    }
    if (EMIT) return;
    for (int d = 32; d; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if (threadIdx.x % 64 == 0) wave_sum[threadIdx.x / 64] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (uint32_t k = 0; k < kWaves; k++) all += wave_sum[k];
        x.tile_raw[blockIdx.x] = all;
    }
}

// ind_head_kernel and ind_place_kernel through the shifted comparison and the shifted bytes
__global__ __launch_bounds__(256) void inl_head_kernel(uint64_t n_raw, const PlpArgs a, const IndWork x) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_raw) return;
    const ind_raw_t e = x.raw[x.order[i]];
    x.head[i] = i == 0 || inl_cmp(x.raw[x.order[i - 1]], e, a.recs, a.off) != 0;
    x.rev[i] = ind_rev(e);
}
__global__ __launch_bounds__(256) void inl_place_kernel(uint64_t n_raw, const PlpArgs a, const PlpWork w, const IndWork x, bg_bam_indel_t* __restrict__ events,
                                                        uint8_t* __restrict__ seq) {
    const uint64_t k = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / PLP_G;
    const uint32_t lane = threadIdx.x % PLP_G;
    if (k >= n_raw || !x.keep[k]) return;
    const uint32_t s = x.run_start[k], e = x.run_start[k + 1];
    const uint32_t rev = (uint32_t)(x.rev_off[e] - x.rev_off[s]);
    ind_raw_t v = x.raw[x.order[s]];
    if (lane == 0) {
        const plp_tile_t t = plp_tile(v.tile, a.regions, a.n_regions, w.tile_off, w.row_off);
        ind_store(ind_event(v, t.ref, t.region, e - s - rev, rev, x.seq_off[k]), events + x.keep_off[k]);
    }
    if (ind_kind(v) == BG_SITE_INS) inl_seq_lane(v, a.recs, a.off, seq + x.seq_off[k], lane, PLP_G);
}

int plp_check(const bg_ctx* ctx, const bg_bam_pileup_t* prm, uint64_t n_slots, const void* recs, const void* off, const void* contigs, uint64_t n_contigs,
              const void* regions, uint64_t n_regions, const void* rows, uint64_t rows_cap, uint64_t* n_rows, uint64_t* first_bad) {
    if (first_bad) *first_bad = UINT64_MAX;
    if (!ctx || !prm || !n_rows || (!rows && rows_cap) || (n_slots && (!recs || !off)) || (n_contigs && !contigs) || (n_regions && !regions))
        return BG_ERR_INVALID_ARG;
    *n_rows = 0;
    if ((prm->flags & ~(uint32_t)BG_PILEUP_STRANDS) || prm->reserved) return bg_refuse("bg_bam_pileup: unknown flag bits, or reserved is not 0");
    if (n_slots >= 0xFFFFFFFFull || n_regions >= (1ull << 24) || n_contigs > BAM_MAX_REF) return BG_ERR_TOO_LARGE;
    return BG_OK;
}

// Steps 1 to 3 of both entry points: the slot pass, the running maxima, the order check, the region pass, the two scans and the
// ONE read-back, then the refusals.  Scratch is ctx->aux: 33 bytes a slot and 24 a region.  The caller holds the scratch guard.
struct PlpFront {
    PlpWork w;
    uint64_t n_rows, tiles;
};
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

int sit_check(const bg_ctx* ctx, const bg_bam_sites_t* prm, uint64_t n_slots, const void* recs, const void* off, const void* contigs, uint64_t n_contigs,
              const void* text, uint64_t n_text, const void* regions, uint64_t n_regions, const void* sites, uint64_t sites_cap, uint64_t* n_sites,
              uint64_t* first_bad) {
    if (first_bad) *first_bad = UINT64_MAX;
    if (!ctx || !prm || !n_sites || (!sites && sites_cap) || (n_slots && (!recs || !off)) || (n_contigs && !contigs) || (n_regions && !regions) ||
        (n_text && !text))
        return BG_ERR_INVALID_ARG;
    *n_sites = 0;
    if (prm->flags || prm->reserved) return bg_refuse("bg_bam_sites: flags or reserved is not 0");
    if (prm->min_alt_permille > 1000) return bg_refuse("bg_bam_sites: min_alt_permille is above 1000");
    if (n_slots >= 0xFFFFFFFFull || n_regions >= (1ull << 24) || n_contigs > BAM_MAX_REF) return BG_ERR_TOO_LARGE;
    return BG_OK;
}

}  // namespace

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

namespace {

int ind_check(const bg_ctx* ctx, const bg_bam_indels_t* prm, uint64_t n_slots, const void* recs, const void* off, const void* contigs, uint64_t n_contigs,
              const void* regions, uint64_t n_regions, const void* events, uint64_t events_cap, const void* seq, uint64_t seq_cap, uint64_t* n_events,
              uint64_t* n_seq, uint64_t* first_bad) {
    if (first_bad) *first_bad = UINT64_MAX;
    if (!ctx || !prm || !n_events || !n_seq || (!events && events_cap) || (!seq && seq_cap) || (!events && seq) || (n_slots && (!recs || !off)) ||
        (n_contigs && !contigs) || (n_regions && !regions))
        return BG_ERR_INVALID_ARG;
    *n_events = 0;
    *n_seq = 0;
    if (prm->flags || prm->reserved) return bg_refuse("bg_bam_indels: flags or reserved is not 0");
    if (prm->min_alt_permille > 1000) return bg_refuse("bg_bam_indels: min_alt_permille is above 1000");
    if (n_slots >= 0xFFFFFFFFull || n_regions >= (1ull << 24) || n_contigs > BAM_MAX_REF) return BG_ERR_TOO_LARGE;
    return BG_OK;
}

// bg_bam_indels_dev and bg_bam_indels_left_dev behind their checks (LEFT: the inl_* kernels in steps 4 to 6 and 8, the regions'
// contigs held against the text, L the text and max_shift): the front (steps 1 to 3 of the pileup), then
//   4. the count pass, one workgroup per tile: the raw events anchored in the tile; a scan places the tiles; the SECOND
//      read-back gives the raw events;
//   5. the emit pass over the tiles that have raw events: the depth counters, the raw events into the tile's range of scratch;
//   6. a merge sort of their indices by the full key; heads of runs and strand bits, two scans; a run's start by its number;
//   7. a run's counts as differences of the scans, the verdict, the bytes of a kept insertion; two scans; the THIRD read-back
//      gives n_events and n_seq, and the sizing call ends here;
//   8. the records, the sequences and the regions' offsets out.
// Scratch: the front's lies in ctx->aux and must survive; 12 bytes a tile in ctx->tb; 88 bytes a raw event and the sort's own
// in ctx->bnd.
template <bool LEFT>
int ind_events_dev(bg_ctx* ctx, const bg_bam_indels_t* prm, const InlArgs& L, uint64_t n_text, uint64_t n_slots, const uint8_t* d_recs, const uint64_t* d_off,
                   const bg_sam_contig_t* d_contigs, uint64_t n_contigs, const bg_bam_region_t* d_regions, uint64_t n_regions, bg_bam_indel_t* d_events,
                   uint64_t events_cap, uint8_t* d_seq, uint64_t seq_cap, uint64_t* d_event_off, uint64_t* n_events, uint64_t* n_seq, uint64_t* first_bad,
                   void* stream) {
    int rc;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);
    const uint64_t nr = n_regions;
    const PlpArgs a = {n_slots, d_recs, d_off, d_contigs, n_contigs, d_regions, nr, ind_pileup_params(*prm), LEFT, LEFT ? n_text : 0};
    PlpFront f;
    if ((rc = plp_front(ctx, st, a, &f, first_bad))) return rc;
    const uint64_t tiles = f.tiles;
    const bool sizing = !d_events;
    IndWork x = {};
    uint64_t n_raw = 0;
    if (tiles && n_slots) {
        uint64_t *d_roff, *d_sums;
        if ((rc = bg_reserve_carved(&ctx->tb, &ctx->tb_bytes, [&](bg_carve& cv) {
            x.tile_raw = cv.take<uint32_t>(tiles);
            x.tile_raw_off = d_roff = cv.take<uint64_t>(tiles + 1);
            d_sums = cv.take<uint64_t>(bg_scan_sums_words(tiles));
        }))) return rc;
        // 4. the count pass
        if (LEFT) inl_tile_kernel<false><<<dim3((uint32_t)tiles), dim3(kThreads), 0, st>>>(a, f.w, x, L);
        else ind_tile_kernel<false><<<dim3((uint32_t)tiles), dim3(kThreads), 0, st>>>(a, f.w, x);
        BG_HIP(hipGetLastError());
        if ((rc = bg_scan_u32(x.tile_raw, tiles, d_roff, d_sums, st))) return rc;
        BG_HIP(hipMemcpyAsync(&n_raw, x.tile_raw_off + tiles, 8, hipMemcpyDeviceToHost, st));
        BG_HIP(hipStreamSynchronize(st));
    }
    if (n_raw >= (1ull << 32)) return BG_ERR_TOO_LARGE;
    uint64_t totals[2] = {0, 0};
    const int stop = ctx->indels_stop_after;  // (A/B: the passes told apart by whole calls)
    if (stop == 1) return BG_OK;
    if (n_raw) {
        const uint64_t n = n_raw;
        const rocprim::counting_iterator<uint32_t> iota(0);
        size_t t_sort = 0;
        BG_HIP(rocprim::merge_sort(nullptr, t_sort, iota, (uint32_t*)nullptr, n, IndOrder{nullptr, nullptr, nullptr}, st));
        uint64_t *d_tot, *d_sums;
        uint8_t* d_tmp;
        if ((rc = bg_reserve_carved(&ctx->bnd, &ctx->bnd_bytes, [&](bg_carve& cv) {
            x.raw = cv.take<ind_raw_t>(n);
            x.order = cv.take<uint32_t>(n), x.head = cv.take<uint32_t>(n), x.rev = cv.take<uint32_t>(n);
            x.head_off = cv.take<uint64_t>(n + 1), x.rev_off = cv.take<uint64_t>(n + 1);
            x.run_start = cv.take<uint32_t>(n + 1);
            x.keep = cv.take<uint32_t>(n), x.seq_len = cv.take<uint32_t>(n);
            x.keep_off = cv.take<uint64_t>(n + 1), x.seq_off = cv.take<uint64_t>(n + 1);
            d_tot = cv.take<uint64_t>(2);
            d_sums = cv.take<uint64_t>(bg_scan_sums_words(n));
            d_tmp = cv.take<uint8_t>(t_sort);
        }))) return rc;
        // 5. the emit pass
        if (LEFT) inl_tile_kernel<true><<<dim3((uint32_t)tiles), dim3(kThreads), 0, st>>>(a, f.w, x, L);
        else ind_tile_kernel<true><<<dim3((uint32_t)tiles), dim3(kThreads), 0, st>>>(a, f.w, x);
        BG_HIP(hipGetLastError());
        if (stop == 2) return BG_OK;
        // 6. the order, the runs
        size_t t = t_sort;
        if (LEFT) {
            if ((rc = inl_sort_raw(d_tmp, t, x.raw, d_recs, d_off, x.order, n, st))) return rc;
        } else {
            BG_HIP(rocprim::merge_sort(d_tmp, t, iota, x.order, n, IndOrder{x.raw, d_recs, d_off}, st));
        }
        if (stop == 3) return BG_OK;
        if (LEFT) inl_head_kernel<<<lanes(n), dim3(256), 0, st>>>(n, a, x);
        else ind_head_kernel<<<lanes(n), dim3(256), 0, st>>>(n, a, x);
        BG_HIP(hipGetLastError());
        if ((rc = bg_scan_u32(x.head, n, x.head_off, d_sums, st))) return rc;
        if ((rc = bg_scan_u32(x.rev, n, x.rev_off, d_sums, st))) return rc;
        ind_run_kernel<<<lanes(n + 1), dim3(256), 0, st>>>(n, x);
        // 7. the events
        ind_judge_kernel<<<lanes(n), dim3(256), 0, st>>>(n, *prm, x);
        BG_HIP(hipGetLastError());
        if ((rc = bg_scan_u32(x.keep, n, x.keep_off, d_sums, st))) return rc;
        if ((rc = bg_scan_u32(x.seq_len, n, x.seq_off, d_sums, st))) return rc;
        BG_HIP(hipMemcpyAsync(d_tot, x.keep_off + n, 8, hipMemcpyDeviceToDevice, st));
        BG_HIP(hipMemcpyAsync(d_tot + 1, x.seq_off + n, 8, hipMemcpyDeviceToDevice, st));
        BG_HIP(hipMemcpyAsync(totals, d_tot, 16, hipMemcpyDeviceToHost, st));
        BG_HIP(hipStreamSynchronize(st));
    }
    if (totals[0] >= (1ull << 32) || totals[1] >= (1ull << 32)) return BG_ERR_TOO_LARGE;
    *n_events = totals[0];
    *n_seq = totals[1];
    if (sizing) return BG_OK;
    if (totals[0] > events_cap || totals[1] > seq_cap) return BG_ERR_OPS_CAP;
    // 8. out
    if (d_event_off) {
        ind_region_off_kernel<<<lanes(nr + 1), dim3(256), 0, st>>>(nr, f.w.tile_off, tiles, n_raw, x, d_event_off);
        BG_HIP(hipGetLastError());
    }
    if (totals[0]) {
        if (LEFT) inl_place_kernel<<<lanes(n_raw * PLP_G), dim3(256), 0, st>>>(n_raw, a, f.w, x, d_events, d_seq);
        else ind_place_kernel<<<lanes(n_raw * PLP_G), dim3(256), 0, st>>>(n_raw, a, f.w, x, d_events, d_seq);
        BG_HIP(hipGetLastError());
    }
    return BG_OK;
}


}  // namespace

extern "C" int bg_bam_indels_dev(bg_ctx* ctx, const bg_bam_indels_t* prm, uint64_t n_slots, const uint8_t* d_recs, const uint64_t* d_off,
                                 const bg_sam_contig_t* d_contigs, uint64_t n_contigs, const bg_bam_region_t* d_regions, uint64_t n_regions,
                                 bg_bam_indel_t* d_events, uint64_t events_cap, uint8_t* d_seq, uint64_t seq_cap, uint64_t* d_event_off, uint64_t* n_events,
                                 uint64_t* n_seq, uint64_t* first_bad, void* stream) {
    int rc = ind_check(ctx, prm, n_slots, d_recs, d_off, d_contigs, n_contigs, d_regions, n_regions, d_events, events_cap, d_seq, seq_cap, n_events, n_seq,
                       first_bad);
    if (rc) return rc;
    if (((uintptr_t)d_events | (uintptr_t)d_event_off) & 7u) return bg_refuse("bg_bam_indels_dev: d_events or d_event_off is not 8-byte aligned");
    return ind_events_dev<false>(ctx, prm, InlArgs{nullptr, 0}, 0, n_slots, d_recs, d_off, d_contigs, n_contigs, d_regions, n_regions, d_events, events_cap, d_seq,
                                 seq_cap, d_event_off, n_events, n_seq, first_bad, stream);
}

extern "C" int bg_bam_indels(bg_ctx* ctx, const bg_bam_indels_t* prm, uint64_t n_slots, const uint8_t* recs, const uint64_t* off, const bg_sam_contig_t* contigs,
                             uint64_t n_contigs, const bg_bam_region_t* regions, uint64_t n_regions, bg_bam_indel_t* events, uint64_t events_cap, uint8_t* seq,
                             uint64_t seq_cap, uint64_t* event_off, uint64_t* n_events, uint64_t* n_seq, uint64_t* first_bad) {
    int rc = ind_check(ctx, prm, n_slots, recs, off, contigs, n_contigs, regions, n_regions, events, events_cap, seq, seq_cap, n_events, n_seq, first_bad);
    if (rc) return rc;
    // what no call on these records exceeds: an event takes four bytes of a record in every region, a sequence byte half a byte
    const uint64_t bytes = n_slots ? off[n_slots] : 0;
    const uint64_t cap = events ? std::min(events_cap, n_regions * (bytes / 4)) : 0, cap_seq = seq ? std::min(seq_cap, n_regions * bytes * 2) : 0;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_recs = s.up(recs, bytes);
    const uint64_t* d_off = s.up(off, n_slots ? n_slots + 1 : 0);
    const bg_sam_contig_t* d_contigs = s.up(contigs, n_contigs);
    const bg_bam_region_t* d_regions = s.up(regions, n_regions);
    bg_bam_indel_t* d_events = events ? s.out<bg_bam_indel_t>(cap) : nullptr;
    uint8_t* d_seq = seq ? s.out<uint8_t>(cap_seq) : nullptr;
    uint64_t* d_event_off = events && event_off ? s.out<uint64_t>(n_regions + 1) : nullptr;
    if (s.rc) return s.rc;
    if ((rc = bg_bam_indels_dev(ctx, prm, n_slots, d_recs, d_off, d_contigs, n_contigs, d_regions, n_regions, d_events, cap, d_seq, cap_seq, d_event_off,
                                n_events, n_seq, first_bad, s.st)))
        return rc;
    if (events) {
        s.down(events, d_events, *n_events);
        if (seq) s.down(seq, d_seq, *n_seq);
        if (event_off) s.down(event_off, d_event_off, n_regions + 1);
    }
    return s.sync();
}

namespace {

int inl_check(const bg_ctx* ctx, const bg_bam_indels_left_t* prm, const void* text, uint64_t n_text, bg_bam_indels_t* shared, uint64_t* n_events,
              uint64_t* n_seq, uint64_t* first_bad) {
    if (first_bad) *first_bad = UINT64_MAX;
    if (!ctx || !prm || !n_events || !n_seq || (n_text && !text)) return BG_ERR_INVALID_ARG;
    *shared = inl_indels_params(*prm);
    return BG_OK;
}

}  // namespace

// bg_bam_indels_left_dev: the checks of bg_bam_indels_dev and the text's, then ind_events_dev<true>
extern "C" int bg_bam_indels_left_dev(bg_ctx* ctx, const bg_bam_indels_left_t* prm, uint64_t n_slots, const uint8_t* d_recs, const uint64_t* d_off,
                                      const bg_sam_contig_t* d_contigs, uint64_t n_contigs, const uint8_t* d_text, uint64_t n_text,
                                      const bg_bam_region_t* d_regions, uint64_t n_regions, bg_bam_indel_t* d_events, uint64_t events_cap, uint8_t* d_seq,
                                      uint64_t seq_cap, uint64_t* d_event_off, uint64_t* n_events, uint64_t* n_seq, uint64_t* first_bad, void* stream) {
    bg_bam_indels_t shared;
    int rc = inl_check(ctx, prm, d_text, n_text, &shared, n_events, n_seq, first_bad);
    if (rc) return rc;
    if ((rc = ind_check(ctx, &shared, n_slots, d_recs, d_off, d_contigs, n_contigs, d_regions, n_regions, d_events, events_cap, d_seq, seq_cap, n_events, n_seq,
                        first_bad)))
        return rc;
    if (((uintptr_t)d_events | (uintptr_t)d_event_off) & 7u) return bg_refuse("bg_bam_indels_left_dev: d_events or d_event_off is not 8-byte aligned");
    return ind_events_dev<true>(ctx, &shared, InlArgs{d_text, prm->max_shift}, n_text, n_slots, d_recs, d_off, d_contigs, n_contigs, d_regions, n_regions, d_events,
                                events_cap, d_seq, seq_cap, d_event_off, n_events, n_seq, first_bad, stream);
}

extern "C" int bg_bam_indels_left(bg_ctx* ctx, const bg_bam_indels_left_t* prm, uint64_t n_slots, const uint8_t* recs, const uint64_t* off,
                                  const bg_sam_contig_t* contigs, uint64_t n_contigs, const uint8_t* text, uint64_t n_text, const bg_bam_region_t* regions,
                                  uint64_t n_regions, bg_bam_indel_t* events, uint64_t events_cap, uint8_t* seq, uint64_t seq_cap, uint64_t* event_off,
                                  uint64_t* n_events, uint64_t* n_seq, uint64_t* first_bad) {
    bg_bam_indels_t shared;
    int rc = inl_check(ctx, prm, text, n_text, &shared, n_events, n_seq, first_bad);
    if (rc) return rc;
    if ((rc = ind_check(ctx, &shared, n_slots, recs, off, contigs, n_contigs, regions, n_regions, events, events_cap, seq, seq_cap, n_events, n_seq, first_bad)))
        return rc;
    // the bounds of bg_bam_indels: a shift moves an event and makes none
    const uint64_t bytes = n_slots ? off[n_slots] : 0;
    const uint64_t cap = events ? std::min(events_cap, n_regions * (bytes / 4)) : 0, cap_seq = seq ? std::min(seq_cap, n_regions * bytes * 2) : 0;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_recs = s.up(recs, bytes);
    const uint64_t* d_off = s.up(off, n_slots ? n_slots + 1 : 0);
    const bg_sam_contig_t* d_contigs = s.up(contigs, n_contigs);
    const uint8_t* d_text = s.up(text, n_text);
    const bg_bam_region_t* d_regions = s.up(regions, n_regions);
    bg_bam_indel_t* d_events = events ? s.out<bg_bam_indel_t>(cap) : nullptr;
    uint8_t* d_seq = seq ? s.out<uint8_t>(cap_seq) : nullptr;
    uint64_t* d_event_off = events && event_off ? s.out<uint64_t>(n_regions + 1) : nullptr;
    if (s.rc) return s.rc;
    if ((rc = bg_bam_indels_left_dev(ctx, prm, n_slots, d_recs, d_off, d_contigs, n_contigs, d_text, n_text, d_regions, n_regions, d_events, cap, d_seq, cap_seq,
                                     d_event_off, n_events, n_seq, first_bad, s.st)))
        return rc;
    if (events) {
        s.down(events, d_events, *n_events);
        if (seq) s.down(seq, d_seq, *n_seq);
        if (event_off) s.down(event_off, d_event_off, n_regions + 1);
    }
    return s.sync();
}
