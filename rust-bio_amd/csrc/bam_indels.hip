// Indel events: deletions by length and insertions by sequence, per anchor (bg_bam_indels[_dev] and bg_bam_indels_left[_dev]; THE
// RULE is in include/biogpu.h, the bodies in bam_indels_rule.h and bam_indels_left_rule.h).  They share steps 1 to 3 of the pileup
// (plp_front, bam_pileup.hip) and the counting of step 4 (plp_count_tile, bam_pileup_front.h) and keep what the pileup's walk
// reads and drops, an operation's length and the inserted bases: a count pass and an emit pass over the tiles leave the raw
// events in scratch, a merge sort orders them by the full key, heads of runs and prefix sums of the strand bits make them events
// (the steps are listed at ind_events_dev).
// The left-aligned call is the plain one with a shift of every raw event against the reference text between the walk and the
// window, the sort and the placement through the shifted codes: the kernels that differ take the flavour as a template argument
// (LEFT), and its merge sort is instantiated in bam_indels_left_sort.hip.
#include <algorithm>

#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "bam_pileup_front.h"
#include "bam_indels_left_rule.h"

// bam_indels_left_sort.hip: the merge sort of the left-aligned raw events by inl_cmp, kept out of this file so that the kernels of
// bg_bam_indels_dev's sort are compiled as they were (the reason is written there)
int inl_sort_raw(void* d_tmp, size_t tmp_bytes, const ind_raw_t* raw, const uint8_t* recs, const uint64_t* off, uint32_t* order, uint64_t n, hipStream_t st);

namespace {

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

struct InlArgs {  // what the left-aligned flavour adds; the plain one's kernels read none of it
    const uint8_t* text;
    uint32_t max_shift;
};

// The emit pass's raw event of slot s, anchored at `anchor` of tile t behind k steps to the left: it takes the next place of the
// tile's range [first, first + room) of scratch from the counter in LDS, with the anchor's depth from the tile's counters; k
// rides in the reserved word (0 where nothing shifts).
__device__ __forceinline__ void ind_emit(const IndWork& x, uint64_t first, uint32_t room, uint32_t* next, const uint32_t* cnt, const plp_tile_t& t, uint32_t kind,
                                         uint32_t anchor, uint32_t len, uint32_t q, uint32_t flag, uint64_t s, uint32_t k) {
    const uint32_t place = atomicAdd(next, 1u);
    if (place >= room) return;
    ind_raw_t e = ind_raw(blockIdx.x, kind, anchor, len, q, flag, ind_depth(cnt, anchor - (uint32_t)t.t0), s);
    e.reserved = k;  // (the plain flavour hands k = 0, which is what ind_raw leaves there: its raw events are bg_bam_indels_dev's as they were)
    x.raw[first + place] = e;
}

// One workgroup per tile, one thread per candidate record.  The count pass (EMIT false) leaves the tile's number of raw events.
// The emit pass runs in the tiles that have some: the 8-column counters of the tile for the depth of the anchors, then the same
// walk again; a raw event takes the next place of the tile's range of scratch (ind_emit), so the order inside the range is that
// of arrival and everything behind this pass is independent of it.
// LEFT puts the shift between the walk and the window.  A thread walks its record's operations from t0 on (inl_walk: not only up
// to t1, an event anchored behind the tile may land in it), shifts every raw event against the contig's text and keeps the one
// whose SHIFTED anchor a' lies in [t0, t1).  The candidate range [lo, hi) of the tile is still complete, and that is what the
// rule's bound a' >= pos is for: a record whose event lands in the tile has pos <= a' < t1 and end > a >= a' >= t0, so it overlaps
// the tile and lies in front of hi and not in front of lo.  The first step fails for most events, and it is the first thing the
// shift tests (two byte loads).  The emit pass takes the depth of a'.
template <bool EMIT, bool LEFT>
__global__ __launch_bounds__(kThreads) void ind_tile_kernel(const PlpArgs a, const PlpWork w, const IndWork x, const InlArgs L) {
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
    } else {  // (the two searches of plp_count_tile, which says why they stand twice)
        if (threadIdx.x == 0) range[0] = plp_lo(w.end_max, a.n, t);
        if (threadIdx.x == 64) range[1] = plp_hi(w.pos_max, a.n, t);
    }
    __syncthreads();
    const uint64_t lo = range[0], hi = range[1];
    const uint8_t* text = nullptr;
    int64_t clen = 0;
    if constexpr (LEFT) {
        const bg_sam_contig_t contig = a.contigs[t.ref];
        text = L.text + contig.start;
        clen = (int64_t)contig.len;
    }
    uint32_t mine = 0;
    for (uint64_t s = lo + threadIdx.x; s < hi; s += kThreads) {
        if (!w.kept[s]) continue;
        const uint8_t* rec = a.recs + a.off[s];
        const uint32_t flag = bai_get16(rec + 18);
        const auto take = [&](uint32_t kind, uint32_t anchor, uint32_t len, uint32_t q, uint32_t k) {
            if (EMIT) ind_emit(x, first, room, &next, cnt, t, kind, anchor, len, q, flag, s, k);
            else mine++;
        };
        if constexpr (LEFT) {
            inl_walk(rec, t.ref, t.t0, t.t1, L.max_shift, [&](uint32_t kind, uint32_t anchor, uint32_t len, uint32_t q, int64_t pos) {
                const uint32_t k = kind == BG_SITE_DEL ? inl_shift_del(text, clen, pos, anchor, len, L.max_shift)
                                                       : inl_shift_ins(text, pos, anchor, len, ind_seq_of(rec), q, L.max_shift);
                const int64_t at = (int64_t)anchor - k;
                if (at >= t.t0 && at < t.t1) take(kind, (uint32_t)at, len, q, k);
            });
        } else {
            ind_walk(rec, t.ref, t.t0, t.t1, [&](uint32_t kind, uint32_t anchor, uint32_t len, uint32_t q) { take(kind, anchor, len, q, 0u); });
        }
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

// sorted index i: does a run begin here (LEFT: by the shifted comparison), and the strand bit
template <bool LEFT>
__global__ __launch_bounds__(256) void ind_head_kernel(uint64_t n_raw, const PlpArgs a, const IndWork x) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_raw) return;
    const ind_raw_t e = x.raw[x.order[i]];
    if constexpr (LEFT) x.head[i] = i == 0 || inl_cmp(x.raw[x.order[i - 1]], e, a.recs, a.off) != 0;
    else x.head[i] = i == 0 || ind_cmp(x.raw[x.order[i - 1]], e, a.recs, a.off) != 0;
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
// PLP_G lanes a run: a kept event's record, and the bytes of a kept insertion (LEFT: the shifted bytes)
template <bool LEFT>
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
    if (ind_kind(v) != BG_SITE_INS) return;
    if constexpr (LEFT) inl_seq_lane(v, a.recs, a.off, seq + x.seq_off[k], lane, PLP_G);
    else ind_seq_lane(v, a.recs, a.off, seq + x.seq_off[k], lane, PLP_G);
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

int ind_check(const bg_ctx* ctx, const bg_bam_indels_t* prm, uint64_t n_slots, const void* recs, const void* off, const void* contigs, uint64_t n_contigs,
              const void* regions, uint64_t n_regions, const void* events, uint64_t events_cap, const void* seq, uint64_t seq_cap, uint64_t* n_events,
              uint64_t* n_seq, uint64_t* first_bad) {
    const bool own_ok = n_events && n_seq && (events || !events_cap) && (seq || !seq_cap) && (events || !seq);
    return plp_check_args(ctx, prm, n_slots, recs, off, contigs, n_contigs, regions, n_regions, first_bad, own_ok, [&] {
        *n_events = 0;
        *n_seq = 0;
        if (prm->flags || prm->reserved) return bg_refuse("bg_bam_indels: flags or reserved is not 0");
        if (prm->min_alt_permille > 1000) return bg_refuse("bg_bam_indels: min_alt_permille is above 1000");
        return (int)BG_OK;
    });
}
// the left-aligned call's own: the text, and its parameters as the plain call's for ind_check
int inl_check(const bg_ctx* ctx, const bg_bam_indels_left_t* prm, const void* text, uint64_t n_text, bg_bam_indels_t* shared, uint64_t* n_events,
              uint64_t* n_seq, uint64_t* first_bad) {
    if (first_bad) *first_bad = UINT64_MAX;
    if (!ctx || !prm || !n_events || !n_seq || (n_text && !text)) return BG_ERR_INVALID_ARG;
    *shared = inl_indels_params(*prm);
    return BG_OK;
}

// bg_bam_indels_dev and bg_bam_indels_left_dev behind their checks (LEFT: the kernels' left flavour in steps 4 to 6 and 8, the
// regions' contigs held against the text, L the text and max_shift): the front (steps 1 to 3 of the pileup), then
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
        ind_tile_kernel<false, LEFT><<<dim3((uint32_t)tiles), dim3(kThreads), 0, st>>>(a, f.w, x, L);
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
        ind_tile_kernel<true, LEFT><<<dim3((uint32_t)tiles), dim3(kThreads), 0, st>>>(a, f.w, x, L);
        BG_HIP(hipGetLastError());
        if (stop == 2) return BG_OK;
        // 6. the order (each flavour's sort in its own translation unit), the runs
        size_t t = t_sort;
        if (LEFT) {
            if ((rc = inl_sort_raw(d_tmp, t, x.raw, d_recs, d_off, x.order, n, st))) return rc;
        } else {
            BG_HIP(rocprim::merge_sort(d_tmp, t, iota, x.order, n, IndOrder{x.raw, d_recs, d_off}, st));
        }
        if (stop == 3) return BG_OK;
        ind_head_kernel<LEFT><<<lanes(n), dim3(256), 0, st>>>(n, a, x);
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
        ind_place_kernel<LEFT><<<lanes(n_raw * PLP_G), dim3(256), 0, st>>>(n_raw, a, f.w, x, d_events, d_seq);
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

namespace {

// bg_bam_indels (left null: no text is staged) and bg_bam_indels_left behind their checks: the host buffers up, the device call,
// the results down.  The capacities are bounded by what no call on these records exceeds: an event takes four bytes of a record in
// every region, a sequence byte half a byte; a shift moves an event and makes none.
int ind_events_host(bg_ctx* ctx, const bg_bam_indels_t* prm, const bg_bam_indels_left_t* left, uint64_t n_slots, const uint8_t* recs, const uint64_t* off,
                    const bg_sam_contig_t* contigs, uint64_t n_contigs, const uint8_t* text, uint64_t n_text, const bg_bam_region_t* regions, uint64_t n_regions,
                    bg_bam_indel_t* events, uint64_t events_cap, uint8_t* seq, uint64_t seq_cap, uint64_t* event_off, uint64_t* n_events, uint64_t* n_seq,
                    uint64_t* first_bad) {
    const uint64_t bytes = n_slots ? off[n_slots] : 0;
    const uint64_t cap = events ? std::min(events_cap, n_regions * (bytes / 4)) : 0, cap_seq = seq ? std::min(seq_cap, n_regions * bytes * 2) : 0;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_recs = s.up(recs, bytes);
    const uint64_t* d_off = s.up(off, n_slots ? n_slots + 1 : 0);
    const bg_sam_contig_t* d_contigs = s.up(contigs, n_contigs);
    const uint8_t* d_text = left ? s.up(text, n_text) : nullptr;
    const bg_bam_region_t* d_regions = s.up(regions, n_regions);
    bg_bam_indel_t* d_events = events ? s.out<bg_bam_indel_t>(cap) : nullptr;
    uint8_t* d_seq = seq ? s.out<uint8_t>(cap_seq) : nullptr;
    uint64_t* d_event_off = events && event_off ? s.out<uint64_t>(n_regions + 1) : nullptr;
    if (s.rc) return s.rc;
    const int rc = left ? bg_bam_indels_left_dev(ctx, left, n_slots, d_recs, d_off, d_contigs, n_contigs, d_text, n_text, d_regions, n_regions, d_events, cap, d_seq,
                                                 cap_seq, d_event_off, n_events, n_seq, first_bad, s.st)
                        : bg_bam_indels_dev(ctx, prm, n_slots, d_recs, d_off, d_contigs, n_contigs, d_regions, n_regions, d_events, cap, d_seq, cap_seq, d_event_off,
                                            n_events, n_seq, first_bad, s.st);
    if (rc) return rc;
    if (events) {
        s.down(events, d_events, *n_events);
        if (seq) s.down(seq, d_seq, *n_seq);
        if (event_off) s.down(event_off, d_event_off, n_regions + 1);
    }
    return s.sync();
}

}  // namespace

extern "C" int bg_bam_indels(bg_ctx* ctx, const bg_bam_indels_t* prm, uint64_t n_slots, const uint8_t* recs, const uint64_t* off, const bg_sam_contig_t* contigs,
                             uint64_t n_contigs, const bg_bam_region_t* regions, uint64_t n_regions, bg_bam_indel_t* events, uint64_t events_cap, uint8_t* seq,
                             uint64_t seq_cap, uint64_t* event_off, uint64_t* n_events, uint64_t* n_seq, uint64_t* first_bad) {
    int rc = ind_check(ctx, prm, n_slots, recs, off, contigs, n_contigs, regions, n_regions, events, events_cap, seq, seq_cap, n_events, n_seq, first_bad);
    if (rc) return rc;
    return ind_events_host(ctx, prm, nullptr, n_slots, recs, off, contigs, n_contigs, nullptr, 0, regions, n_regions, events, events_cap, seq, seq_cap, event_off,
                           n_events, n_seq, first_bad);
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
    return ind_events_host(ctx, &shared, prm, n_slots, recs, off, contigs, n_contigs, text, n_text, regions, n_regions, events, events_cap, seq, seq_cap, event_off,
                           n_events, n_seq, first_bad);
}
