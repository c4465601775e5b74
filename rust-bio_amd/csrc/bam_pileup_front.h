// What the calls over a pileup's tiles share (bg_bam_pileup[_dev] in bam_pileup.hip, bg_bam_sites[_dev] in bam_sites.hip,
// bg_bam_indels[_dev] and bg_bam_indels_left[_dev] in bam_indels.hip): the call's arguments and the front's scratch as the kernels
// take them, the argument check, the front (plp_front: steps 1 to 3 of the pileup, defined with its kernels in bam_pileup.hip and
// compiled there once), and the counting of a tile as a device function every tile kernel inlines.
#ifndef BG_BAM_PILEUP_FRONT_H
#define BG_BAM_PILEUP_FRONT_H
#include "bg_common.h"
#include "bam_pileup_rule.h"

constexpr uint32_t kThreads = 256;  // of a tile's workgroup
constexpr uint32_t kWaves = kThreads / 64;

struct PlpArgs {
    uint64_t n;  // slots
    const uint8_t* recs;
    const uint64_t* off;
    const bg_sam_contig_t* contigs;
    uint64_t n_contigs;
    const bg_bam_region_t* regions;
    uint64_t n_regions;
    bg_bam_pileup_t prm;
    bool in_text;     // bg_bam_sites, bg_bam_indels_left: a region's contig must lie inside [0, n_text)
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

// The checks every call of the family makes, in the order the status codes imply: first_bad reset; a null pointer among the
// shared arguments, or `own_ok` false (the call's own pointers, tested by the caller without a load), is BG_ERR_INVALID_ARG;
// then `own` zeroes the call's outputs and refuses its flags and thresholds (non-zero: that status); then the three size limits.
template <class Own>
int plp_check_args(const bg_ctx* ctx, const void* prm, uint64_t n_slots, const void* recs, const void* off, const void* contigs, uint64_t n_contigs,
                   const void* regions, uint64_t n_regions, uint64_t* first_bad, bool own_ok, Own own) {
    if (first_bad) *first_bad = UINT64_MAX;
    if (!ctx || !prm || !own_ok || (n_slots && (!recs || !off)) || (n_contigs && !contigs) || (n_regions && !regions)) return BG_ERR_INVALID_ARG;
    if (const int rc = own()) return rc;
    if (n_slots >= 0xFFFFFFFFull || n_regions >= (1ull << 24) || n_contigs > BAM_MAX_REF) return BG_ERR_TOO_LARGE;
    return BG_OK;
}

// Steps 1 to 3 of every entry point: the slot pass, the running maxima, the order check, the region pass, the two scans and the
// ONE read-back, then the refusals.  Scratch is ctx->aux: 33 bytes a slot and 24 a region.  The caller holds the scratch guard.
struct PlpFront {
    PlpWork w;
    uint64_t n_rows, tiles;
};
int plp_front(bg_ctx* ctx, hipStream_t st, const PlpArgs& a, PlpFront* f, uint64_t* first_bad);

// A tile's counters, by all the threads of its workgroup: cnt zeroed, the candidate slots [lo, hi) by two binary searches in the
// running maxima (lo: the first slot whose end maximum exceeds (ref, t0); hi: the first whose key is >= (ref, t1)) in two threads
// of different waves, every kept one walked by a group of PLP_G lanes striding over the positions of an operation inside the tile
// (LDS adds whose value is not used: ds_add_u32), a barrier.  W: the columns counted (SIT_W under BG_PILEUP_STRANDS).
// The two searches stand once more in the count pass of bam_indels.hip's tile kernel, which counts nothing.  A device function
// for the two lines was tried and taken out again: behind it the compiler lays the two branches out otherwise, and the count
// kernels no longer had their registers (profiles/bam_pileup_split_resources.txt).
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

#endif
