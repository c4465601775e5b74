// Device functions shared by the reduction stages of seed-and-extend (one read or one pair per group of 16 lanes, on the
// pass view of seed_pass.h): the group reductions and their keys, the record of a hit, the best candidate away from a
// locus, and the MAPQ arithmetic of include/biogpu.h.  Each is stated once here.
#ifndef BG_SEED_RULE_H
#define BG_SEED_RULE_H
#include "seed_pass.h"

namespace bgseed {

// max of a 64-bit key over the 16 lanes of a group
__device__ __forceinline__ uint64_t max16(uint64_t v) {
#pragma unroll
    for (int o = 8; o; o >>= 1) {
        const uint64_t other = ((uint64_t)(uint32_t)__shfl_xor((int)(v >> 32), o, 16) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, o, 16);
        v = max(v, other);
    }
    return v;
}

// lane `src` of the group's value
__device__ __forceinline__ uint64_t bcast16(uint64_t v, uint32_t src) {
    return ((uint64_t)(uint32_t)__shfl((int)(v >> 32), (int)src, 16) << 32) | (uint32_t)__shfl((int)(uint32_t)v, (int)src, 16);
}

// The own-best key of candidate c of a read (numbered forward strand first): score biased to unsigned in the high word, ~c in
// the low one, so the max is the highest score and, among equals, the first candidate.  Never 0 for a candidate (c < 2 kMaxCand).
__device__ __forceinline__ uint64_t own_key(int32_t score, uint32_t c) { return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint32_t)~c; }
__device__ __forceinline__ int32_t key_score(uint64_t key) { return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u); }
__device__ __forceinline__ uint32_t key_cand(uint64_t key) { return ~(uint32_t)key; }

// a score alone as a key of max16; 0: none
__device__ __forceinline__ uint64_t score_key(int32_t s) { return (uint64_t)((uint32_t)s ^ 0x80000000u) | 1ull << 32; }
__device__ __forceinline__ int32_t score_of(uint64_t key) { return (int32_t)((uint32_t)key ^ 0x80000000u); }

// bg_pairq_params_t
struct PairqPrm {
    int32_t min_score;
    uint32_t mapq_cap;
};

// MAPQ of a placement with score s1 that is ahead by num (0 ..= s1): min(cap, cap * num / s1), 0 unless s1 > 0
__device__ __forceinline__ uint8_t mapq_of(uint32_t cap, uint64_t num, int64_t s1) {
    return s1 > 0 ? (uint8_t)min((uint64_t)cap, (uint64_t)cap * num / (uint64_t)s1) : 0;
}

// a read's candidates and the suffix-array rows its seeds resolved, as every slot of the read reports them
struct ReadCounts {
    uint32_t n_candidates, n_seed_hits;
};

// the record of a slot without a hit (an unmapped read), its empty operations ending at ops_off
__device__ __forceinline__ bg_seed_hit_t unmapped_hit(uint32_t nc, uint32_t nsh, uint64_t ops_off) {
    bg_seed_hit_t h;
    memset(&h, 0, sizeof(h));
    h.aln.score = BG_MIN_SCORE;
    h.window_start = h.ref_start = h.ref_end = ~0ull;
    h.n_candidates = nc;
    h.n_seed_hits = nsh;
    h.aln.ops_off = ops_off;
    return h;
}

// Slot `slot` of O.hits / O.strand / O.ops, by the 16 lanes of a group.  won = BG_HIT_FORWARD / BG_HIT_REVERSE: alignment `a`
// against the window at text offset `window`, its operations (at src_ops + a.ops_off) right-aligned in the slot; won =
// BG_HIT_NONE: the slot of an unmapped read (a, window and src_ops are not read).
__device__ __forceinline__ void write_hit(const SeedOut& O, uint64_t slot, uint32_t l16, const bg_alignment_t* a, uint64_t window,
                                          const uint8_t* src_ops, uint8_t won, ReadCounts n) {
    bg_seed_hit_t h = unmapped_hit(n.n_candidates, n.n_seed_hits, (slot + 1) * O.ops_stride);
    if (won != BG_HIT_NONE) {
        h.aln = *a;
        h.aln.ops_off = (slot + 1) * O.ops_stride - h.aln.n_ops;
        h.window_start = window;
        h.ref_start = window + h.aln.ystart;
        h.ref_end = window + h.aln.yend;
        if (O.ops && src_ops) {
            const uint64_t from = a->ops_off;
            for (uint32_t i = l16; i < h.aln.n_ops; i += 16) O.ops[h.aln.ops_off + i] = src_ops[from + i];
        }
    }
    if (l16 == 0) {
        O.hits[slot] = h;
        if (O.strand) O.strand[slot] = won;
    }
}

// candidate c of the pass (absolute) into a slot
__device__ __forceinline__ void write_cand(const SeedPass& P, const SeedOut& O, uint64_t slot, uint32_t l16, uint64_t c, uint8_t won,
                                           uint32_t nc, uint32_t nsh) {
    write_hit(O, slot, l16, won != BG_HIT_NONE ? &P.aln[c] : nullptr, won != BG_HIT_NONE ? P.w_lo[c] : 0, P.c_ops, won, ReadCounts{nc, nsh});
}

// Over candidates c0 .. c0 + nc of the pass, strided over the group's lanes: the best score (as a score_key; 0: none) among
// those scoring >= min_score whose text interval does not touch [lo, hi].
__device__ __forceinline__ uint64_t best_elsewhere(const SeedPass& P, uint32_t l16, uint64_t c0, uint32_t nc, uint64_t lo, uint64_t hi,
                                                   int32_t min_score) {
    uint64_t best = 0;
    for (uint32_t c = l16; c < nc; c += 16) {
        const bg_alignment_t& a = P.aln[c0 + c];
        const int32_t score = a.score;
        const uint64_t x_lo = P.w_lo[c0 + c] + a.ystart, x_hi = P.w_lo[c0 + c] + a.yend;
        if (score < min_score || (x_lo <= hi && lo <= x_hi)) continue;
        best = max(best, score_key(score));
    }
    return max16(best);
}

}  // namespace bgseed

#endif
