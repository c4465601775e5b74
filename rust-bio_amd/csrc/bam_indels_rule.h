// The bodies behind the indel events (bam_indels.hip: bg_bam_indels[_dev]; THE RULE is in include/biogpu.h) as __host__
// __device__ functions, so that the kernels and tests/bam_indels_host_bodies.cpp, which runs them on the CPU under
// AddressSanitizer, share ONE definition of what a record yields and of how raw events become events.
//   * the walk:    ind_walk: the raw events of a kept record anchored inside a window, in the pileup's walk (r = pos, q = 0);
//                  ind_walk_pos: the same with the record's pos handed on, which bam_indels_left_rule.h's inl_walk is made of
//   * a raw event: ind_raw_t, 32 bytes in scratch: the tile, the anchor, kind, length, strand, the anchor's depth, and where
//                  the inserted codes lie (slot, q); ind_depth: the depth of a position from the 8-column counters of a tile
//   * the order:   ind_code: a 4-bit code of a record's bases; ind_cmp: the full key (tile, anchor, kind, len, codes left to
//                  right), exact for insertions of any length; ind_less / ind_same
//   * an event:    ind_is_kept: the four conditions of bg_bam_sites; ind_store: a record as five 8-byte stores; ind_seq_lane:
//                  a lane's share of the ASCII bytes of an insertion
#ifndef BG_BAM_INDELS_RULE_H
#define BG_BAM_INDELS_RULE_H
#include "bam_pileup_rule.h"

static_assert(sizeof(bg_bam_indels_t) == 28 && sizeof(bg_bam_indel_t) == 40, "the boundary's structs");

SAM_HD bg_bam_pileup_t ind_pileup_params(const bg_bam_indels_t& p) {
    bg_bam_pileup_t q = {0, p.require, p.exclude, p.min_mapq, p.min_baseq, 0};  // 8 columns: the depth sums both strands anyway
    return q;
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------
// The kept record rec (one that passed plp_slot): emit(kind, anchor, len, q, pos) for every raw event anchored in [t0, last) of
// `ref`.  q is the index of an insertion's first base (0 for a deletion), pos the record's.  Every byte read lies inside the record.
template <class Emit>
SAM_HD void ind_walk_pos(const uint8_t* rec, uint32_t ref, int64_t t0, int64_t last, Emit emit) {
    if (bai_get32(rec + 4) != ref) return;
    const int64_t pos = (int32_t)bai_get32(rec + 8);
    const uint32_t l_name = rec[12], n_cigar = bai_get16(rec + 16), l_seq = bai_get32(rec + 20);
    const uint8_t* cig = rec + BAM_FIXED + l_name;
    int64_t r = pos, q = 0;
    for (uint32_t k = 0; k < n_cigar && r <= last; k++) {  // (an event at r == last is anchored at last - 1)
        const uint32_t w = bai_get32(cig + 4ull * k), op = w & 15u;
        const int64_t n = w >> 4;
        const bool here = n >= 1 && r > pos && r - 1 >= t0 && r - 1 < last;
        if (op == BAM_CIGAR_M || op == BAM_CIGAR_EQ || op == BAM_CIGAR_X) {
            r += n;
            q += n;
        } else if (op == BAM_CIGAR_D) {
            if (here) emit((uint32_t)BG_SITE_DEL, (uint32_t)(r - 1), (uint32_t)n, 0u, pos);
            r += n;
        } else if (op == BAM_CIGAR_N) {
            r += n;
        } else if (op == BAM_CIGAR_I) {
            if (here && l_seq) emit((uint32_t)BG_SITE_INS, (uint32_t)(r - 1), (uint32_t)n, (uint32_t)q, pos);
            q += n;
        } else if (op == BAM_CIGAR_S) {
            q += n;
        }
    }
}
// emit(kind, anchor, len, q) for every raw event anchored in [t0, t1) of `ref`
template <class Emit>
SAM_HD void ind_walk(const uint8_t* rec, uint32_t ref, int64_t t0, int64_t t1, Emit emit) {
    ind_walk_pos(rec, ref, t0, t1, [&](uint32_t kind, uint32_t anchor, uint32_t len, uint32_t q, int64_t) { emit(kind, anchor, len, q); });
}

// ---- a raw event ------------------------------------------------------------------------------------------------------------
struct ind_raw_t {
    uint32_t tile;    // tiles ascend by (region, position)
    uint32_t anchor;
    uint32_t kind;    // BG_SITE_DEL or BG_SITE_INS in the low byte; bit 8: FLAG 0x10
    uint32_t len;
    uint32_t depth;   // of the anchor
    uint32_t slot;    // INS: the record that holds the codes ...
    uint32_t q;       // ... and the index of the first
    uint32_t reserved;
};
static_assert(sizeof(ind_raw_t) == 32, "32 bytes a raw event");
SAM_HD uint32_t ind_kind(const ind_raw_t& e) { return e.kind & 0xFFu; }
SAM_HD uint32_t ind_rev(const ind_raw_t& e) { return e.kind >> 8 & 1u; }
SAM_HD ind_raw_t ind_raw(uint32_t tile, uint32_t kind, uint32_t anchor, uint32_t len, uint32_t q, uint32_t flag, uint32_t depth, uint64_t slot) {
    const ind_raw_t e = {tile, anchor, kind | ((flag >> 4 & 1u) << 8), len, depth, (uint32_t)slot, q, 0};
    return e;
}
// cnt: the 8-column counters of a tile (no BG_PILEUP_STRANDS); i: the position's index in the tile
SAM_HD uint32_t ind_depth(const uint32_t* cnt, uint32_t i) {
    uint32_t d = 0;
    for (uint32_t c = 0; c <= BG_PILEUP_DEL; c++) d += cnt[c * BG_PILEUP_TILE + i];
    return d;
}

// ---- the order --------------------------------------------------------------------------------------------------------------
SAM_HD const uint8_t* ind_seq_of(const uint8_t* rec) { return rec + BAM_FIXED + rec[12] + 4ull * bai_get16(rec + 16); }
SAM_HD uint32_t ind_code(const uint8_t* seq, uint64_t j) { return (seq[j >> 1] >> ((j & 1u) ? 0 : 4)) & 15u; }
// < 0, 0, > 0 as a sorts before, with, behind b
SAM_HD int ind_cmp(const ind_raw_t& a, const ind_raw_t& b, const uint8_t* recs, const uint64_t* off) {
    if (a.tile != b.tile) return a.tile < b.tile ? -1 : 1;
    if (a.anchor != b.anchor) return a.anchor < b.anchor ? -1 : 1;
    const uint32_t ka = ind_kind(a), kb = ind_kind(b);
    if (ka != kb) return ka < kb ? -1 : 1;
    if (a.len != b.len) return a.len < b.len ? -1 : 1;
    if (ka != BG_SITE_INS || (a.slot == b.slot && a.q == b.q)) return 0;
    const uint8_t *sa = ind_seq_of(recs + off[a.slot]), *sb = ind_seq_of(recs + off[b.slot]);
    for (uint32_t j = 0; j < a.len; j++) {
        const uint32_t ca = ind_code(sa, (uint64_t)a.q + j), cb = ind_code(sb, (uint64_t)b.q + j);
        if (ca != cb) return ca < cb ? -1 : 1;
    }
    return 0;
}

// ---- an event ---------------------------------------------------------------------------------------------------------------
SAM_HD bool ind_is_kept(uint32_t fwd, uint32_t rev, uint32_t depth, const bg_bam_indels_t& p) {
    const uint64_t alt = (uint64_t)fwd + rev;
    return depth >= p.min_depth && alt >= (p.min_alt > 1 ? p.min_alt : 1u) && alt * 1000u >= (uint64_t)p.min_alt_permille * depth &&
           fwd >= p.min_alt_strand && rev >= p.min_alt_strand;
}
SAM_HD bg_bam_indel_t ind_event(const ind_raw_t& e, uint32_t ref, uint32_t region, uint32_t fwd, uint32_t rev, uint64_t seq_off) {
    bg_bam_indel_t v;
    v.ref = (int32_t)ref;
    v.pos = (int32_t)e.anchor;
    v.region = region;
    v.kind = (uint8_t)ind_kind(e);
    v.reserved[0] = v.reserved[1] = v.reserved[2] = 0;
    v.len = e.len;
    v.depth = e.depth;
    v.alt_fwd = fwd;
    v.alt_rev = rev;
    v.seq_off = seq_off;
    return v;
}
// dst is 8-byte aligned
SAM_HD void ind_store(const bg_bam_indel_t& v, bg_bam_indel_t* dst) {
    uint64_t* d = (uint64_t*)dst;
    d[0] = (uint64_t)(uint32_t)v.ref | ((uint64_t)(uint32_t)v.pos << 32);
    d[1] = (uint64_t)v.region | ((uint64_t)v.kind << 32);
    d[2] = (uint64_t)v.len | ((uint64_t)v.depth << 32);
    d[3] = (uint64_t)v.alt_fwd | ((uint64_t)v.alt_rev << 32);
    d[4] = v.seq_off;
}
// Lane `lane` of G: its bytes of the insertion e, ASCII, at dst[0 .. e.len)
SAM_HD void ind_seq_lane(const ind_raw_t& e, const uint8_t* recs, const uint64_t* off, uint8_t* dst, uint32_t lane, uint32_t G) {
    const uint8_t* seq = ind_seq_of(recs + off[e.slot]);
    for (uint32_t j = lane; j < e.len; j += G) dst[j] = (uint8_t)"=ACMGRSVTWYHKDBN"[ind_code(seq, (uint64_t)e.q + j)];
}

#endif
