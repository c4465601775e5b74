// The bodies behind the candidate sites and region summaries (bam_sites.hip: bg_bam_sites[_dev]; THE RULE is in
// include/biogpu.h) as __host__ __device__ functions, so that the kernels and tests/bam_sites_host_bodies.cpp, which runs them
// on the CPU under AddressSanitizer, share ONE definition of what a position yields.  The counters are the pileup's
// (bam_pileup_rule.h), column-major in a tile: counter c of position p at c * BG_PILEUP_TILE + p.
//   * a region:    sit_region_ok: the pileup's check and the contig inside the text
//   * a position:  sit_judge: the 16 counters of a position against its reference byte: depth, the reference column, the
//                  candidates that are sites (a 5-bit mask in candidate order); sit_site: the record of one of them
//   * a share:     sit_share_t: what a run of positions adds to its region's summary; the five small counts (covered[0 .. 3],
//                  n_ref_other) and the number of sites ride in ONE 64-bit word, 10 bits each and 12 for the sites, which a
//                  tile of 512 positions and at most 2 560 sites cannot overflow; sit_share_pos, sit_share_join;
//                  sit_share_summary: the share as the 48-byte record a tile parks in scratch; sit_summary_stride,
//                  sit_summary_join, sit_summary_store: the reduction of a region's tiles
//   * placing:     sit_scan_pair / sit_scan_place: the two steps a thread takes around the scan of the 256 pair sums that
//                  turns the 512 per-position site counts into their exclusive offsets, in position order
//   * the records: sit_store: a record as two 16-byte stores or eight dwords
#ifndef BG_BAM_SITES_RULE_H
#define BG_BAM_SITES_RULE_H
#include "bam_pileup_rule.h"

#define SIT_W (2u * BG_PILEUP_COLS)  // the counters of a position: the BG_PILEUP_STRANDS form, always
static_assert(sizeof(bg_bam_sites_t) == 44 && sizeof(bg_bam_site_t) == 32 && sizeof(bg_bam_region_summary_t) == 48, "the boundary's structs");
static_assert(BG_PILEUP_TILE <= 1023 && 5 * BG_PILEUP_TILE <= 4095, "sit_share_t::packed: 10 bits a count, 12 for the sites");

SAM_HD bg_bam_pileup_t sit_pileup_params(const bg_bam_sites_t& p) {
    bg_bam_pileup_t q = {BG_PILEUP_STRANDS, p.require, p.exclude, p.min_mapq, p.min_baseq, 0};
    return q;
}

// ---- a region ---------------------------------------------------------------------------------------------------------------
// the pileup's check, and the region's contig inside [0, n_text)
SAM_HD bool sit_region_ok(const bg_bam_region_t& g, const bg_sam_contig_t* contigs, uint64_t n_contigs, uint64_t n_text) {
    if (!plp_region_ok(g, contigs, n_contigs)) return false;
    const bg_sam_contig_t c = contigs[g.ref];
    return c.start <= n_text && c.len <= n_text - c.start;
}

// ---- a position -------------------------------------------------------------------------------------------------------------
SAM_HD uint8_t sit_fold(uint8_t b) { return b >= 'a' && b <= 'z' ? (uint8_t)(b - 32) : b; }
SAM_HD int sit_ref_column(uint8_t folded) {
    return folded == 'A' ? (int)BG_PILEUP_A : folded == 'C' ? (int)BG_PILEUP_C : folded == 'G' ? (int)BG_PILEUP_G : folded == 'T' ? (int)BG_PILEUP_T : -1;
}
struct sit_pos_t {
    uint32_t depth, ref_count;
    uint64_t mismatch;  // the other three base columns, both strands
    uint8_t ref_base;   // folded
    int8_t ref_col;     // -1: unjudged
    uint8_t mask;       // bit k: candidate k (the three non-reference bases ascending, DEL, INS) is a site
    uint8_t n_sites;
};
SAM_HD bool sit_is_site(uint32_t fwd, uint32_t rev, uint32_t depth, const bg_bam_sites_t& p) {
    const uint64_t alt = (uint64_t)fwd + rev;
    return depth >= p.min_depth && alt >= (p.min_alt > 1 ? p.min_alt : 1u) && alt * 1000u >= (uint64_t)p.min_alt_permille * depth &&
           fwd >= p.min_alt_strand && rev >= p.min_alt_strand;
}
// the column of candidate k of a position whose reference column is ref_col
SAM_HD uint32_t sit_candidate_column(uint32_t k, int ref_col) {
    if (k == 3) return BG_PILEUP_DEL;
    if (k == 4) return BG_PILEUP_INS;
    return k + (k >= (uint32_t)ref_col);
}
// cnt: a tile's counters; i: the position's index in the tile
SAM_HD sit_pos_t sit_judge(const uint32_t* cnt, uint32_t i, uint8_t ref_byte, const bg_bam_sites_t& p) {
    sit_pos_t v;
    uint32_t both[BG_PILEUP_COLS];
    for (uint32_t c = 0; c < BG_PILEUP_COLS; c++) both[c] = cnt[c * BG_PILEUP_TILE + i] + cnt[(BG_PILEUP_COLS + c) * BG_PILEUP_TILE + i];
    v.depth = both[BG_PILEUP_A] + both[BG_PILEUP_C] + both[BG_PILEUP_G] + both[BG_PILEUP_T] + both[BG_PILEUP_OTHER] + both[BG_PILEUP_DEL];
    v.ref_base = sit_fold(ref_byte);
    v.ref_col = (int8_t)sit_ref_column(v.ref_base);
    v.ref_count = 0;
    v.mismatch = 0;
    v.mask = 0;
    v.n_sites = 0;
    if (v.ref_col < 0) return v;
    for (uint32_t c = 0; c <= BG_PILEUP_T; c++) {
        if (c == (uint32_t)v.ref_col) v.ref_count = both[c];
        else v.mismatch += both[c];
    }
    for (uint32_t k = 0; k < 5; k++) {
        const uint32_t c = sit_candidate_column(k, v.ref_col);
        if (sit_is_site(cnt[c * BG_PILEUP_TILE + i], cnt[(BG_PILEUP_COLS + c) * BG_PILEUP_TILE + i], v.depth, p)) {
            v.mask |= (uint8_t)(1u << k);
            v.n_sites++;
        }
    }
    return v;
}
SAM_HD bg_bam_site_t sit_site(const uint32_t* cnt, uint32_t i, const sit_pos_t& v, uint32_t k, uint32_t ref, int64_t pos, uint32_t region) {
    const uint32_t c = sit_candidate_column(k, v.ref_col);
    bg_bam_site_t s;
    s.ref = (int32_t)ref;
    s.pos = (int32_t)pos;
    s.region = region;
    s.kind = k == 3 ? BG_SITE_DEL : k == 4 ? BG_SITE_INS : BG_SITE_SNV;
    s.ref_base = v.ref_base;
    s.alt = k < 3 ? (uint8_t)"ACGT"[c] : 0;
    s.reserved = 0;
    s.depth = v.depth;
    s.ref_count = v.ref_count;
    s.alt_fwd = cnt[c * BG_PILEUP_TILE + i];
    s.alt_rev = cnt[(BG_PILEUP_COLS + c) * BG_PILEUP_TILE + i];
    return s;
}

// ---- a share of a region's summary ------------------------------------------------------------------------------------------
#define SIT_PACK_BITS 10u
#define SIT_PACK_SITES (5u * SIT_PACK_BITS)  // covered[0 .. 3] at bits 0, 10, 20, 30; n_ref_other at 40; the sites from 50
struct sit_share_t {
    uint64_t sum_depth, match, mismatch, packed;
    uint32_t max_depth;
};
SAM_HD sit_share_t sit_share_zero() {
    sit_share_t s = {0, 0, 0, 0, 0};
    return s;
}
SAM_HD void sit_share_pos(sit_share_t& s, const sit_pos_t& v, const bg_bam_sites_t& p) {
    s.sum_depth += v.depth;
    s.match += v.ref_count;
    s.mismatch += v.mismatch;
    for (uint32_t k = 0; k < 4; k++) s.packed += (uint64_t)(v.depth >= p.cover[k]) << (SIT_PACK_BITS * k);
    s.packed += (uint64_t)(v.ref_col < 0) << (SIT_PACK_BITS * 4);
    s.packed += (uint64_t)v.n_sites << SIT_PACK_SITES;
    s.max_depth = v.depth > s.max_depth ? v.depth : s.max_depth;
}
SAM_HD void sit_share_join(sit_share_t& s, const sit_share_t& o) {
    s.sum_depth += o.sum_depth;
    s.match += o.match;
    s.mismatch += o.mismatch;
    s.packed += o.packed;
    s.max_depth = o.max_depth > s.max_depth ? o.max_depth : s.max_depth;
}
SAM_HD uint32_t sit_share_count(const sit_share_t& s, uint32_t k) { return (uint32_t)(s.packed >> (SIT_PACK_BITS * k)) & ((1u << SIT_PACK_BITS) - 1u); }
SAM_HD uint32_t sit_share_sites(const sit_share_t& s) { return (uint32_t)(s.packed >> SIT_PACK_SITES); }
// a tile's share as the record the reduction over a region's tiles reads, and the joining of two such records
SAM_HD bg_bam_region_summary_t sit_share_summary(const sit_share_t& s) {
    bg_bam_region_summary_t r;
    r.sum_depth = s.sum_depth;
    r.match = s.match;
    r.mismatch = s.mismatch;
    for (uint32_t k = 0; k < 4; k++) r.covered[k] = sit_share_count(s, k);
    r.max_depth = s.max_depth;
    r.n_ref_other = sit_share_count(s, 4);
    return r;
}
SAM_HD void sit_summary_join(bg_bam_region_summary_t& a, const bg_bam_region_summary_t& b) {
    a.sum_depth += b.sum_depth;
    a.match += b.match;
    a.mismatch += b.mismatch;
    for (uint32_t k = 0; k < 4; k++) a.covered[k] += b.covered[k];
    a.max_depth = b.max_depth > a.max_depth ? b.max_depth : a.max_depth;
    a.n_ref_other += b.n_ref_other;
}
// Thread `thread` of `n_threads`: its part of the tiles [t0, t1) of a region
SAM_HD bg_bam_region_summary_t sit_summary_stride(const bg_bam_region_summary_t* tile_share, uint64_t t0, uint64_t t1, uint32_t thread, uint32_t n_threads) {
    bg_bam_region_summary_t r = {0, 0, 0, {0, 0, 0, 0}, 0, 0};
    for (uint64_t t = t0 + thread; t < t1; t += n_threads) sit_summary_join(r, tile_share[t]);
    return r;
}
// a summary out as twelve dwords: the caller's buffer is 4-byte aligned
SAM_HD void sit_summary_store(const bg_bam_region_summary_t& r, bg_bam_region_summary_t* dst) {
    const uint32_t w[12] = {(uint32_t)r.sum_depth, (uint32_t)(r.sum_depth >> 32), (uint32_t)r.match, (uint32_t)(r.match >> 32), (uint32_t)r.mismatch,
                            (uint32_t)(r.mismatch >> 32), r.covered[0], r.covered[1], r.covered[2], r.covered[3], r.max_depth, r.n_ref_other};
    for (uint32_t k = 0; k < 12; k++) ((uint32_t*)dst)[k] = w[k];
}

// ---- placing ----------------------------------------------------------------------------------------------------------------
// scan[0 .. BG_PILEUP_TILE): the site counts by position.  Thread t of BG_PILEUP_TILE / 2 returns the sum of its pair
// (2 t, 2 t + 1); with `ex`, the exclusive sum of the pairs in front of it, it then leaves the pair's exclusive offsets.
SAM_HD uint32_t sit_scan_pair(const uint32_t* scan, uint32_t t) { return scan[2 * t] + scan[2 * t + 1]; }
SAM_HD void sit_scan_place(uint32_t* scan, uint32_t t, uint32_t ex) {
    const uint32_t first = scan[2 * t];
    scan[2 * t] = ex;
    scan[2 * t + 1] = ex + first;
}

// ---- the records ------------------------------------------------------------------------------------------------------------
SAM_HD void sit_store(const bg_bam_site_t& s, bg_bam_site_t* dst, bool wide) {
    const uint32_t word3 = (uint32_t)s.kind | ((uint32_t)s.ref_base << 8) | ((uint32_t)s.alt << 16) | ((uint32_t)s.reserved << 24);
    const uint32_t w[8] = {(uint32_t)s.ref, (uint32_t)s.pos, s.region, word3, s.depth, s.ref_count, s.alt_fwd, s.alt_rev};
    if (wide) {
        const sam_v16 lo = {{w[0], w[1], w[2], w[3]}}, hi = {{w[4], w[5], w[6], w[7]}};
        ((sam_v16*)dst)[0] = lo;
        ((sam_v16*)dst)[1] = hi;
    } else {
        for (uint32_t k = 0; k < 8; k++) ((uint32_t*)dst)[k] = w[k];
    }
}

#endif
