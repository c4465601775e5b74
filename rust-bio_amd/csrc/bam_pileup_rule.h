// The bodies behind the pileup (bam_pileup.hip: bg_bam_pileup[_dev]; THE RULE is in include/biogpu.h) as __host__ __device__
// functions, so that the kernels and tests/bam_pileup_host_bodies.cpp, which runs them on the CPU under AddressSanitizer,
// share ONE definition of what a record is checked for and of every counter it touches.
//   * a slot:     plp_slot: bai_decode, the checks of the pileup's own (operation codes, the query lengths against l_seq, the
//                 CG placeholder), the kept verdict, the two keys the searches run on
//   * a region:   plp_region_ok, plp_tiles; plp_tile: the region, the window and the output row of a tile
//   * a window:   plp_first_above / plp_first_from: the candidate slots [lo, hi) of a window, two binary searches in the
//                 running maxima of the keys
//   * the walk:   plp_walk_lane: a lane's share of a record's counts inside a window, every operation clipped to the window by
//                 arithmetic; the counters are column-major (counter c of position p at c * BG_PILEUP_TILE + p)
//   * the rows:   plp_store_rows: a thread's share of a tile's rows, transposed, 16 bytes wide or dword by dword
#ifndef BG_BAM_PILEUP_RULE_H
#define BG_BAM_PILEUP_RULE_H
#include "bam_index_rule.h"

#define BG_PILEUP_TILE 512u  // positions of a tile: 16 columns x 512 x 4 bytes = 32 KB of LDS, so four workgroups fit a CU's 160 KB
#define PLP_G 16u            // lanes that share a record
#define PLP_MAX_OP 9u        // codes 0 .. 8 are MIDNSHP=X; 9 (htslib's B) is taken and consumes nothing
enum { BAM_CIGAR_M = 0 };

// ---- a slot -----------------------------------------------------------------------------------------------------------------
struct plp_slot_t {
    uint64_t pos_key;  // ((uint32) refID, pos + 1): what the input must ascend by; 0 for an empty slot
    uint64_t end_key;  // bai_end_key: ((uint32) refID, end); 0 for an empty slot
    uint8_t kept;
};
SAM_HD uint64_t plp_pos_key(int32_t ref, int32_t pos) { return ((uint64_t)(uint32_t)ref << 32) | (uint32_t)(pos + 1); }
SAM_HD bool plp_kept(const bai_rec_t& r, uint32_t flag, uint32_t mapq, const bg_bam_pileup_t& p) {
    return r.ref >= 0 && r.pos >= 0 && !(flag & 4u) && (flag & p.require) == p.require && (flag & p.exclude) == 0 && mapq >= p.min_mapq;
}
// The record rec[0 .. len), len > 0: BAI_OK, BAI_INVALID or BAI_UNSUPPORTED (a record is UNSUPPORTED only if nothing about it
// is INVALID), and *s.  Reads no byte outside the record.
SAM_HD int plp_slot(const uint8_t* rec, uint64_t len, const bg_sam_contig_t* contigs, uint64_t n_contigs, const bg_bam_pileup_t& prm, plp_slot_t* s) {
    bai_rec_t r;
    const int kind = bai_decode(rec, len, contigs, n_contigs, &r);
    s->pos_key = plp_pos_key(r.ref, r.pos);
    s->end_key = bai_end_key(r);
    s->kept = 0;
    if (kind == BAI_INVALID) return kind;
    const uint32_t l_name = rec[12], mapq = rec[13], n_cigar = bai_get16(rec + 16), flag = bai_get16(rec + 18), l_seq = bai_get32(rec + 20);
    const uint8_t* cig = rec + BAM_FIXED + l_name;
    uint64_t query = 0;
    for (uint32_t k = 0; k < n_cigar; k++) {
        const uint32_t w = bai_get32(cig + 4ull * k), op = w & 15u;
        if (op > PLP_MAX_OP) return BAI_INVALID;
        if (op == BAM_CIGAR_M || op == BAM_CIGAR_I || op == BAM_CIGAR_S || op == BAM_CIGAR_EQ || op == BAM_CIGAR_X) query += w >> 4;
    }
    if (n_cigar && l_seq && query != l_seq) return BAI_INVALID;
    if (kind) return kind;
    if (r.ref >= 0 && n_cigar == 2) {
        const uint32_t w0 = bai_get32(cig), w1 = bai_get32(cig + 4);
        if (w0 == ((l_seq << 4) | BAM_CIGAR_S) && (w1 & 15u) == BAM_CIGAR_N) return BAI_UNSUPPORTED;
    }
    s->kept = plp_kept(r, flag, mapq, prm);
    return BAI_OK;
}

// ---- regions and tiles ------------------------------------------------------------------------------------------------------
SAM_HD bool plp_region_ok(const bg_bam_region_t& g, const bg_sam_contig_t* contigs, uint64_t n_contigs) {
    return g.ref >= 0 && (uint64_t)g.ref < n_contigs && g.beg >= 0 && g.beg <= g.end && (uint64_t)g.end <= contigs[g.ref].len;
}
SAM_HD uint32_t plp_tiles(uint32_t len) { return len / BG_PILEUP_TILE + (len % BG_PILEUP_TILE != 0); }
struct plp_tile_t {
    uint32_t ref;
    int64_t t0, t1;  // the window: positions [t0, t1) of ref, at most BG_PILEUP_TILE
    uint64_t row;    // the row of position t0
    uint32_t region;
};
// tile_off / row_off: the exclusive sums of the regions' tile counts and lengths (n_regions + 1 entries each); tile < tile_off[n_regions]
SAM_HD plp_tile_t plp_tile(uint64_t tile, const bg_bam_region_t* regions, uint64_t n_regions, const uint64_t* tile_off, const uint64_t* row_off) {
    uint64_t lo = 0, hi = n_regions - 1;  // the first r with tile_off[r + 1] > tile
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (tile_off[mid + 1] > tile) hi = mid;
        else lo = mid + 1;
    }
    const bg_bam_region_t g = regions[lo];
    const uint64_t first = (tile - tile_off[lo]) * BG_PILEUP_TILE;
    plp_tile_t t;
    t.ref = (uint32_t)g.ref;
    t.t0 = (int64_t)g.beg + (int64_t)first;
    t.t1 = t.t0 + BG_PILEUP_TILE < g.end ? t.t0 + BG_PILEUP_TILE : g.end;
    t.row = row_off[lo] + first;
    t.region = (uint32_t)lo;
    return t;
}

// ---- a window's candidates --------------------------------------------------------------------------------------------------
// m[0 .. n) ascends.  The first j with m[j] > want / m[j] >= want; n where there is none.
SAM_HD uint64_t plp_first_above(const uint64_t* m, uint64_t n, uint64_t want) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (m[mid] > want) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
SAM_HD uint64_t plp_first_from(const uint64_t* m, uint64_t n, uint64_t want) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (m[mid] >= want) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
// end_max / pos_max: the running maxima of the slots' keys.  In front of lo every record ends at or in front of t0 (or lies on
// an earlier reference), from hi on every record starts at t1 or behind (or lies on a later one).
SAM_HD uint64_t plp_lo(const uint64_t* end_max, uint64_t n, const plp_tile_t& t) { return plp_first_above(end_max, n, ((uint64_t)t.ref << 32) | (uint64_t)t.t0); }
SAM_HD uint64_t plp_hi(const uint64_t* pos_max, uint64_t n, const plp_tile_t& t) { return plp_first_from(pos_max, n, ((uint64_t)t.ref << 32) | (uint64_t)(t.t1 + 1)); }

// ---- the walk ---------------------------------------------------------------------------------------------------------------
SAM_HD uint32_t plp_base_column(uint32_t code) {
    return code == 1 ? BG_PILEUP_A : code == 2 ? BG_PILEUP_C : code == 4 ? BG_PILEUP_G : code == 8 ? BG_PILEUP_T : BG_PILEUP_OTHER;
}
// Lane `lane` of PLP_G: its share of what the kept record rec (one that passed plp_slot) adds to the window [t0, t1) of
// reference `ref`.  add(i) adds one to counter i = column * BG_PILEUP_TILE + (position - t0).  The operations are walked by
// every lane alike; the positions of an operation INSIDE the window are what the lanes stride over, so a pair (record, window)
// costs its operations plus its positions in the window.  Every byte read lies inside the record.
template <class Add>
SAM_HD void plp_walk_lane(const uint8_t* rec, const bg_bam_pileup_t& prm, uint32_t ref, int64_t t0, int64_t t1, uint32_t lane, Add add) {
    if (bai_get32(rec + 4) != ref) return;
    const int64_t pos = (int32_t)bai_get32(rec + 8);
    const uint32_t l_name = rec[12], n_cigar = bai_get16(rec + 16), flag = bai_get16(rec + 18), l_seq = bai_get32(rec + 20);
    const uint8_t* cig = rec + BAM_FIXED + l_name;
    const uint8_t* seq = cig + 4ull * n_cigar;
    const uint8_t* qual = seq + ((uint64_t)l_seq + 1) / 2;
    const uint32_t col0 = (prm.flags & BG_PILEUP_STRANDS) && (flag & 0x10u) ? BG_PILEUP_COLS : 0;
    int64_t r = pos, q = 0;
    for (uint32_t k = 0; k < n_cigar && r <= t1; k++) {  // (an I at r == t1 is anchored at t1 - 1)
        const uint32_t w = bai_get32(cig + 4ull * k), op = w & 15u;
        const int64_t n = w >> 4;
        const int64_t a = r > t0 ? r : t0, b = r + n < t1 ? r + n : t1;  // the operation's reference bases inside the window
        if (op == BAM_CIGAR_M || op == BAM_CIGAR_EQ || op == BAM_CIGAR_X) {
            for (int64_t p = a + lane; p < b; p += PLP_G) {
                uint32_t col = BG_PILEUP_OTHER;
                if (l_seq) {
                    const uint64_t j = (uint64_t)(q + (p - r));
                    if (qual[j] < prm.min_baseq) continue;
                    col = plp_base_column((seq[j >> 1] >> ((j & 1u) ? 0 : 4)) & 15u);
                }
                add((col0 + col) * BG_PILEUP_TILE + (uint32_t)(p - t0));
            }
            r += n;
            q += n;
        } else if (op == BAM_CIGAR_D || op == BAM_CIGAR_N) {
            const uint32_t col = col0 + (op == BAM_CIGAR_D ? BG_PILEUP_DEL : BG_PILEUP_SKIP);
            for (int64_t p = a + lane; p < b; p += PLP_G) add(col * BG_PILEUP_TILE + (uint32_t)(p - t0));
            r += n;
        } else if (op == BAM_CIGAR_I) {
            if (lane == 0 && r > pos && r - 1 >= t0 && r - 1 < t1) add((col0 + BG_PILEUP_INS) * BG_PILEUP_TILE + (uint32_t)(r - 1 - t0));
            q += n;
        } else if (op == BAM_CIGAR_S) {
            q += n;
        }
    }
}

// ---- the rows ---------------------------------------------------------------------------------------------------------------
// Thread `thread` of `n_threads`: its share of the n_pos rows of a tile, W adjacent uint32 each, from the column-major counters.
// wide: dst is 16-byte aligned (a row is 32 or 64 bytes, so every row then is) and each store takes four columns of a position.
SAM_HD void plp_store_rows(const uint32_t* cnt, uint32_t W, uint32_t n_pos, uint32_t* dst, bool wide, uint32_t thread, uint32_t n_threads) {
    if (wide) {
        const uint32_t per = W / 4;  // vectors a row
        for (uint32_t v = thread; v < n_pos * per; v += n_threads) {
            const uint32_t p = v / per, c = 4 * (v % per);
            sam_v16 x;
            for (uint32_t i = 0; i < 4; i++) x.w[i] = cnt[(c + i) * BG_PILEUP_TILE + p];
            *(sam_v16*)(dst + 4ull * v) = x;
        }
    } else {
        for (uint32_t j = thread; j < n_pos * W; j += n_threads) dst[j] = cnt[(j % W) * BG_PILEUP_TILE + j / W];
    }
}

#endif
