// What the stand-alone CPU programs of the pileup family share (tests/bam_pileup_host_bodies.cpp, tests/bam_sites_host_bodies.cpp,
// tests/bam_indels_host_bodies.cpp): exact-size heap buffers, a case's tables with every slot a buffer of its own, and the front
// — steps 1 to 3 of csrc/bam_pileup.hip's plp_front, by the bodies of csrc/bam_pileup_rule.h.  The slot pass: plp_slot per
// non-empty slot, the first error by minimum over slot << 2 | kind; the running maxima of both keys; the order check against the
// running maximum.  The regions: the caller's rule (plp_region_ok, or sit_region_ok with n_text), lengths and tile counts, their
// sums.  Then the verdict as the call gives it: a refusal of the parameters or of a region names no slot and comes first.
// Every buffer is a heap allocation of exactly its size, so a body that reads or writes one byte outside stops a program built
// with -fsanitize=address.
#ifndef BAM_PILEUP_HOST_FRONT_H
#define BAM_PILEUP_HOST_FRONT_H
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rust-bio_amd/csrc/bam_sites_rule.h"

template <typename T>
static T* make(size_t count) {
    return (T*)calloc(count ? count : 1, sizeof(T));
}
template <typename T>
static T* load(FILE* f, size_t count) {
    T* p = (T*)malloc(count * sizeof(T) ? count * sizeof(T) : 1);
    if (count && fread(p, sizeof(T), count, f) != count) exit(2);
    return p;
}
static const uint32_t THREADS = 256;

// the records, n + 1 offsets, the contigs and the regions, as they follow one another in a case's input
struct HostTables {
    uint64_t n, rec_bytes, n_contigs, n_regions;
    uint8_t* all;
    uint64_t* off;
    bg_sam_contig_t* contigs;
    bg_bam_region_t* regions;
    std::vector<uint8_t*> rec;  // every slot a buffer of its own

    HostTables(FILE* f, uint64_t n_, uint64_t rec_bytes_, uint64_t n_contigs_, uint64_t n_regions_)
        : n(n_), rec_bytes(rec_bytes_), n_contigs(n_contigs_), n_regions(n_regions_), rec(n_) {
        all = load<uint8_t>(f, rec_bytes);
        off = load<uint64_t>(f, n + 1);
        contigs = load<bg_sam_contig_t>(f, n_contigs);
        regions = load<bg_bam_region_t>(f, n_regions);
        for (uint64_t i = 0; i < n; i++) {
            rec[i] = (uint8_t*)malloc(off[i + 1] - off[i] ? off[i + 1] - off[i] : 1);
            memcpy(rec[i], all + off[i], off[i + 1] - off[i]);
        }
    }
    ~HostTables() {
        for (uint64_t i = 0; i < n; i++) free(rec[i]);
        free(regions);
        free(contigs);
        free(off);
        free(all);
    }
};

struct HostFront {
    uint64_t *pos_key, *end_key, *pos_max, *end_max;  // [n]
    uint8_t* kept;                                    // [n]
    uint64_t *row_off, *tile_off;                     // [n_regions + 1]
    int64_t rc;
    uint64_t first_bad;

    // refused: the call refuses its parameters; region_ok(region): the call's rule for a region
    template <class RegionOk>
    HostFront(const HostTables& c, const bg_bam_pileup_t& prm, bool refused, RegionOk region_ok) {
        const uint64_t n = c.n;
        // ---- 1., 2. the slots
        uint64_t bad = BAI_NONE;
        pos_key = make<uint64_t>(n);
        end_key = make<uint64_t>(n);
        pos_max = make<uint64_t>(n);
        end_max = make<uint64_t>(n);
        kept = make<uint8_t>(n);
        for (uint64_t i = 0; i < n; i++) {
            plp_slot_t s = {0, 0, 0};
            if (c.off[i + 1] > c.off[i]) {
                const int kind = plp_slot(c.rec[i], c.off[i + 1] - c.off[i], c.contigs, c.n_contigs, prm, &s);
                if (kind && ((i << 2) | (uint64_t)kind) < bad) bad = (i << 2) | (uint64_t)kind;
            }
            pos_key[i] = s.pos_key;
            end_key[i] = s.end_key;
            kept[i] = s.kept;
        }
        for (uint64_t i = 0; i < n; i++) {
            pos_max[i] = i && pos_max[i - 1] > pos_key[i] ? pos_max[i - 1] : pos_key[i];
            end_max[i] = i && end_max[i - 1] > end_key[i] ? end_max[i - 1] : end_key[i];
        }
        for (uint64_t i = 0; i < n; i++)
            if (c.off[i + 1] > c.off[i] && pos_max[i] != pos_key[i] && ((i << 2) | BAI_INVALID) < bad) bad = (i << 2) | BAI_INVALID;
        // ---- 3. the regions
        bool region_bad = false;
        row_off = make<uint64_t>(c.n_regions + 1);
        tile_off = make<uint64_t>(c.n_regions + 1);
        for (uint64_t r = 0; r < c.n_regions; r++) {
            uint32_t len = 0;
            if (region_ok(c.regions[r])) len = (uint32_t)(c.regions[r].end - c.regions[r].beg);
            else region_bad = true;
            row_off[r + 1] = row_off[r] + len;
            tile_off[r + 1] = tile_off[r] + plp_tiles(len);
        }
        rc = BG_OK;
        first_bad = UINT64_MAX;
        if (refused || region_bad) rc = BG_ERR_INVALID_ARG;
        else if (bad != BAI_NONE) {
            first_bad = bad >> 2;
            rc = (bad & 3) == BAI_UNSUPPORTED ? BG_ERR_UNSUPPORTED : BG_ERR_INVALID_ARG;
        }
    }
    ~HostFront() {
        free(tile_off);
        free(row_off);
        free(kept);
        free(end_max);
        free(pos_max);
        free(end_key);
        free(pos_key);
    }
    // a counted tile: W columns, every kept candidate walked by lanes 0 .. PLP_G - 1 in turn; the caller frees it
    uint32_t* count(const HostTables& c, const bg_bam_pileup_t& prm, uint32_t W, const plp_tile_t& t) const {
        uint32_t* cnt = make<uint32_t>((size_t)W * BG_PILEUP_TILE);
        const uint64_t lo = plp_lo(end_max, c.n, t), hi = plp_hi(pos_max, c.n, t);
        for (uint64_t s = lo; s < hi; s++) {
            if (!kept[s]) continue;
            for (uint32_t lane = 0; lane < PLP_G; lane++) plp_walk_lane(c.rec[s], prm, t.ref, t.t0, t.t1, lane, [&](uint32_t i) { cnt[i]++; });
        }
        return cnt;
    }
};

#endif
