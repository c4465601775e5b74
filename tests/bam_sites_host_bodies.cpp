// Stand-alone CPU program for tests/test_bam_sites_host_bodies.py: the __host__ __device__ bodies of csrc/bam_sites_rule.h (and
// those of csrc/bam_pileup_rule.h they stand on) run on the host, in the steps the kernels of csrc/bam_sites.hip take for
// bg_bam_sites_dev.  The front of tests/bam_pileup_host_front.h, with sit_region_ok for the regions.  The count
// pass, tile by tile: the counters by plp_walk_lane, then threads 0 .. 255 in turn judge positions tid and tid + 256
// (sit_judge) into a share each (sit_share_pos), the shares joined (sit_share_join), the tile's sites from the packed word, the
// share parked as a record (sit_share_summary); a region's tiles summed by strided threads (sit_summary_stride, sit_summary_join)
// and stored as dwords (sit_summary_store).  The tile counts summed in order.  The emit pass: the counters
// again, the per-position counts into the scan array, sit_scan_pair / sit_scan_place around a plain sum of the 256 pairs,
// then sit_site / sit_store — once 16 bytes wide and once dword by dword, which must agree.  The first test builds it with
// -fsanitize=address,undefined.  Every record, table, text, counter tile, scan array and site buffer is a heap allocation of
// exactly its size, so a body that reads or writes one byte outside stops the program.
// Input: uint64 cases; per case uint64 n_slots, rec_bytes, n_contigs, n_regions, text_bytes, n_text (what the call is told),
// bg_bam_sites_t; the records; n_slots + 1 offsets; the contigs; the regions; text_bytes of text.  Then uint64 synthetic tiles;
// per tile bg_bam_sites_t, 16 uint32 counters, the reference byte: positions 0 and T - 1 of a tile get the counters.
// Output per case: int64 rc, uint64 first_bad, n_sites; if rc == 0 the sites, n_regions + 1 offsets, n_regions summaries.  Per
// synthetic tile: uint64 n, the sites.
#include "bam_pileup_host_front.h"

// the tail of the count pass over a counted tile: the tile's share
static sit_share_t count_tail(const uint32_t* cnt, uint32_t n_pos, const uint8_t* ref, const bg_bam_sites_t& prm) {
    sit_share_t all = sit_share_zero();
    for (uint32_t th = 0; th < THREADS; th++) {
        sit_share_t share = sit_share_zero();
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t i = th + h * THREADS;
            if (i < n_pos) sit_share_pos(share, sit_judge(cnt, i, ref[i], prm), prm);
        }
        sit_share_join(all, share);
    }
    return all;
}
// the tail of the emit pass: the tile's records at dst (exactly n of them, which the count pass said), in both store forms
static bool emit_tail(const uint32_t* cnt, uint32_t n_pos, const uint8_t* ref, const bg_bam_sites_t& prm, uint32_t ref_id, int64_t t0, uint32_t region,
                      bg_bam_site_t* wide, bg_bam_site_t* narrow, uint32_t n) {
    uint32_t* scan = make<uint32_t>(BG_PILEUP_TILE);
    std::vector<sit_pos_t> v(BG_PILEUP_TILE);
    for (uint32_t th = 0; th < THREADS; th++)
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t i = th + h * THREADS;
            v[i].n_sites = 0;
            v[i].mask = 0;
            if (i < n_pos) v[i] = sit_judge(cnt, i, ref[i], prm);
            scan[i] = v[i].n_sites;
        }
    uint32_t* pair = make<uint32_t>(THREADS);
    for (uint32_t th = 0; th < THREADS; th++) pair[th] = sit_scan_pair(scan, th);
    uint32_t ex = 0;
    for (uint32_t th = 0; th < THREADS; th++) {
        sit_scan_place(scan, th, ex);
        ex += pair[th];
    }
    bool ok = ex == n;
    for (uint32_t th = 0; th < THREADS && ok; th++)
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t i = th + h * THREADS;
            uint32_t at = scan[i];
            for (uint32_t k = 0; k < 5; k++)
                if (v[i].mask >> k & 1u) {
                    const bg_bam_site_t s = sit_site(cnt, i, v[i], k, ref_id, t0 + i, region);
                    sit_store(s, wide + at, true);
                    sit_store(s, narrow + at, false);
                    at++;
                }
        }
    free(pair);
    free(scan);
    return ok;
}
template <class T>
static T* aligned16(size_t count) {  // exact size, 16-byte aligned for the wide stores
    void* p = nullptr;
    if (posix_memalign(&p, 16, count * sizeof(T) ? count * sizeof(T) : 16)) exit(2);
    memset(p, 0, count * sizeof(T) ? count * sizeof(T) : 16);
    return (T*)p;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint64_t* n_cases = load<uint64_t>(f, 1);
    for (uint64_t c = 0; c < *n_cases; c++) {
        uint64_t* hd = load<uint64_t>(f, 6);
        const uint64_t n = hd[0], rec_bytes = hd[1], n_contigs = hd[2], n_regions = hd[3], text_bytes = hd[4], n_text = hd[5];
        bg_bam_sites_t* sp = load<bg_bam_sites_t>(f, 1);
        const bg_bam_sites_t sprm = *sp;
        const bg_bam_pileup_t prm = sit_pileup_params(sprm);
        const HostTables tb(f, n, rec_bytes, n_contigs, n_regions);
        uint8_t* text = load<uint8_t>(f, text_bytes);
        // ---- the front
        const HostFront fr(tb, prm, sprm.flags || sprm.reserved || sprm.min_alt_permille > 1000,
                           [&](const bg_bam_region_t& g) { return sit_region_ok(g, tb.contigs, n_contigs, n_text); });
        uint64_t n_sites = 0;
        auto count = [&](const plp_tile_t& t) { return fr.count(tb, prm, SIT_W, t); };
        if (!fr.rc && text_bytes != n_text) return 4;  // only a refusal may be told of a text it does not get

        if (!fr.rc) {
            const uint64_t tiles = fr.tile_off[n_regions];
            // ---- the count pass
            uint32_t* tile_sites = make<uint32_t>(tiles);
            uint64_t* tile_site_off = make<uint64_t>(tiles + 1);
            bg_bam_region_summary_t* tile_share = make<bg_bam_region_summary_t>(tiles);
            for (uint64_t tile = 0; tile < tiles; tile++) {
                const plp_tile_t t = plp_tile(tile, tb.regions, n_regions, fr.tile_off, fr.row_off);
                uint32_t* cnt = count(t);
                const sit_share_t share = count_tail(cnt, (uint32_t)(t.t1 - t.t0), text + tb.contigs[t.ref].start + t.t0, sprm);
                tile_sites[tile] = sit_share_sites(share);
                tile_share[tile] = sit_share_summary(share);
                free(cnt);
            }
            for (uint64_t tile = 0; tile < tiles; tile++) tile_site_off[tile + 1] = tile_site_off[tile] + tile_sites[tile];
            n_sites = tile_site_off[tiles];
            // ---- the regions' summaries: threads 0 .. 255 stride over a region's tiles, their sums joined; stored as dwords at
            // an address that is 4-byte aligned and no more
            uint8_t* summary_raw = make<uint8_t>(n_regions * sizeof(bg_bam_region_summary_t) + 4);
            bg_bam_region_summary_t* summary = (bg_bam_region_summary_t*)(summary_raw + 4);
            for (uint64_t r = 0; r < n_regions; r++) {
                bg_bam_region_summary_t a = sit_summary_stride(tile_share, fr.tile_off[r], fr.tile_off[r + 1], 0, THREADS);
                for (uint32_t th = 1; th < THREADS; th++) sit_summary_join(a, sit_summary_stride(tile_share, fr.tile_off[r], fr.tile_off[r + 1], th, THREADS));
                sit_summary_store(a, summary + r);
            }
            // ---- the emit pass
            bg_bam_site_t* sites = aligned16<bg_bam_site_t>(n_sites);
            bg_bam_site_t* narrow = aligned16<bg_bam_site_t>(n_sites);
            uint64_t* site_off = make<uint64_t>(n_regions + 1);
            for (uint64_t r = 0; r <= n_regions; r++) site_off[r] = tiles ? tile_site_off[fr.tile_off[r]] : 0;
            for (uint64_t tile = 0; tile < tiles; tile++) {
                if (tile_site_off[tile + 1] == tile_site_off[tile]) continue;
                const plp_tile_t t = plp_tile(tile, tb.regions, n_regions, fr.tile_off, fr.row_off);
                uint32_t* cnt = count(t);
                if (!emit_tail(cnt, (uint32_t)(t.t1 - t.t0), text + tb.contigs[t.ref].start + t.t0, sprm, t.ref, t.t0, t.region, sites + tile_site_off[tile],
                               narrow + tile_site_off[tile], tile_sites[tile]))
                    return 3;
                free(cnt);
            }
            if (n_sites && memcmp(sites, narrow, n_sites * sizeof(bg_bam_site_t))) return 3;
            fwrite(&fr.rc, 8, 1, o);
            fwrite(&fr.first_bad, 8, 1, o);
            fwrite(&n_sites, 8, 1, o);
            if (n_sites) fwrite(sites, sizeof(bg_bam_site_t), n_sites, o);
            fwrite(site_off, 8, n_regions + 1, o);
            if (n_regions) fwrite(summary_raw + 4, sizeof(bg_bam_region_summary_t), n_regions, o);
            free(site_off);
            free(narrow);
            free(sites);
            free(summary_raw);
            free(tile_share);
            free(tile_site_off);
            free(tile_sites);
        } else {
            fwrite(&fr.rc, 8, 1, o);
            fwrite(&fr.first_bad, 8, 1, o);
            fwrite(&n_sites, 8, 1, o);
        }
        free(text);
        free(sp);
        free(hd);
    }
    free(n_cases);

    // ---- synthetic tiles: counters no record table reaches cheaply
    uint64_t* n_synth = load<uint64_t>(f, 1);
    for (uint64_t c = 0; c < *n_synth; c++) {
        bg_bam_sites_t* sp = load<bg_bam_sites_t>(f, 1);
        uint32_t* row = load<uint32_t>(f, SIT_W);
        uint8_t* byte = load<uint8_t>(f, 1);
        uint32_t* cnt = make<uint32_t>((size_t)SIT_W * BG_PILEUP_TILE);
        uint8_t* ref = (uint8_t*)malloc(BG_PILEUP_TILE);
        memset(ref, 'A', BG_PILEUP_TILE);
        for (uint32_t i : {0u, BG_PILEUP_TILE - 1}) {
            ref[i] = *byte;
            for (uint32_t k = 0; k < SIT_W; k++) cnt[k * BG_PILEUP_TILE + i] = row[k];
        }
        const sit_share_t share = count_tail(cnt, BG_PILEUP_TILE, ref, *sp);
        const uint64_t n = sit_share_sites(share);
        bg_bam_site_t* sites = aligned16<bg_bam_site_t>(n);
        bg_bam_site_t* narrow = aligned16<bg_bam_site_t>(n);
        if (!emit_tail(cnt, BG_PILEUP_TILE, ref, *sp, 0, 0, 0, sites, narrow, (uint32_t)n)) return 3;
        if (n && memcmp(sites, narrow, n * sizeof(bg_bam_site_t))) return 3;
        fwrite(&n, 8, 1, o);
        if (n) fwrite(sites, sizeof(bg_bam_site_t), n, o);
        free(narrow);
        free(sites);
        free(ref);
        free(cnt);
        free(byte);
        free(row);
        free(sp);
    }
    free(n_synth);
    fclose(o);
    fclose(f);
    return 0;
}
