// Stand-alone CPU program for tests/test_bam_pileup_host_bodies.py: the __host__ __device__ bodies of csrc/bam_pileup_rule.h run
// on the host, in the steps the kernels of csrc/bam_pileup.hip take.  The slot pass: plp_slot per non-empty slot, the first
// error by minimum over slot << 2 | kind; the running maxima of both keys; the order check against the running maximum.  The
// regions: plp_region_ok, lengths and tile counts, their sums.  Then every tile: plp_tile, the two searches plp_lo / plp_hi,
// zeroed counters, every kept candidate walked by lanes 0 .. 15 in turn through plp_walk_lane, the rows by plp_store_rows,
// threads 0 .. 255 in turn — once 16 bytes wide and once dword by dword, which must agree.  The first test builds it with
// -fsanitize=address,undefined.  Every record, table, counter tile and row buffer is a heap allocation of exactly its size,
// so a body that reads or writes one byte outside stops the program.
// Input: uint64 cases; per case uint64 n_slots, rec_bytes, n_contigs, n_regions, flags, require, exclude, min_mapq, min_baseq;
// the records; n_slots + 1 offsets; n_contigs x bg_sam_contig_t; n_regions x bg_bam_region_t.
// Output per case: int64 rc, uint64 first_bad, n_rows; if rc == 0 the rows (n_rows x W uint32) and n_regions + 1 row offsets.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rust-bio_amd/csrc/bam_pileup_rule.h"

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

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint64_t* n_cases = load<uint64_t>(f, 1);
    for (uint64_t c = 0; c < *n_cases; c++) {
        uint64_t* hd = load<uint64_t>(f, 9);
        const uint64_t n = hd[0], rec_bytes = hd[1], n_contigs = hd[2], n_regions = hd[3];
        const bg_bam_pileup_t prm = {(uint32_t)hd[4], (uint16_t)hd[5], (uint16_t)hd[6], (uint8_t)hd[7], (uint8_t)hd[8], 0};
        const uint32_t W = prm.flags & BG_PILEUP_STRANDS ? 2 * BG_PILEUP_COLS : BG_PILEUP_COLS;
        uint8_t* all = load<uint8_t>(f, rec_bytes);
        uint64_t* off = load<uint64_t>(f, n + 1);
        bg_sam_contig_t* contigs = load<bg_sam_contig_t>(f, n_contigs);
        bg_bam_region_t* regions = load<bg_bam_region_t>(f, n_regions);
        std::vector<uint8_t*> rec(n);  // every slot a buffer of its own
        for (uint64_t i = 0; i < n; i++) {
            rec[i] = (uint8_t*)malloc(off[i + 1] - off[i] ? off[i + 1] - off[i] : 1);
            memcpy(rec[i], all + off[i], off[i + 1] - off[i]);
        }

        // ---- 1., 2. the slots
        uint64_t bad = BAI_NONE;
        uint64_t* pos_key = make<uint64_t>(n);
        uint64_t* end_key = make<uint64_t>(n);
        uint64_t* pos_max = make<uint64_t>(n);
        uint64_t* end_max = make<uint64_t>(n);
        uint8_t* kept = make<uint8_t>(n);
        for (uint64_t i = 0; i < n; i++) {
            plp_slot_t s = {0, 0, 0};
            if (off[i + 1] > off[i]) {
                const int kind = plp_slot(rec[i], off[i + 1] - off[i], contigs, n_contigs, prm, &s);
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
            if (off[i + 1] > off[i] && pos_max[i] != pos_key[i] && ((i << 2) | BAI_INVALID) < bad) bad = (i << 2) | BAI_INVALID;

        // ---- 3. the regions
        bool region_bad = false;
        uint64_t* row_off = make<uint64_t>(n_regions + 1);
        uint64_t* tile_off = make<uint64_t>(n_regions + 1);
        for (uint64_t r = 0; r < n_regions; r++) {
            uint32_t len = 0;
            if (plp_region_ok(regions[r], contigs, n_contigs)) len = (uint32_t)(regions[r].end - regions[r].beg);
            else region_bad = true;
            row_off[r + 1] = row_off[r] + len;
            tile_off[r + 1] = tile_off[r] + plp_tiles(len);
        }
        int64_t rc = BG_OK;
        uint64_t first_bad = UINT64_MAX, n_rows = 0;
        if (region_bad) rc = BG_ERR_INVALID_ARG;
        else if (bad != BAI_NONE) {
            first_bad = bad >> 2;
            rc = (bad & 3) == BAI_UNSUPPORTED ? BG_ERR_UNSUPPORTED : BG_ERR_INVALID_ARG;
        } else n_rows = row_off[n_regions];
        fwrite(&rc, 8, 1, o);
        fwrite(&first_bad, 8, 1, o);
        fwrite(&n_rows, 8, 1, o);

        // ---- 4. the tiles
        if (!rc) {
            uint32_t* rows = make<uint32_t>(n_rows * W);
            uint32_t* narrow = make<uint32_t>(n_rows * W);
            for (uint64_t tile = 0; tile < tile_off[n_regions]; tile++) {
                const plp_tile_t t = plp_tile(tile, regions, n_regions, tile_off, row_off);
                const uint64_t lo = plp_lo(end_max, n, t), hi = plp_hi(pos_max, n, t);
                uint32_t* cnt = make<uint32_t>((size_t)W * BG_PILEUP_TILE);
                for (uint64_t s = lo; s < hi; s++) {
                    if (!kept[s]) continue;
                    for (uint32_t lane = 0; lane < PLP_G; lane++) plp_walk_lane(rec[s], prm, t.ref, t.t0, t.t1, lane, [&](uint32_t i) { cnt[i]++; });
                }
                for (uint32_t th = 0; th < THREADS; th++) {
                    plp_store_rows(cnt, W, (uint32_t)(t.t1 - t.t0), rows + t.row * W, true, th, THREADS);
                    plp_store_rows(cnt, W, (uint32_t)(t.t1 - t.t0), narrow + t.row * W, false, th, THREADS);
                }
                free(cnt);
            }
            if (memcmp(rows, narrow, n_rows * W * 4)) return 3;
            if (n_rows) fwrite(rows, 4, n_rows * W, o);
            fwrite(row_off, 8, n_regions + 1, o);
            free(narrow);
            free(rows);
        }
        free(tile_off);
        free(row_off);
        free(kept);
        free(end_max);
        free(pos_max);
        free(end_key);
        free(pos_key);
        for (uint64_t i = 0; i < n; i++) free(rec[i]);
        free(regions);
        free(contigs);
        free(off);
        free(all);
        free(hd);
    }
    free(n_cases);
    fclose(o);
    fclose(f);
    return 0;
}
