// Stand-alone CPU program for tests/test_bam_pileup_host_bodies.py: the __host__ __device__ bodies of csrc/bam_pileup_rule.h run
// on the host, in the steps the kernels of csrc/bam_pileup.hip take.  The front (tests/bam_pileup_host_front.h: the slot pass,
// the running maxima, the order check, the regions by plp_region_ok).  Then every tile: plp_tile, the two searches plp_lo / plp_hi,
// zeroed counters, every kept candidate walked by lanes 0 .. 15 in turn through plp_walk_lane, the rows by plp_store_rows,
// threads 0 .. 255 in turn — once 16 bytes wide and once dword by dword, which must agree.  The first test builds it with
// -fsanitize=address,undefined.  Every record, table, counter tile and row buffer is a heap allocation of exactly its size,
// so a body that reads or writes one byte outside stops the program.
// Input: uint64 cases; per case uint64 n_slots, rec_bytes, n_contigs, n_regions, flags, require, exclude, min_mapq, min_baseq;
// the records; n_slots + 1 offsets; n_contigs x bg_sam_contig_t; n_regions x bg_bam_region_t.
// Output per case: int64 rc, uint64 first_bad, n_rows; if rc == 0 the rows (n_rows x W uint32) and n_regions + 1 row offsets.
#include "bam_pileup_host_front.h"

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
        const HostTables tb(f, n, rec_bytes, n_contigs, n_regions);
        // ---- 1. to 3. the front
        const HostFront fr(tb, prm, false, [&](const bg_bam_region_t& g) { return plp_region_ok(g, tb.contigs, n_contigs); });
        const int64_t rc = fr.rc;
        const uint64_t n_rows = rc ? 0 : fr.row_off[n_regions];
        fwrite(&rc, 8, 1, o);
        fwrite(&fr.first_bad, 8, 1, o);
        fwrite(&n_rows, 8, 1, o);

        // ---- 4. the tiles
        if (!rc) {
            uint32_t* rows = make<uint32_t>(n_rows * W);
            uint32_t* narrow = make<uint32_t>(n_rows * W);
            for (uint64_t tile = 0; tile < fr.tile_off[n_regions]; tile++) {
                const plp_tile_t t = plp_tile(tile, tb.regions, n_regions, fr.tile_off, fr.row_off);
                uint32_t* cnt = fr.count(tb, prm, W, t);
                for (uint32_t th = 0; th < THREADS; th++) {
                    plp_store_rows(cnt, W, (uint32_t)(t.t1 - t.t0), rows + t.row * W, true, th, THREADS);
                    plp_store_rows(cnt, W, (uint32_t)(t.t1 - t.t0), narrow + t.row * W, false, th, THREADS);
                }
                free(cnt);
            }
            if (memcmp(rows, narrow, n_rows * W * 4)) return 3;
            if (n_rows) fwrite(rows, 4, n_rows * W, o);
            fwrite(fr.row_off, 8, n_regions + 1, o);
            free(narrow);
            free(rows);
        }
        free(hd);
    }
    free(n_cases);
    fclose(o);
    fclose(f);
    return 0;
}
