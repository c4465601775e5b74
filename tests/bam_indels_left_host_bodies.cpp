// Stand-alone CPU program for tests/test_bam_indels_left_host_bodies.py: the __host__ __device__ bodies of
// csrc/bam_indels_left_rule.h (and those of csrc/bam_indels_rule.h and csrc/bam_pileup_rule.h they stand on) run on the host, in
// the steps the kernels of csrc/bam_pileup.hip take for bg_bam_indels_left_dev.  The front as tests/bam_indels_host_bodies.cpp
// runs it, with the regions' contigs held against the text.  The count pass, tile by tile: threads 0 .. 255 stride over the
// candidate slots, inl_walk, the shift, and count what lands in the tile.  The emit pass over the tiles that have raw events: the
// 8-column counters by plp_walk_lane, the walk and the shift again with threads 255 .. 0 in turn, so that the places inside a
// tile's range go out in another order than the count pass saw (nothing behind may depend on it); ind_raw with ind_depth of the
// SHIFTED anchor and k in the spare word.  The order by std::sort over indices with inl_cmp (not stable, as the merge sort is
// not); heads by inl_cmp with the predecessor; the sums in order; a run's start at its number; the verdict by ind_is_kept;
// ind_event / ind_store and inl_seq_lane for lanes 0 .. 15.
// The test builds it with -fsanitize=address,undefined.  Every record, table, counter tile, scratch array, event buffer and
// sequence buffer is a heap allocation of exactly its size, and so is the text of every contig, WITHOUT the `$` behind it: a
// shift that reads F(-1), the `$` or a byte of another contig stops the program.
// Input: uint64 cases; per case uint64 n_slots, rec_bytes, n_contigs, n_regions, n_text, text_bytes, bg_bam_indels_left_t; the
// records; n_slots + 1 offsets; the contigs; the regions; text_bytes bytes of text.
// Output per case: int64 rc, uint64 first_bad, n_events, n_seq; if rc == 0 the events, the sequence bytes, n_regions + 1 offsets.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rust-bio_amd/csrc/bam_indels_left_rule.h"

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

// the steps of one raw event, as inl_tile_kernel takes them
static uint32_t shift_of(const uint8_t* text, uint64_t clen, const uint8_t* rec, uint32_t kind, uint32_t anchor, uint32_t len, uint32_t q, int64_t pos,
                         uint32_t max_shift) {
    return kind == BG_SITE_DEL ? inl_shift_del(text, (int64_t)clen, pos, anchor, len, max_shift) : inl_shift_ins(text, pos, anchor, len, ind_seq_of(rec), q, max_shift);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint64_t* n_cases = load<uint64_t>(f, 1);
    for (uint64_t c = 0; c < *n_cases; c++) {
        uint64_t* hd = load<uint64_t>(f, 6);
        const uint64_t n = hd[0], rec_bytes = hd[1], n_contigs = hd[2], n_regions = hd[3], n_text = hd[4], text_bytes = hd[5];
        bg_bam_indels_left_t* ip = load<bg_bam_indels_left_t>(f, 1);
        const bg_bam_indels_t iprm = inl_indels_params(*ip);
        const uint32_t max_shift = ip->max_shift;
        const bg_bam_pileup_t prm = ind_pileup_params(iprm);
        uint8_t* all = load<uint8_t>(f, rec_bytes);
        uint64_t* off = load<uint64_t>(f, n + 1);
        bg_sam_contig_t* contigs = load<bg_sam_contig_t>(f, n_contigs);
        bg_bam_region_t* regions = load<bg_bam_region_t>(f, n_regions);
        uint8_t* whole_text = load<uint8_t>(f, text_bytes);  // n_text is what the call is told; a refused case may hold fewer
        // every contig that lies inside the text a buffer of its own, of exactly its length: F(-1) and the `$` lie outside it
        std::vector<uint8_t*> text(n_contigs, nullptr);
        for (uint64_t k = 0; k < n_contigs; k++) {
            if (contigs[k].start > text_bytes || contigs[k].len > text_bytes - contigs[k].start) continue;
            text[k] = (uint8_t*)malloc(contigs[k].len ? contigs[k].len : 1);
            memcpy(text[k], whole_text + contigs[k].start, contigs[k].len);
        }
        std::vector<uint8_t*> rec(n);  // every slot a buffer of its own
        for (uint64_t i = 0; i < n; i++) {
            rec[i] = (uint8_t*)malloc(off[i + 1] - off[i] ? off[i + 1] - off[i] : 1);
            memcpy(rec[i], all + off[i], off[i + 1] - off[i]);
        }

        // ---- the front
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
        bool region_bad = false;
        uint64_t* row_off = make<uint64_t>(n_regions + 1);
        uint64_t* tile_off = make<uint64_t>(n_regions + 1);
        for (uint64_t r = 0; r < n_regions; r++) {
            uint32_t len = 0;
            if (sit_region_ok(regions[r], contigs, n_contigs, n_text)) len = (uint32_t)(regions[r].end - regions[r].beg);
            else region_bad = true;
            row_off[r + 1] = row_off[r] + len;
            tile_off[r + 1] = tile_off[r] + plp_tiles(len);
        }
        int64_t rc = BG_OK;
        uint64_t first_bad = UINT64_MAX, n_events = 0, n_seq = 0;
        if (iprm.flags || iprm.reserved || iprm.min_alt_permille > 1000 || region_bad) rc = BG_ERR_INVALID_ARG;
        else if (bad != BAI_NONE) {
            first_bad = bad >> 2;
            rc = (bad & 3) == BAI_UNSUPPORTED ? BG_ERR_UNSUPPORTED : BG_ERR_INVALID_ARG;
        }

        if (!rc) {
            const uint64_t tiles = tile_off[n_regions];
            // ---- the count pass
            uint32_t* tile_raw = make<uint32_t>(tiles);
            uint64_t* tile_raw_off = make<uint64_t>(tiles + 1);
            for (uint64_t tile = 0; tile < tiles; tile++) {
                const plp_tile_t t = plp_tile(tile, regions, n_regions, tile_off, row_off);
                const uint64_t lo = plp_lo(end_max, n, t), hi = plp_hi(pos_max, n, t);
                for (uint32_t th = 0; th < THREADS; th++)
                    for (uint64_t s = lo + th; s < hi; s += THREADS)
                        if (kept[s])
                            inl_walk(rec[s], t.ref, t.t0, t.t1, max_shift, [&](uint32_t kind, uint32_t anchor, uint32_t len, uint32_t q, int64_t pos) {
                                const int64_t at = (int64_t)anchor - shift_of(text[t.ref], contigs[t.ref].len, rec[s], kind, anchor, len, q, pos, max_shift);
                                if (at >= t.t0 && at < t.t1) tile_raw[tile]++;
                            });
            }
            for (uint64_t tile = 0; tile < tiles; tile++) tile_raw_off[tile + 1] = tile_raw_off[tile] + tile_raw[tile];
            const uint64_t n_raw = tile_raw_off[tiles];
            // ---- the emit pass
            ind_raw_t* raw = make<ind_raw_t>(n_raw);
            for (uint64_t tile = 0; tile < tiles; tile++) {
                const uint32_t room = tile_raw[tile];
                if (!room) continue;
                const plp_tile_t t = plp_tile(tile, regions, n_regions, tile_off, row_off);
                uint32_t* cnt = make<uint32_t>((size_t)BG_PILEUP_COLS * BG_PILEUP_TILE);
                const uint64_t lo = plp_lo(end_max, n, t), hi = plp_hi(pos_max, n, t);
                for (uint64_t s = lo; s < hi; s++) {
                    if (!kept[s]) continue;
                    for (uint32_t lane = 0; lane < PLP_G; lane++) plp_walk_lane(rec[s], prm, t.ref, t.t0, t.t1, lane, [&](uint32_t i) { cnt[i]++; });
                }
                uint32_t next = 0;
                for (uint32_t th = THREADS; th-- > 0;)
                    for (uint64_t s = lo + th; s < hi; s += THREADS) {
                        if (!kept[s]) continue;
                        const uint32_t flag = bai_get16(rec[s] + 18);
                        inl_walk(rec[s], t.ref, t.t0, t.t1, max_shift, [&](uint32_t kind, uint32_t anchor, uint32_t len, uint32_t q, int64_t pos) {
                            const uint32_t k = shift_of(text[t.ref], contigs[t.ref].len, rec[s], kind, anchor, len, q, pos, max_shift);
                            const int64_t at = (int64_t)anchor - k;
                            if (at < t.t0 || at >= t.t1) return;
                            const uint32_t place = next++;
                            if (place >= room) exit(3);
                            ind_raw_t e = ind_raw((uint32_t)tile, kind, (uint32_t)at, len, q, flag, ind_depth(cnt, (uint32_t)(at - t.t0)), s);
                            e.reserved = k;
                            raw[tile_raw_off[tile] + place] = e;
                        });
                    }
                if (next != room) return 3;
                free(cnt);
            }
            // ---- the order, the runs
            uint8_t* recs = make<uint8_t>(rec_bytes);
            memcpy(recs, all, rec_bytes);
            uint32_t* order = make<uint32_t>(n_raw);
            for (uint64_t i = 0; i < n_raw; i++) order[i] = (uint32_t)i;
            std::sort(order, order + n_raw, [&](uint32_t a, uint32_t b) { return inl_cmp(raw[a], raw[b], recs, off) < 0; });
            uint32_t* head = make<uint32_t>(n_raw);
            uint32_t* rev = make<uint32_t>(n_raw);
            uint64_t* head_off = make<uint64_t>(n_raw + 1);
            uint64_t* rev_off = make<uint64_t>(n_raw + 1);
            for (uint64_t i = 0; i < n_raw; i++) {
                head[i] = i == 0 || inl_cmp(raw[order[i - 1]], raw[order[i]], recs, off) != 0;
                rev[i] = ind_rev(raw[order[i]]);
            }
            for (uint64_t i = 0; i < n_raw; i++) {
                head_off[i + 1] = head_off[i] + head[i];
                rev_off[i + 1] = rev_off[i] + rev[i];
            }
            uint32_t* run_start = make<uint32_t>(n_raw + 1);
            for (uint64_t i = 0; i <= n_raw; i++) {
                if (i == n_raw) run_start[head_off[n_raw]] = (uint32_t)n_raw;
                else if (head[i]) run_start[head_off[i]] = (uint32_t)i;
            }
            // ---- the events
            uint32_t* keep = make<uint32_t>(n_raw);
            uint32_t* seq_len = make<uint32_t>(n_raw);
            uint64_t* keep_off = make<uint64_t>(n_raw + 1);
            uint64_t* seq_off = make<uint64_t>(n_raw + 1);
            for (uint64_t k = 0; k < n_raw; k++) {
                if (k >= head_off[n_raw]) continue;
                const uint32_t s = run_start[k], e = run_start[k + 1];
                const uint32_t r = (uint32_t)(rev_off[e] - rev_off[s]);
                const ind_raw_t v = raw[order[s]];
                keep[k] = ind_is_kept(e - s - r, r, v.depth, iprm);
                seq_len[k] = keep[k] && ind_kind(v) == BG_SITE_INS ? v.len : 0;
            }
            for (uint64_t k = 0; k < n_raw; k++) {
                keep_off[k + 1] = keep_off[k] + keep[k];
                seq_off[k + 1] = seq_off[k] + seq_len[k];
            }
            n_events = keep_off[n_raw];
            n_seq = seq_off[n_raw];
            bg_bam_indel_t* events = make<bg_bam_indel_t>(n_events);
            uint8_t* seq = make<uint8_t>(n_seq);
            uint64_t* event_off = make<uint64_t>(n_regions + 1);
            for (uint64_t r = 0; r <= n_regions; r++) {
                uint64_t v = 0;
                if (tiles && n_raw) {
                    const uint64_t i = tile_raw_off[tile_off[r]];
                    v = keep_off[i < n_raw ? head_off[i] : head_off[n_raw]];
                }
                event_off[r] = v;
            }
            for (uint64_t k = 0; k < n_raw; k++) {
                if (!keep[k]) continue;
                const uint32_t s = run_start[k], e = run_start[k + 1];
                const uint32_t r = (uint32_t)(rev_off[e] - rev_off[s]);
                const ind_raw_t v = raw[order[s]];
                const plp_tile_t t = plp_tile(v.tile, regions, n_regions, tile_off, row_off);
                ind_store(ind_event(v, t.ref, t.region, e - s - r, r, seq_off[k]), events + keep_off[k]);
                if (ind_kind(v) == BG_SITE_INS)
                    for (uint32_t lane = 0; lane < PLP_G; lane++) inl_seq_lane(v, recs, off, seq + seq_off[k], lane, PLP_G);
            }
            fwrite(&rc, 8, 1, o);
            fwrite(&first_bad, 8, 1, o);
            fwrite(&n_events, 8, 1, o);
            fwrite(&n_seq, 8, 1, o);
            if (n_events) fwrite(events, sizeof(bg_bam_indel_t), n_events, o);
            if (n_seq) fwrite(seq, 1, n_seq, o);
            fwrite(event_off, 8, n_regions + 1, o);
            free(event_off);
            free(seq);
            free(events);
            free(seq_off);
            free(keep_off);
            free(seq_len);
            free(keep);
            free(run_start);
            free(rev_off);
            free(head_off);
            free(rev);
            free(head);
            free(order);
            free(recs);
            free(raw);
            free(tile_raw_off);
            free(tile_raw);
        } else {
            fwrite(&rc, 8, 1, o);
            fwrite(&first_bad, 8, 1, o);
            fwrite(&n_events, 8, 1, o);
            fwrite(&n_seq, 8, 1, o);
        }
        free(tile_off);
        free(row_off);
        free(kept);
        free(end_max);
        free(pos_max);
        free(end_key);
        free(pos_key);
        for (uint64_t i = 0; i < n; i++) free(rec[i]);
        for (uint64_t k = 0; k < n_contigs; k++) free(text[k]);
        free(whole_text);
        free(regions);
        free(contigs);
        free(off);
        free(all);
        free(ip);
        free(hd);
    }
    free(n_cases);
    fclose(o);
    fclose(f);
    return 0;
}
