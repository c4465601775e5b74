// Stand-alone CPU program for tests/test_bam_indels_host_bodies.py and tests/test_bam_indels_left_host_bodies.py: the __host__
// __device__ bodies of csrc/bam_indels_rule.h and csrc/bam_indels_left_rule.h (and those of csrc/bam_pileup_rule.h they stand on)
// run on the host, in the steps the kernels of csrc/bam_indels.hip take for bg_bam_indels_dev and bg_bam_indels_left_dev.  A word
// of a case's header says which: the plain flavour runs ind_walk, ind_cmp and ind_seq_lane and sees no text; the left flavour
// runs inl_walk, inl_shift_del / inl_shift_ins, inl_cmp and inl_seq_lane, with the regions' contigs held against the text.
// The front of tests/bam_pileup_host_front.h.  The count pass, tile by tile: threads 0 .. 255 stride over the candidate slots
// and count what the walk emits (left: what lands in the tile behind the shift).  The emit pass over the tiles that have raw
// events: the 8-column counters by plp_walk_lane, the walk (and the shift) again with threads 255 .. 0 in turn, so that the places
// inside a tile's range go out in another order than the count pass saw (nothing behind may depend on it); ind_raw with ind_depth
// (left: of the SHIFTED anchor, and k in the spare word).  The order by std::sort over indices with the flavour's comparison (not
// stable, as the merge sort is not); heads by the same comparison with the predecessor; the sums in order; a run's start at its
// number; the verdict by ind_is_kept; ind_event / ind_store and the flavour's sequence bytes for lanes 0 .. 15.
// The tests build it with -fsanitize=address,undefined.  Every record, table, counter tile, scratch array, event buffer and
// sequence buffer is a heap allocation of exactly its size, and so is the text of every contig, WITHOUT the `$` behind it: a body
// that reads or writes one byte outside, a shift that reads F(-1), the `$` or a byte of another contig stops the program.  The
// records are concatenated once more into a buffer of exactly their size for the comparator, which reads through (recs, off) as
// the kernels do.
// Input: uint64 cases; per case uint64 n_slots, rec_bytes, n_contigs, n_regions, left, n_text, text_bytes (the last two 0 unless
// left), bg_bam_indels_left_t if left and bg_bam_indels_t otherwise; the records; n_slots + 1 offsets; the contigs; the regions;
// text_bytes bytes of text.
// Output per case: int64 rc, uint64 first_bad, n_events, n_seq; if rc == 0 the events, the sequence bytes, n_regions + 1 offsets.
#include <algorithm>

#include "bam_pileup_host_front.h"
#include "../rust-bio_amd/csrc/bam_indels_left_rule.h"

// the steps of one raw event, as the left flavour of ind_tile_kernel takes them
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
        uint64_t* hd = load<uint64_t>(f, 7);
        const uint64_t n = hd[0], rec_bytes = hd[1], n_contigs = hd[2], n_regions = hd[3], n_text = hd[5], text_bytes = hd[6];
        const bool left = hd[4] != 0;
        bg_bam_indels_t iprm;
        uint32_t max_shift = 0;
        if (left) {
            bg_bam_indels_left_t* ip = load<bg_bam_indels_left_t>(f, 1);
            iprm = inl_indels_params(*ip);
            max_shift = ip->max_shift;
            free(ip);
        } else {
            bg_bam_indels_t* ip = load<bg_bam_indels_t>(f, 1);
            iprm = *ip;
            free(ip);
        }
        const bg_bam_pileup_t prm = ind_pileup_params(iprm);
        const HostTables tb(f, n, rec_bytes, n_contigs, n_regions);
        uint8_t* whole_text = load<uint8_t>(f, text_bytes);  // n_text is what the call is told; a refused case may hold fewer
        // every contig that lies inside the text a buffer of its own, of exactly its length: F(-1) and the `$` lie outside it
        std::vector<uint8_t*> text(left ? n_contigs : 0, nullptr);
        for (uint64_t k = 0; k < text.size(); k++) {
            if (tb.contigs[k].start > text_bytes || tb.contigs[k].len > text_bytes - tb.contigs[k].start) continue;
            text[k] = (uint8_t*)malloc(tb.contigs[k].len ? tb.contigs[k].len : 1);
            memcpy(text[k], whole_text + tb.contigs[k].start, tb.contigs[k].len);
        }

        // ---- the front
        const HostFront fr(tb, prm, iprm.flags || iprm.reserved || iprm.min_alt_permille > 1000, [&](const bg_bam_region_t& g) {
            return left ? sit_region_ok(g, tb.contigs, n_contigs, n_text) : plp_region_ok(g, tb.contigs, n_contigs);
        });
        uint64_t n_events = 0, n_seq = 0;

        if (!fr.rc) {
            const uint64_t tiles = fr.tile_off[n_regions];
            uint8_t* recs = make<uint8_t>(rec_bytes);
            memcpy(recs, tb.all, rec_bytes);
            // the raw events of slot s in tile t, by flavour: emit(kind, anchor, len, q, k) with the shifted anchor and its steps
            auto walk = [&](uint64_t s, const plp_tile_t& t, auto emit) {
                if (!left) {
                    ind_walk(tb.rec[s], t.ref, t.t0, t.t1, [&](uint32_t kind, uint32_t anchor, uint32_t len, uint32_t q) { emit(kind, anchor, len, q, 0u); });
                    return;
                }
                inl_walk(tb.rec[s], t.ref, t.t0, t.t1, max_shift, [&](uint32_t kind, uint32_t anchor, uint32_t len, uint32_t q, int64_t pos) {
                    const uint32_t k = shift_of(text[t.ref], tb.contigs[t.ref].len, tb.rec[s], kind, anchor, len, q, pos, max_shift);
                    const int64_t at = (int64_t)anchor - k;
                    if (at >= t.t0 && at < t.t1) emit(kind, (uint32_t)at, len, q, k);
                });
            };
            auto cmp = [&](const ind_raw_t& a, const ind_raw_t& b) { return left ? inl_cmp(a, b, recs, tb.off) : ind_cmp(a, b, recs, tb.off); };
            // ---- the count pass
            uint32_t* tile_raw = make<uint32_t>(tiles);
            uint64_t* tile_raw_off = make<uint64_t>(tiles + 1);
            for (uint64_t tile = 0; tile < tiles; tile++) {
                const plp_tile_t t = plp_tile(tile, tb.regions, n_regions, fr.tile_off, fr.row_off);
                const uint64_t lo = plp_lo(fr.end_max, n, t), hi = plp_hi(fr.pos_max, n, t);
                for (uint32_t th = 0; th < THREADS; th++)
                    for (uint64_t s = lo + th; s < hi; s += THREADS)
                        if (fr.kept[s]) walk(s, t, [&](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) { tile_raw[tile]++; });
            }
            for (uint64_t tile = 0; tile < tiles; tile++) tile_raw_off[tile + 1] = tile_raw_off[tile] + tile_raw[tile];
            const uint64_t n_raw = tile_raw_off[tiles];
            // ---- the emit pass
            ind_raw_t* raw = make<ind_raw_t>(n_raw);
            for (uint64_t tile = 0; tile < tiles; tile++) {
                const uint32_t room = tile_raw[tile];
                if (!room) continue;
                const plp_tile_t t = plp_tile(tile, tb.regions, n_regions, fr.tile_off, fr.row_off);
                uint32_t* cnt = fr.count(tb, prm, BG_PILEUP_COLS, t);
                const uint64_t lo = plp_lo(fr.end_max, n, t), hi = plp_hi(fr.pos_max, n, t);
                uint32_t next = 0;
                for (uint32_t th = THREADS; th-- > 0;)
                    for (uint64_t s = lo + th; s < hi; s += THREADS) {
                        if (!fr.kept[s]) continue;
                        const uint32_t flag = bai_get16(tb.rec[s] + 18);
                        walk(s, t, [&](uint32_t kind, uint32_t anchor, uint32_t len, uint32_t q, uint32_t k) {
                            const uint32_t place = next++;
                            if (place >= room) exit(3);
                            ind_raw_t e = ind_raw((uint32_t)tile, kind, anchor, len, q, flag, ind_depth(cnt, anchor - (uint32_t)t.t0), s);
                            e.reserved = k;
                            raw[tile_raw_off[tile] + place] = e;
                        });
                    }
                if (next != room) return 3;
                free(cnt);
            }
            // ---- the order, the runs
            uint32_t* order = make<uint32_t>(n_raw);
            for (uint64_t i = 0; i < n_raw; i++) order[i] = (uint32_t)i;
            std::sort(order, order + n_raw, [&](uint32_t a, uint32_t b) { return cmp(raw[a], raw[b]) < 0; });
            uint32_t* head = make<uint32_t>(n_raw);
            uint32_t* rev = make<uint32_t>(n_raw);
            uint64_t* head_off = make<uint64_t>(n_raw + 1);
            uint64_t* rev_off = make<uint64_t>(n_raw + 1);
            for (uint64_t i = 0; i < n_raw; i++) {
                head[i] = i == 0 || cmp(raw[order[i - 1]], raw[order[i]]) != 0;
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
                    const uint64_t i = tile_raw_off[fr.tile_off[r]];
                    v = keep_off[i < n_raw ? head_off[i] : head_off[n_raw]];
                }
                event_off[r] = v;
            }
            for (uint64_t k = 0; k < n_raw; k++) {
                if (!keep[k]) continue;
                const uint32_t s = run_start[k], e = run_start[k + 1];
                const uint32_t r = (uint32_t)(rev_off[e] - rev_off[s]);
                const ind_raw_t v = raw[order[s]];
                const plp_tile_t t = plp_tile(v.tile, tb.regions, n_regions, fr.tile_off, fr.row_off);
                ind_store(ind_event(v, t.ref, t.region, e - s - r, r, seq_off[k]), events + keep_off[k]);
                if (ind_kind(v) != BG_SITE_INS) continue;
                for (uint32_t lane = 0; lane < PLP_G; lane++) {
                    if (left) inl_seq_lane(v, recs, tb.off, seq + seq_off[k], lane, PLP_G);
                    else ind_seq_lane(v, recs, tb.off, seq + seq_off[k], lane, PLP_G);
                }
            }
            fwrite(&fr.rc, 8, 1, o);
            fwrite(&fr.first_bad, 8, 1, o);
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
            free(raw);
            free(tile_raw_off);
            free(tile_raw);
            free(recs);
        } else {
            fwrite(&fr.rc, 8, 1, o);
            fwrite(&fr.first_bad, 8, 1, o);
            fwrite(&n_events, 8, 1, o);
            fwrite(&n_seq, 8, 1, o);
        }
        for (uint8_t* t : text) free(t);
        free(whole_text);
        free(hd);
    }
    free(n_cases);
    fclose(o);
    fclose(f);
    return 0;
}
