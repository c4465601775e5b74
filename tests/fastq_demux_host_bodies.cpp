// Stand-alone CPU program for tests/test_fastq_demux_host_bodies.py: the per-record bodies of csrc/fastq_demux.hip
// (csrc/fastq_demux_rule.h, __host__ __device__) run on the host, lane by lane, on a batch read from a file; the test builds it
// with -fsanitize=address,undefined and compares what it writes with the restatement (tests/fastq_demux_oracle.py).  What a
// kernel gets from a shuffle or a ballot is computed here from the other lanes' values; the order of the steps is the kernels'.
// Input: 11 uint32 (n, n_pat, n_bins, G, flags, min_margin, max_offset, prefix bytes of seq / qual, bytes of seq / qual behind
// their prefixes), pat_bin[n_pat], the n * n_pat hit records, split_bin[n] (the bins the split is given), n records, the two
// buffers with their prefixes, n + 1 sequence and quality offsets.  Every buffer is allocated at exactly its size, so that a
// byte read or written outside it stops the program.
// Output: assign's bin[n], hit_out[n], pat_out[n]; the split of the columns by split_bin with assign's hit_out as `hit`:
// recs[n], seq_off[n + 1], qual_off[n + 1], seq, qual, hit_out[n], perm[n], bin_off[n_bins + 3].
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rust-bio_amd/csrc/fastq_demux_rule.h"

template <typename T>
static T* exact(size_t count) {
    return (T*)malloc(count * sizeof(T));
}
template <typename T>
static T* load(FILE* f, size_t count) {
    T* p = exact<T>(count);
    if (fread(p, sizeof(T), count, f) != count) exit(2);
    return p;
}
static uint8_t* source(FILE* f, uint32_t prefix, uint32_t bytes) {
    uint8_t* p = load<uint8_t>(f, (size_t)prefix + bytes);
    ASAN_POISON_MEMORY_REGION(p, prefix & ~7u);
    return p;
}
static bool same(const dmx_state& a, const dmx_state& b) {
    return a.s1 == b.s1 && a.p1 == b.p1 && a.bin1 == b.bin1 && a.has2 == b.has2 && (!a.has2 || a.s2 == b.s2);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    uint32_t h[11];
    if (!f || fread(h, 4, 11, f) != 11) return 2;
    const uint32_t n = h[0], n_pat = h[1], n_bins = h[2], G = h[3], flags = h[4], min_margin = h[5], max_offset = h[6];
    uint32_t* pat_bin = load<uint32_t>(f, n_pat);
    bg_alignment_t* hits = load<bg_alignment_t>(f, (size_t)n * n_pat);
    uint32_t* split_bin = load<uint32_t>(f, n);
    bg_fastq_record_t* recs = load<bg_fastq_record_t>(f, n);
    const uint8_t* seq = source(f, h[7], h[9]);
    const uint8_t* qual = source(f, h[8], h[10]);
    uint64_t* seq_off = load<uint64_t>(f, n + 1);
    uint64_t* qual_off = load<uint64_t>(f, n + 1);
    fclose(f);

    // ---- assign: the lanes' shares, the butterfly of the group, the pair rule, the verdict, the 16 words of hit_out
    dmx_bins* bins = exact<dmx_bins>(1);
    for (uint32_t p = 0; p < BG_MYERS_MAX_PATTERNS; p++)
        bins->b[p] = p < n_pat && pat_bin[p] != BG_DMX_IGNORE ? (uint16_t)pat_bin[p] : (uint16_t)DMX_BIN_IGNORE;
    std::vector<dmx_state> own(n);
    for (uint32_t r = 0; r < n; r++) {
        std::vector<dmx_state> s(G, dmx_empty()), t(G);
        if (dmx_mate_counts(flags, r & 1))
            for (uint32_t lane = 0; lane < G; lane++) s[lane] = dmx_lane_share(hits + (size_t)r * n_pat, n_pat, bins->b, flags, max_offset, lane, G);
        for (uint32_t o = G / 2; o; o >>= 1) {
            for (uint32_t lane = 0; lane < G; lane++) t[lane] = dmx_merge(s[lane], s[lane ^ o]);
            s = t;
        }
        for (uint32_t lane = 1; lane < G; lane++)
            if (!same(s[lane], s[0])) return 3;  // every lane of the group holds the read's state
        own[r] = s[0];
    }
    uint32_t* bin = exact<uint32_t>(n);
    uint32_t* pat_out = exact<uint32_t>(n);
    bg_alignment_t* hit_out = exact<bg_alignment_t>(n);
    for (uint32_t r = 0; r < n; r++) {
        dmx_state s = own[r];
        bool holds = !dmx_is_empty(s);
        if (flags & BG_DMX_PAIRED) s = dmx_pair(own[r], own[r ^ 1], r & 1, &holds);
        bin[r] = dmx_verdict(s, n_bins, min_margin);
        const bool carries = bin[r] < n_bins && holds;
        const bg_alignment_t* mine = hits + (size_t)r * n_pat;
        for (uint32_t lane = 0; lane < G; lane++) dmx_write_hit(hit_out + r, mine, carries ? mine + s.p1 : nullptr, lane, G);
        pat_out[r] = carries ? s.p1 : BG_DMX_IGNORE;
    }

    // ---- split: histogram per (group, tile), its scan, the in-tile stable rank, the two offset scans, the copy
    const uint32_t ng = n_bins + 2, n_tiles = (n + DMX_TILE - 1) / DMX_TILE, n_bits = dmx_group_bits(n_bins);
    std::vector<uint64_t> base((size_t)ng * n_tiles + 1, 0);
    for (uint32_t r = 0; r < n; r++) base[(size_t)dmx_group(split_bin[r], n_bins) * n_tiles + r / DMX_TILE + 1]++;
    for (size_t i = 1; i < base.size(); i++) base[i] += base[i - 1];
    uint64_t* perm = exact<uint64_t>(n);
    uint32_t* sl = exact<uint32_t>(n);
    uint32_t* ql = exact<uint32_t>(n);
    for (uint32_t tile = 0; tile < n_tiles; tile++) {
        std::vector<uint32_t> s_w((size_t)DMX_WAVES * ng, 0);
        for (uint32_t w = 0; w < DMX_WAVES; w++)
            for (uint32_t i = 0; i < DMX_STEPS; i++)
                for (uint32_t lane = 0; lane < 64; lane++) {
                    const uint64_t r = dmx_item(tile, w, i, lane);
                    if (r < n) s_w[w * ng + dmx_group(split_bin[r], n_bins)]++;
                }
        for (uint32_t g = 0; g < ng; g++) {
            uint32_t run = 0;
            for (uint32_t w = 0; w < DMX_WAVES; w++) {
                const uint32_t c = s_w[w * ng + g];
                s_w[w * ng + g] = run;
                run += c;
            }
        }
        for (uint32_t w = 0; w < DMX_WAVES; w++)
            for (uint32_t i = 0; i < DMX_STEPS; i++) {
                uint64_t live = 0, ballot[16] = {};
                uint32_t g[64] = {};
                for (uint32_t lane = 0; lane < 64; lane++) {
                    const uint64_t r = dmx_item(tile, w, i, lane);
                    if (r >= n) continue;
                    live |= (uint64_t)1 << lane;
                    g[lane] = dmx_group(split_bin[r], n_bins);
                    for (uint32_t b = 0; b < n_bits; b++) ballot[b] |= (uint64_t)((g[lane] >> b) & 1) << lane;
                }
                uint32_t before[64], below[64], count[64];
                for (uint32_t lane = 0; lane < 64; lane++) {  // every lane reads before any lane writes
                    if (!(live >> lane & 1)) continue;
                    uint64_t peers = live;
                    for (uint32_t b = 0; b < n_bits; b++) peers = dmx_narrow(peers, ballot[b], (g[lane] >> b) & 1);
                    below[lane] = dmx_rank_below(peers, lane);
                    count[lane] = dmx_peer_count(peers);
                    before[lane] = s_w[w * ng + g[lane]];
                }
                for (uint32_t lane = 0; lane < 64; lane++) {
                    if (!(live >> lane & 1)) continue;
                    const uint64_t r = dmx_item(tile, w, i, lane);
                    if (below[lane] == 0) s_w[w * ng + g[lane]] = before[lane] + count[lane];
                    const uint64_t k = base[(size_t)g[lane] * n_tiles + tile] + before[lane] + below[lane];
                    perm[k] = r;
                    sl[k] = (uint32_t)(seq_off[r + 1] - seq_off[r]);
                    ql[k] = (uint32_t)(qual_off[r + 1] - qual_off[r]);
                }
            }
    }
    uint64_t* so_out = exact<uint64_t>(n + 1);
    uint64_t* qo_out = exact<uint64_t>(n + 1);
    so_out[0] = qo_out[0] = 0;
    for (uint32_t k = 0; k < n; k++) {
        so_out[k + 1] = so_out[k] + sl[k];
        qo_out[k + 1] = qo_out[k] + ql[k];
    }
    bg_fastq_record_t* recs_out = exact<bg_fastq_record_t>(n);
    uint8_t* seq_out = exact<uint8_t>(so_out[n]);
    uint8_t* qual_out = exact<uint8_t>(qo_out[n]);
    bg_alignment_t* hit_split = exact<bg_alignment_t>(n);
    for (uint32_t k = 0; k < n; k++) {
        const uint64_t r = perm[k];
        for (uint32_t lane = 0; lane < 16; lane++) {
            fq_copy_record(recs[r], seq + seq_off[r], (uint32_t)(seq_off[r + 1] - seq_off[r]), qual + qual_off[r],
                           (uint32_t)(qual_off[r + 1] - qual_off[r]), k, so_out[k], qo_out[k], recs_out, seq_out, so_out, qual_out, qo_out, lane, 16);
            ((uint32_t*)(hit_split + k))[lane] = ((const uint32_t*)(hit_out + r))[lane];
        }
    }
    std::vector<uint64_t> bin_off(ng + 1);
    for (uint32_t g = 0; g <= ng; g++) bin_off[g] = base[(size_t)g * n_tiles];

    FILE* o = fopen(argv[2], "wb");
    fwrite(bin, 4, n, o);
    fwrite(hit_out, sizeof(bg_alignment_t), n, o);
    fwrite(pat_out, 4, n, o);
    fwrite(recs_out, sizeof(bg_fastq_record_t), n, o);
    fwrite(so_out, 8, n + 1, o);
    fwrite(qo_out, 8, n + 1, o);
    fwrite(seq_out, 1, so_out[n], o);
    fwrite(qual_out, 1, qo_out[n], o);
    fwrite(hit_split, sizeof(bg_alignment_t), n, o);
    fwrite(perm, 8, n, o);
    fwrite(bin_off.data(), 8, ng + 1, o);
    fclose(o);
    for (void* p : {(void*)pat_bin, (void*)hits, (void*)split_bin, (void*)recs, (void*)seq, (void*)qual, (void*)seq_off, (void*)qual_off, (void*)bins,
                    (void*)bin, (void*)pat_out, (void*)hit_out, (void*)perm, (void*)sl, (void*)ql, (void*)so_out, (void*)qo_out, (void*)recs_out,
                    (void*)seq_out, (void*)qual_out, (void*)hit_split})
        free(p);
    return 0;
}
