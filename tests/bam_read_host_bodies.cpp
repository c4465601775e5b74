// Stand-alone CPU program for tests/test_bam_read_host_bodies.py and the GPU tests of reading BAM: the __host__ __device__
// bodies of csrc/bam_read_rule.h (and bai_voff_blocks of csrc/bam_index_rule.h) run on the host, in the steps the kernels of
// csrc/bam_read.hip take.  The record table: bamr_verdict at EVERY position from body_off on (the candidates), a successor per
// candidate, chain membership by bamr_rounds() rounds of doubling, the rows, the verdict on the chain's end.  The reads: the
// slot check and the lengths, then per kept record lanes 0 .. 15 in turn through bamr_column_lane, the flags ORed, the record
// by bamr_read_record.  The keys by bamr_key, virtual offsets by bai_voff_blocks.  The first test builds it with
// -fsanitize=address,undefined.  Every stream, table and output column is a heap allocation of exactly its size, so a body
// that reads or writes one byte outside stops the program.
// Input: uint64 cases; per case uint64 len, body_off, n_ref, flags, require, exclude, n_contigs, n_off (0: the walk's table),
// n_blocks, n_voff; the stream; n_contigs x bg_sam_contig_t; n_off offsets; 2 x (n_blocks + 1) rows (block_off, out_off) where
// n_blocks != UINT64_MAX; n_voff stream offsets.
// Output per case: int64 rc, uint64 n_records, n_candidates, first_bad of the table; its n_records + 1 rows if rc == 0.  If a
// table is at hand (the walk's or the given one): int64 rc, uint64 first_bad, n_reads, seq_bytes, qual_bytes of the reads; if
// rc == 0 the records, seq, seq_off, qual, qual_off, src; int64 rc, uint64 first_bad of the keys, the keys if rc == 0.  Then
// n_voff virtual offsets.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rust-bio_amd/csrc/bam_read_rule.h"

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
template <typename T>
static void put(FILE* o, const T* p, size_t count) {
    if (count) fwrite(p, sizeof(T), count, o);
}
static const int G = 16;

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint64_t* n_cases = load<uint64_t>(f, 1);
    for (uint64_t c = 0; c < *n_cases; c++) {
        uint64_t* hd = load<uint64_t>(f, 10);
        const uint64_t len = hd[0], body_off = hd[1], n_ref = hd[2], n_contigs = hd[6], n_off = hd[7], n_blocks = hd[8], n_voff = hd[9];
        const bg_bam_reads_t prm = {(uint32_t)hd[3], (uint16_t)hd[4], (uint16_t)hd[5]};
        uint8_t* s = load<uint8_t>(f, len);
        bg_sam_contig_t* contigs = load<bg_sam_contig_t>(f, n_contigs);
        uint64_t* given = load<uint64_t>(f, n_off);
        const bool framed = n_blocks != UINT64_MAX;
        uint64_t* block_off = load<uint64_t>(f, framed ? n_blocks + 1 : 0);
        uint64_t* out_off = load<uint64_t>(f, framed ? n_blocks + 1 : 0);
        uint64_t* ask = load<uint64_t>(f, n_voff);

        // ---- the table: candidates, successors, doubling, rows, the end
        std::vector<uint64_t> pos;
        uint64_t size;
        for (uint64_t p = body_off; p < len; p++)
            if (bamr_verdict(s, len, p, n_ref, &size) == BG_OK) pos.push_back(p);
        const uint64_t n = pos.size();
        std::vector<uint32_t> jump[2] = {std::vector<uint32_t>(n), std::vector<uint32_t>(n)};
        std::vector<uint8_t> chain(n), tail(n);
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t target = pos[i] + 4 + bai_get32(s + pos[i]);
            uint64_t lo = i + 1, hi = n;
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (pos[mid] < target) lo = mid + 1;
                else hi = mid;
            }
            const bool found = lo < n && pos[lo] == target;
            jump[0][i] = found ? (uint32_t)lo : BAMR_NONE;
            tail[i] = !found;
            chain[i] = i == 0 && pos[0] == body_off;
        }
        const uint32_t rounds = len > body_off ? bamr_rounds(len - body_off) : 0;
        for (uint32_t k = 0; k < rounds; k++) {
            const std::vector<uint32_t>& jin = jump[k & 1];
            std::vector<uint32_t>& jout = jump[(k + 1) & 1];
            for (uint64_t i = 0; i < n; i++) {
                const uint32_t j = jin[i];
                if (j == BAMR_NONE) {
                    jout[i] = BAMR_NONE;
                    continue;
                }
                if (chain[i]) chain[j] = 1;
                jout[i] = jin[j];
            }
        }
        std::vector<uint64_t> off;
        uint64_t last = UINT64_MAX;
        for (uint64_t i = 0; i < n; i++)
            if (chain[i]) {
                off.push_back(pos[i]);
                if (tail[i]) last = i;
            }
        const uint64_t end = last == UINT64_MAX ? body_off : pos[last] + 4 + bai_get32(s + pos[last]);
        int64_t rc = end == len ? BG_OK : BG_ERR_INVALID_ARG;
        const uint64_t head[3] = {off.size(), n, rc ? off.size() : UINT64_MAX};
        fwrite(&rc, 8, 1, o);
        fwrite(head, 8, 3, o);
        off.push_back(len);
        if (!rc) put(o, off.data(), off.size());

        // ---- the reads and the keys over an exact-size copy of the table
        const bool have = n_off || !rc;
        const uint64_t m = n_off ? n_off - 1 : off.size() - 1;
        uint64_t* tab = make<uint64_t>(m + 1);
        if (have) memcpy(tab, n_off ? given : off.data(), 8 * (m + 1));
        if (have) {
            uint64_t bad = UINT64_MAX, n_reads = 0, seq_bytes = 0, qual_bytes = 0;
            std::vector<uint64_t> rank(m + 1), soff(m + 1), qoff(m + 1);
            std::vector<uint8_t> keep(m);
            for (uint64_t i = 0; i < m; i++) {
                rank[i] = n_reads;
                soff[i] = seq_bytes;
                qoff[i] = qual_bytes;
                if (tab[i + 1] == tab[i]) continue;
                if (!bamr_slot_ok(s, tab[i], tab[i + 1], n_ref)) {
                    if (bad == UINT64_MAX) bad = i;
                    continue;
                }
                const bamr_fields_t fl = bamr_fields(s + tab[i]);
                if (!bamr_kept(fl.flag, prm)) continue;
                keep[i] = 1;
                n_reads++;
                seq_bytes += fl.l_seq;
                qual_bytes += bamr_qual_len(s + tab[i], fl);
            }
            rank[m] = n_reads;
            soff[m] = seq_bytes;
            qoff[m] = qual_bytes;
            rc = bad == UINT64_MAX ? BG_OK : BG_ERR_INVALID_ARG;
            const uint64_t rhead[4] = {bad, n_reads, seq_bytes, qual_bytes};
            fwrite(&rc, 8, 1, o);
            fwrite(rhead, 8, 4, o);
            if (!rc) {
                bg_fastq_record_t* recs = make<bg_fastq_record_t>(n_reads);
                uint8_t* seq = make<uint8_t>(seq_bytes);
                uint8_t* qual = make<uint8_t>(qual_bytes);
                uint64_t* seq_off = make<uint64_t>(n_reads + 1);
                uint64_t* qual_off = make<uint64_t>(n_reads + 1);
                uint64_t* src = make<uint64_t>(n_reads);
                for (uint64_t i = 0; i < m; i++) {
                    if (!keep[i]) continue;
                    const uint8_t* r = s + tab[i];
                    const bamr_fields_t fl = bamr_fields(r);
                    const uint32_t ql = bamr_qual_len(r, fl);
                    const bool rev = bamr_reversed(fl.flag, prm);
                    uint32_t flags = 0;
                    for (uint32_t lane = 0; lane < (uint32_t)G; lane++) {
                        flags |= bamr_column_lane<true>(r + fl.seq_at, fl.l_seq, rev, seq + soff[i], lane, G);
                        if (ql) flags |= bamr_column_lane<false>(r + fl.qual_at, ql, rev, qual + qoff[i], lane, G) << 1;
                    }
                    const uint64_t j = rank[i];
                    recs[j] = bamr_read_record(r, tab[i], fl, ql, soff[i], qoff[i], flags & 1u, flags & 2u);
                    seq_off[j] = soff[i];
                    qual_off[j] = qoff[i];
                    src[j] = i;
                }
                seq_off[n_reads] = seq_bytes;
                qual_off[n_reads] = qual_bytes;
                put(o, recs, n_reads);
                put(o, seq, seq_bytes);
                put(o, seq_off, n_reads + 1);
                put(o, qual, qual_bytes);
                put(o, qual_off, n_reads + 1);
                put(o, src, n_reads);
                free(src);
                free(qual_off);
                free(seq_off);
                free(qual);
                free(seq);
                free(recs);
            }
            // keys: the slot check against the contig table
            bad = UINT64_MAX;
            uint64_t* key = make<uint64_t>(m);
            for (uint64_t i = 0; i < m; i++) {
                if (tab[i + 1] != tab[i] && !bamr_slot_ok(s, tab[i], tab[i + 1], n_contigs)) {
                    if (bad == UINT64_MAX) bad = i;
                    key[i] = UINT64_MAX;
                    continue;
                }
                key[i] = bamr_key(s + tab[i], tab[i + 1] - tab[i], contigs);
            }
            rc = bad == UINT64_MAX ? BG_OK : BG_ERR_INVALID_ARG;
            fwrite(&rc, 8, 1, o);
            fwrite(&bad, 8, 1, o);
            if (!rc) put(o, key, m);
            free(key);
        }
        for (uint64_t q = 0; q < n_voff; q++) {
            const uint64_t v = bai_voff_blocks(ask[q], n_blocks, block_off, out_off);
            fwrite(&v, 8, 1, o);
        }
        free(tab);
        free(ask);
        free(out_off);
        free(block_off);
        free(given);
        free(contigs);
        free(s);
        free(hd);
    }
    free(n_cases);
    fclose(o);
    fclose(f);
    return 0;
}
