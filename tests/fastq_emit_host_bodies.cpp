// Stand-alone CPU program for tests/test_fastq_emit_host_bodies.py: the per-record bodies of csrc/fastq_emit.hip
// (csrc/fastq_emit_rule.h, __host__ __device__) run on the host, lane by lane, on a batch read from a file; the test builds it
// with -fsanitize=address,undefined and compares what it writes with the restatement (tests/fastq_write_oracle.py).
// Input: 18 uint32 (n, G, prefix bytes of text / seq / qual / out, bytes of text / seq / qual behind their prefixes, first,
// step, filter flags / min_len / max_len / max_n, n_pat, hits given), n records (their offsets include the prefixes), the
// three buffers with their prefixes, n + 1 sequence and quality offsets, the hits.  Every buffer is allocated at exactly its
// size, so that a byte read or written outside it stops the program; the prefix of a source is poisoned by hand (in whole
// 8-byte granules, which is what the shadow memory can express), the prefix of the output is checked to be untouched.
// Output: the staged and the direct text, n_lines + 1 offsets, keep[n], the kept count, the filter's five columns.
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rust-bio_amd/csrc/fastq_emit_rule.h"

template <typename T>
static T* exact(size_t count) {
    return (T*)malloc(count * sizeof(T));
}
// 16-byte aligned and of exactly `bytes` bytes (the sanitizer's red zone starts at the byte behind them)
static char* aligned_exact(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0) return (char*)malloc(0);
    if (posix_memalign(&p, 16, bytes)) exit(2);
    return (char*)p;
}
static uint8_t* source(FILE* f, uint32_t prefix, uint32_t bytes) {
    uint8_t* p = exact<uint8_t>((size_t)prefix + bytes);
    if (fread(p, 1, (size_t)prefix + bytes, f) != (size_t)prefix + bytes) exit(2);
    ASAN_POISON_MEMORY_REGION(p, prefix & ~7u);
    return p;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    uint32_t h[18];
    if (!f || fread(h, 4, 18, f) != 18) return 2;
    const uint32_t n = h[0], G = h[1], a_out = h[5], first = h[9], step = h[10], n_pat = h[15];
    const bg_fastq_filter_t flt = {h[11], h[12], h[13], h[14]};
    bg_fastq_record_t* recs = exact<bg_fastq_record_t>(n);
    if (fread(recs, sizeof(bg_fastq_record_t), n, f) != n) return 2;
    const uint8_t* text = source(f, h[2], h[6]);
    const uint8_t* seq = source(f, h[3], h[7]);
    const uint8_t* qual = source(f, h[4], h[8]);
    uint64_t* seq_off = exact<uint64_t>(n + 1);
    uint64_t* qual_off = exact<uint64_t>(n + 1);
    if (fread(seq_off, 8, n + 1, f) != n + 1 || fread(qual_off, 8, n + 1, f) != n + 1) return 2;
    bg_alignment_t* hits = nullptr;
    if (h[16]) {
        hits = exact<bg_alignment_t>((size_t)n * n_pat);
        if (fread(hits, sizeof(bg_alignment_t), (size_t)n * n_pat, f) != (size_t)n * n_pat) return 2;
    }
    fclose(f);

    // ---- emit: lengths, offsets, then every line staged and flushed, and written directly
    const uint32_t m = first < n ? (n - first - 1) / step + 1 : 0;
    std::vector<uint64_t> off(m + 1, 0);
    for (uint32_t j = 0; j < m; j++) off[j + 1] = off[j] + fq_line_len(recs[first + j * step]);
    const uint64_t total = off[m];
    char* out = aligned_exact(a_out + total);
    char* direct = aligned_exact(a_out + total);
    memset(out, 0xA5, a_out);
    memset(direct, 0xA5, a_out);
    for (uint32_t j = 0; j < m; j++) {
        const bg_fastq_record_t& r = recs[first + j * step];
        const uint32_t len = (uint32_t)(off[j + 1] - off[j]);
        char* line = out + a_out + off[j];
        const uint32_t mis = (uint32_t)((uintptr_t)line & 15);
        char* stage_buf = aligned_exact(mis + len);
        for (uint32_t lane = 0; lane < G; lane++) fq_line_write(text, r, seq, qual, stage_buf + mis, lane, G);
        for (uint32_t lane = 0; lane < G; lane++) fq_line_flush(stage_buf + mis, line, len, lane, G);
        free(stage_buf);
        for (uint32_t lane = 0; lane < G; lane++) fq_line_write(text, r, seq, qual, direct + a_out + off[j], lane, G);
    }
    int prefix_ok = 1;
    for (uint32_t i = 0; i < a_out; i++) prefix_ok &= (uint8_t)out[i] == 0xA5 && (uint8_t)direct[i] == 0xA5;

    // ---- filter: pass, pair rule, ranks and offsets, copy (16 lanes per record, as the kernel)
    const bool count_n = flt.max_n != 0xFFFFFFFFu;
    std::vector<uint8_t> pass(n), keep(n);
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t sl = (uint32_t)(seq_off[r + 1] - seq_off[r]);
        uint32_t nc = 0;
        if (count_n)
            for (uint32_t lane = 0; lane < 16; lane++) nc += fq_count_n(seq + seq_off[r], sl, lane, 16);
        const bool trimmed = (flt.flags & (BG_FQF_DISCARD_UNTRIMMED | BG_FQF_DISCARD_TRIMMED)) && fq_trimmed(hits, r, n_pat);
        pass[r] = fq_passes(flt, sl, recs[r].check, trimmed, nc);
    }
    std::vector<uint64_t> rank(n + 1, 0), so(n + 1, 0), qo(n + 1, 0);
    for (uint32_t r = 0; r < n; r++) {
        keep[r] = fq_keeps(flt.flags, pass[r], (flt.flags & BG_FQF_PAIRED) ? pass[r ^ 1] : false);
        rank[r + 1] = rank[r] + keep[r];
        so[r + 1] = so[r] + (keep[r] ? seq_off[r + 1] - seq_off[r] : 0);
        qo[r + 1] = qo[r] + (keep[r] ? qual_off[r + 1] - qual_off[r] : 0);
    }
    const uint64_t nk = rank[n];
    bg_fastq_record_t* recs_out = exact<bg_fastq_record_t>(nk);
    uint8_t* seq_out = exact<uint8_t>(so[n]);
    uint8_t* qual_out = exact<uint8_t>(qo[n]);
    uint64_t* so_out = exact<uint64_t>(nk + 1);
    uint64_t* qo_out = exact<uint64_t>(nk + 1);
    so_out[nk] = so[n];
    qo_out[nk] = qo[n];
    for (uint32_t r = 0; r < n; r++)
        if (keep[r])
            for (uint32_t lane = 0; lane < 16; lane++)
                fq_copy_record(recs[r], seq + seq_off[r], (uint32_t)(seq_off[r + 1] - seq_off[r]), qual + qual_off[r],
                               (uint32_t)(qual_off[r + 1] - qual_off[r]), rank[r], so[r], qo[r], recs_out, seq_out, so_out, qual_out, qo_out, lane,
                               16);

    FILE* o = fopen(argv[2], "wb");
    fwrite(&prefix_ok, 4, 1, o);
    fwrite(&total, 8, 1, o);
    fwrite(out + a_out, 1, total, o);
    fwrite(direct + a_out, 1, total, o);
    fwrite(off.data(), 8, m + 1, o);
    fwrite(keep.data(), 1, n, o);
    fwrite(&nk, 8, 1, o);
    fwrite(recs_out, sizeof(bg_fastq_record_t), nk, o);
    fwrite(so_out, 8, nk + 1, o);
    fwrite(qo_out, 8, nk + 1, o);
    fwrite(seq_out, 1, so[n], o);
    fwrite(qual_out, 1, qo[n], o);
    fclose(o);
    for (void* p : {(void*)recs, (void*)text, (void*)seq, (void*)qual, (void*)seq_off, (void*)qual_off, (void*)hits, (void*)out, (void*)direct,
                    (void*)recs_out, (void*)seq_out, (void*)qual_out, (void*)so_out, (void*)qo_out})
        free(p);
    return 0;
}
