// Stand-alone CPU program for tests/test_fastq_qual_host_bodies.py: the lane-group bodies of csrc/fastq_qual.hip
// (csrc/fastq_qual_rule.h, __host__ __device__) run on the host, lane by lane, on a batch read from a file; the test builds it
// with -fsanitize=address,undefined and compares what it writes with the restatement (tests/fastq_qual_oracle.py).  What a
// kernel gets from a shuffle — a scan, a minimum, a maximum, a sum over the group — is computed here from the other lanes'
// values; the order of the steps is the kernels'.  The serial statement of the same header runs next to it and must agree
// (exit status 3 if not).
// Input: 4 uint32 (n, G, prefix bytes of qual, bytes of qual behind the prefix), bg_qual_cut_t, bg_qual_select_t, 1 uint32
// (a weight table is given), weight[256], the quality buffer with its prefix, n + 1 quality offsets.  Every buffer is
// allocated at exactly its size, so that a byte read or written outside it stops the program.
// Output: cut_out[n], stats_out[n], bin_out[n], 3 uint64 (reads cut, symbols removed, records passed).
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rust-bio_amd/csrc/fastq_qual_rule.h"

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

static uint32_t G;

static std::vector<int32_t> scan(const std::vector<int32_t>& v) {
    std::vector<int32_t> p(G);
    int32_t run = 0;
    for (uint32_t lane = 0; lane < G; lane++) p[lane] = run += v[lane];
    return p;
}
template <typename F>
static uint32_t lowest(F f) {
    uint32_t m = 0xFFFFFFFFu;
    for (uint32_t lane = 0; lane < G; lane++) m = std::min<uint32_t>(m, f(lane));
    return m;
}

static uint32_t runsum(const uint8_t* q, uint32_t L, uint32_t phred, uint32_t cutoff_in, bool from_end) {
    const int32_t cutoff = ql_run_cutoff(cutoff_in);
    ql_run st = ql_run_start();
    for (uint64_t t0 = 0; t0 < L && !st.stopped; t0 += G) {
        std::vector<int32_t> d(G);
        for (uint32_t lane = 0; lane < G; lane++) d[lane] = ql_run_term(q, L, phred, cutoff, from_end, t0, lane);
        const std::vector<int32_t> p = scan(d);
        const uint32_t first_neg = lowest([&](uint32_t lane) { return ql_run_neg(st, p[lane], L, t0, lane, G); });
        uint32_t key = 0;
        for (uint32_t lane = 0; lane < G; lane++) key = std::max(key, ql_run_key(p[lane], L, t0, lane, first_neg));
        ql_run_carry(st, t0, first_neg, key, p[G - 1], G);
    }
    return (uint32_t)st.cnt;
}

static uint32_t window(const uint8_t* q, uint32_t L, uint32_t phred, uint32_t cutoff, uint32_t win) {
    if (L == 0) return 0;
    const uint32_t W = win < L ? win : L;
    const uint64_t threshold = (uint64_t)cutoff * W;
    uint64_t D = 0, e = L;
    for (uint32_t lane = 0; lane < G; lane++) D += ql_win_share(q, W, phred, lane, G);
    bool found = false;
    for (uint64_t j0 = 0; j0 + W <= L; j0 += G) {
        std::vector<int32_t> d(G);
        for (uint32_t lane = 0; lane < G; lane++) d[lane] = ql_win_term(q, L, W, phred, j0, lane);
        const std::vector<int32_t> incl = scan(d);
        const uint32_t f = lowest([&](uint32_t lane) { return ql_win_fails(D, incl[lane] - d[lane], threshold, L, W, j0, lane, G); });
        if (f < G) {
            e = j0 + f;
            found = true;
            break;
        }
        D = (uint64_t)((int64_t)D + incl[G - 1]);
    }
    while (found) {
        const uint32_t f = lowest([&](uint32_t lane) { return ql_back_stops(q, e, phred, cutoff, lane, G); });
        e -= f < G ? f : G;
        if (f < G) break;
    }
    return (uint32_t)e;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    uint32_t h[4], has_weight;
    bg_qual_cut_t cp;
    bg_qual_select_t sp;
    if (!f || fread(h, 4, 4, f) != 4 || fread(&cp, sizeof cp, 1, f) != 1 || fread(&sp, sizeof sp, 1, f) != 1 || fread(&has_weight, 4, 1, f) != 1)
        return 2;
    const uint32_t n = h[0];
    G = h[1];
    uint32_t* weight = load<uint32_t>(f, 256);
    uint8_t* qual = load<uint8_t>(f, (size_t)h[2] + h[3]);
    ASAN_POISON_MEMORY_REGION(qual, h[2] & ~7u);
    uint64_t* qual_off = load<uint64_t>(f, n + 1);
    fclose(f);

    bg_alignment_t* cut_out = exact<bg_alignment_t>(n);
    bg_qual_stats_t* stats_out = exact<bg_qual_stats_t>(n);
    uint32_t* bin_out = exact<uint32_t>(n);
    std::vector<char> own(n);
    uint64_t totals[3] = {0, 0, 0};
    for (uint32_t r = 0; r < n; r++) {
        const uint8_t* q = qual + qual_off[r];
        const uint32_t L = (uint32_t)(qual_off[r + 1] - qual_off[r]);
        // ---- cut
        uint32_t b = 0, e = L;
        if (cp.method_5p == BG_QCUT_RUNSUM) b = runsum(q, L, cp.phred_offset, cp.cutoff_5p, false);
        if (cp.method_3p == BG_QCUT_RUNSUM) e = L - runsum(q, L, cp.phred_offset, cp.cutoff_3p, true);
        if (cp.method_3p == BG_QCUT_WINDOW) e = window(q, L, cp.phred_offset, cp.cutoff_3p, cp.window);
        if (e < b) e = b;
        uint32_t sb, se;
        ql_cut_serial(q, L, cp, &sb, &se);
        if (sb != b || se != e) return 3;
        for (uint32_t lane = 0; lane < 16; lane++) ((uint32_t*)(cut_out + r))[lane] = ql_cut_word(L, b, e, lane);
        totals[0] += L - (e - b) != 0;
        totals[1] += L - (e - b);
        // ---- select: the lanes' shares, the butterfly of the group
        std::vector<bg_qual_stats_t> s(G), t(G);
        for (uint32_t lane = 0; lane < G; lane++) s[lane] = ql_stats_share(q, L, sp.phred_offset, sp.low_q, has_weight ? weight : nullptr, lane, G);
        for (uint32_t o = G / 2; o; o >>= 1) {
            for (uint32_t lane = 0; lane < G; lane++) t[lane] = ql_stats_merge(s[lane], s[lane ^ o]);
            s = t;
        }
        for (uint32_t lane = 1; lane < G; lane++)
            if (memcmp(&s[lane], &s[0], sizeof s[0]) != 0) return 3;  // every lane of the group holds the read's sums
        const bg_qual_stats_t st = ql_stats_close(s[0], L), serial = ql_stats_serial(q, L, sp.phred_offset, sp.low_q, has_weight ? weight : nullptr);
        if (memcmp(&st, &serial, sizeof st) != 0) return 3;
        for (uint32_t lane = 0; lane < 8; lane++) ((uint32_t*)(stats_out + r))[lane] = ql_stats_word(st, lane);
        own[r] = ql_passes(sp, st, has_weight != 0);
    }
    for (uint32_t r = 0; r < n; r++) {
        const bool keep = ql_keeps(sp.flags, own[r], (sp.flags & BG_QSEL_PAIRED) ? own[r ^ 1] : false);
        bin_out[r] = keep ? 0u : 1u;
        totals[2] += keep;
    }

    FILE* o = fopen(argv[2], "wb");
    fwrite(cut_out, sizeof(bg_alignment_t), n, o);
    fwrite(stats_out, sizeof(bg_qual_stats_t), n, o);
    fwrite(bin_out, 4, n, o);
    fwrite(totals, 8, 3, o);
    fclose(o);
    for (void* p : {(void*)weight, (void*)qual, (void*)qual_off, (void*)cut_out, (void*)stats_out, (void*)bin_out}) free(p);
    return 0;
}
