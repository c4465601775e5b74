// Stand-alone CPU program for tests/test_myers_host_bodies.py: the per-job bodies of csrc/myers.hip (my_best_job,
// my_find_all_job: __host__ __device__) run on the host, job by job, on a batch read from a file; the test builds it with
// -fsanitize=address,undefined and compares what it writes with the restatement.  Input: six uint32 (n_pat, k, max_hits,
// n_texts, text bytes, ops_stride), the bg_myers_pattern_t array, n_texts + 1 uint64 offsets, the text.  The text is placed 3
// bytes past an 8-byte boundary.  Output: best records, the strided operations, find-all records and counts with starts and
// with ends only, the overflow flag.
#include "../rust-bio_amd/csrc/myers.hip"
thread_local std::string bg_tls_error;
int bg_reserve(void**, size_t*, size_t) { return 0; }
#include <fstream>
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    uint32_t hdr[6];  // n_pat, k, max_hits, n_texts, text_bytes, ops_stride
    fread(hdr, 4, 6, f);
    uint32_t n_pat = hdr[0], k = hdr[1], max_hits = hdr[2], n_texts = hdr[3], tb = hdr[4], stride = hdr[5];
    std::vector<bg_myers_pattern_t> pats(n_pat);
    fread(pats.data(), sizeof(bg_myers_pattern_t), n_pat, f);
    std::vector<uint64_t> off(n_texts + 1);
    fread(off.data(), 8, n_texts + 1, f);
    std::vector<uint64_t> textbuf((tb + 3) / 8 + 2);
    uint8_t* text = (uint8_t*)textbuf.data() + 3;
    fread(text, 1, tb, f);
    fclose(f);
    MyTables T;
    my_tables(pats.data(), n_pat, k, T);
    uint64_t nj = (uint64_t)n_texts * n_pat;
    uint64_t pitch = 64;
    std::vector<uint64_t> spv(T.max_ring * pitch), smv(T.max_ring * pitch);
    std::vector<uint8_t> sd(T.max_ring * pitch);
    std::vector<bg_alignment_t> best(nj), fa(nj * max_hits), fe(nj * max_hits);
    std::vector<uint32_t> cnt(nj), cnte(nj);
    std::vector<uint8_t> ops(nj * stride + 1, 0);
    int flag = 0;
    MyArgs a = {};
    a.text = text; a.off = off.data(); a.n_texts = n_texts;
    a.peqc = (const uint64_t*)T.blob.data(); a.pm = (const uint32_t*)(T.blob.data() + T.off_pm); a.cls = T.blob.data() + T.off_cls;
    a.n_pat = n_pat; a.n_cls = T.n_cls; a.g0 = 0; a.gn = n_pat; a.k = k; a.max_hits = max_hits;
    a.s_pv = spv.data(); a.s_mv = smv.data(); a.s_dist = sd.data(); a.pitch = pitch;
    a.ops = ops.data(); a.ops_stride = stride; a.flag = &flag;
    for (uint64_t t = 0; t < n_texts; t++)
        for (uint32_t p = 0; p < n_pat; p++) {
            MyJob j;
            j.job = t * n_pat + p; j.lane = j.job % 64; j.pl = p; j.m = a.pm[p];
            j.tb = text + off[t]; j.te = text + off[t + 1]; j.ylen = (uint32_t)(off[t + 1] - off[t]);
            const uint64_t* peq = a.peqc + (size_t)p * a.n_cls;
            a.aln = best.data(); my_best_job(a, j, peq, a.cls);
            a.aln = fa.data(); a.count = cnt.data(); my_find_all_job<false>(a, j, peq, a.cls);
            a.aln = fe.data(); a.count = cnte.data(); my_find_all_job<true>(a, j, peq, a.cls);
        }
    FILE* o = fopen(argv[2], "wb");
    fwrite(best.data(), 64, nj, o); fwrite(ops.data(), 1, nj * stride, o);
    fwrite(fa.data(), 64, nj * max_hits, o); fwrite(cnt.data(), 4, nj, o);
    fwrite(fe.data(), 64, nj * max_hits, o); fwrite(cnte.data(), 4, nj, o);
    fwrite(&flag, 4, 1, o);
    fclose(o);
    printf("n_cls %u ring %u flag %d\n", T.n_cls, T.max_ring, flag);
    return 0;
}
