// Stand-alone CPU program for tests/test_myers_long_host_bodies.py: the per-job bodies of csrc/myers_long.hip (ml_best_job,
// ml_find_all_job: __host__ __device__) run on the host, job by job, on a batch read from a file; the test builds it with
// -fsanitize=address,undefined and compares what it writes with the restatement.  Input: seven uint32 (n_pat, k, max_hits,
// n_texts, text bytes, ops_stride, blocks), m[n_pat] uint32, the blocks' peq tables (256 uint64 each), n_texts + 1 uint64
// offsets, the text.  The text is placed 3 bytes past an 8-byte boundary.  Output: best records, the strided operations,
// find-all records and counts with starts and with ends only, the overflow flag.  Every job runs in the instantiation its
// launch would have, on scratch of exactly the size ml_run reserves for it.
#include "../rust-bio_amd/csrc/myers_long.hip"
thread_local std::string bg_tls_error;
int bg_reserve(void**, size_t*, size_t) { return 0; }

template <int NB>
static void run_job(MlArgs a, const MlJob& j, const uint64_t* peq, uint32_t ring, bg_alignment_t* best, bg_alignment_t* fa, uint32_t* cnt,
                    bg_alignment_t* fe, uint32_t* cnte) {
    const uint64_t pitch = 64;
    std::vector<uint64_t> spv((size_t)ring * NB * pitch), smv((size_t)ring * NB * pitch);
    std::vector<uint32_t> sd((size_t)ring * pitch);
    a.s_pv = spv.data(); a.s_mv = smv.data(); a.s_dist = sd.data(); a.pitch = pitch;
    a.aln = best; ml_best_job<NB>(a, j, peq, a.cls);
    a.aln = fa; a.count = cnt; ml_find_all_job<NB, false>(a, j, peq, a.cls);
    a.aln = fe; a.count = cnte; ml_find_all_job<NB, true>(a, j, peq, a.cls);
}

int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    uint32_t hdr[7];
    if (fread(hdr, 4, 7, f) != 7) return 2;
    uint32_t n_pat = hdr[0], k = hdr[1], max_hits = hdr[2], n_texts = hdr[3], tb = hdr[4], stride = hdr[5], blocks = hdr[6];
    std::vector<uint32_t> m(n_pat);
    if (fread(m.data(), 4, n_pat, f) != n_pat) return 2;
    std::vector<uint64_t> peq((size_t)blocks * 256);
    if (fread(peq.data(), 8, peq.size(), f) != peq.size()) return 2;
    std::vector<uint64_t> off(n_texts + 1);
    if (fread(off.data(), 8, n_texts + 1, f) != n_texts + 1) return 2;
    std::vector<uint64_t> textbuf((tb + 3) / 8 + 2);
    uint8_t* text = (uint8_t*)textbuf.data() + 3;
    if (fread(text, 1, tb, f) != tb) return 2;
    fclose(f);
    std::vector<uint64_t> blk_off(n_pat + 1, 0);
    for (uint32_t p = 0; p < n_pat; p++) blk_off[p + 1] = blk_off[p] + (m[p] + 63) / 64;
    if (ml_check(peq.data(), blk_off.data(), m.data(), n_pat) != BG_OK || blk_off[n_pat] != blocks) return 3;
    MlTables T;
    ml_tables(peq.data(), m.data(), n_pat, k, T);
    uint64_t nj = (uint64_t)n_texts * n_pat;
    std::vector<bg_alignment_t> best(nj), fa(nj * max_hits), fe(nj * max_hits);
    std::vector<uint32_t> cnt(nj), cnte(nj);
    std::vector<uint8_t> ops(nj * stride + 1, 0);
    int flag = 0;
    MlArgs a = {};
    a.text = text; a.off = off.data(); a.n_texts = n_texts;
    a.peqc = (const uint64_t*)T.blob.data(); a.pm = T.pm.data(); a.pb = T.pb.data(); a.cls = T.blob.data() + T.off_cls;
    a.n_pat = n_pat; a.n_cls = T.n_cls; a.g0 = 0; a.gn = n_pat; a.k = k; a.max_hits = max_hits;
    a.ops = ops.data(); a.ops_stride = stride; a.flag = &flag;
    for (uint64_t t = 0; t < n_texts; t++)
        for (uint32_t p = 0; p < n_pat; p++) {
            MlJob j;
            j.job = t * n_pat + p; j.lane = j.job % 64; j.m = m[p];
            j.tb = text + off[t]; j.te = text + off[t + 1]; j.ylen = (uint32_t)(off[t + 1] - off[t]);
            const uint64_t* q = a.peqc + (size_t)T.pb[p] * a.n_cls;
            const uint32_t ring = m[p] + std::min(k, m[p]) + 2;
            switch (ml_width(T.pb[p + 1] - T.pb[p])) {
                case 1: run_job<1>(a, j, q, ring, best.data(), fa.data(), cnt.data(), fe.data(), cnte.data()); break;
                case 2: run_job<2>(a, j, q, ring, best.data(), fa.data(), cnt.data(), fe.data(), cnte.data()); break;
                case 3: run_job<3>(a, j, q, ring, best.data(), fa.data(), cnt.data(), fe.data(), cnte.data()); break;
                case 4: run_job<4>(a, j, q, ring, best.data(), fa.data(), cnt.data(), fe.data(), cnte.data()); break;
                case 8: run_job<8>(a, j, q, ring, best.data(), fa.data(), cnt.data(), fe.data(), cnte.data()); break;
                default: run_job<16>(a, j, q, ring, best.data(), fa.data(), cnt.data(), fe.data(), cnte.data()); break;
            }
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
