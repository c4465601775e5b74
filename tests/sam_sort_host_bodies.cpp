// Stand-alone CPU program for tests/test_sam_sort_host_bodies.py: the __host__ __device__ bodies of csrc/sam_rule.h — placement,
// the sort key, the score, the ends and the entries that are sorted, the pass over runs, and the per-line copy — run on the
// host in the order the kernels of csrc/sam_sort.hip run them, on a batch read from a file; the test builds it with
// -fsanitize=address,undefined and compares what it writes with the restatement (tests/sam_sort_oracle.py).  What the device
// gets from rocPRIM is std::sort with md_less (a total order) and std::stable_sort by key here; what a shuffle gives the
// score kernel is a sum over the lanes.  The serial score must agree with the lanes' (exit status 3 if not).
// Input: 10 uint64 (n_reads, K, key flags, markdup flags, phred_offset, min_qual, n_contigs, bytes of qual, prefix bytes in front
// of the lines, bytes of the lines), contigs, hits[n K], strand[n K], recs[n], qual, prefix + lines, n K + 1 offsets of the
// lines.  Every buffer is allocated at exactly its size and the prefix is poisoned, so that a byte read or written outside a
// buffer stops the program.
// Output: dup[n], counts[4], key[n K], perm[n K], out_off[n K + 1], the permuted lines.
#include <sanitizer/asan_interface.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../rust-bio_amd/csrc/sam_rule.h"

template <typename T>
static T* exact(size_t count) {
    return (T*)malloc(count * sizeof(T) ? count * sizeof(T) : 1);
}
template <typename T>
static T* load(FILE* f, size_t count) {
    T* p = exact<T>(count);
    if (count && fread(p, sizeof(T), count, f) != count) exit(2);
    return p;
}

// the pass over runs of md_run_kernel
static void run_pass(const md_entry_t* sorted, uint64_t n, int words, bool paired, uint8_t* dup, uint64_t* counts) {
    for (uint64_t i = 0; i < n; i++) {
        if (!md_flagged(sorted, i, words)) continue;
        const uint64_t idx = sorted[i].idx;
        if (words == 4) {
            dup[2 * idx] = dup[2 * idx + 1] = 1;
            counts[1] += 2;
            counts[2] += 1;
        } else {
            dup[idx] = 1;
            counts[1] += 1;
            if (paired && md_group_has_pair_end(sorted, i)) counts[3] += 1;
        }
    }
}
static md_entry_t* sort_entries(const md_entry_t* e, uint64_t n) {
    std::vector<uint64_t> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return md_less(e[a], e[b]); });
    md_entry_t* sorted = exact<md_entry_t>(n);
    for (uint64_t i = 0; i < n; i++) sorted[i] = e[order[i]];
    return sorted;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    uint64_t h[10];
    if (!f || fread(h, 8, 10, f) != 10) return 2;
    const uint64_t n = h[0], K = h[1], n_contigs = h[6], n_slots = n * K, prefix = h[8], text_bytes = h[9];
    const uint32_t key_flags = (uint32_t)h[2], phred = (uint32_t)h[4], min_qual = (uint32_t)h[5];
    const bool paired = (h[3] & BG_SAM_PAIRED) != 0;
    bg_sam_contig_t* contigs = load<bg_sam_contig_t>(f, n_contigs);
    bg_seed_hit_t* hits = load<bg_seed_hit_t>(f, n_slots);
    uint8_t* strand = load<uint8_t>(f, n_slots);
    bg_fastq_record_t* recs = load<bg_fastq_record_t>(f, n);
    uint8_t* qual = load<uint8_t>(f, h[7]);
    uint8_t* in = load<uint8_t>(f, prefix + text_bytes);
    ASAN_POISON_MEMORY_REGION(in, prefix & ~(uint64_t)7);
    uint64_t* in_off = load<uint64_t>(f, n_slots + 1);
    fclose(f);

    // ---- markdup: the score kernel's lanes, the entry kernel, the two sorts and passes
    uint32_t* score = exact<uint32_t>(n);
    for (uint64_t r = 0; r < n; r++) {
        const uint8_t* q = qual + recs[r].qual_off;
        uint32_t s = 0;
        for (uint32_t lane = 0; lane < MD_G; lane++) s += md_score_share(q, recs[r].qual_len, phred, min_qual, lane, MD_G);
        if (s != md_score_serial(q, recs[r].qual_len, phred, min_qual)) return 3;
        score[r] = s;
    }
    md_entry_t* ends = exact<md_entry_t>(n);
    md_entry_t* pairs = exact<md_entry_t>(paired ? n / 2 : 0);
    uint8_t* dup = exact<uint8_t>(n);
    uint64_t counts[4] = {0, 0, 0, 0};
    for (uint64_t r = 0; r < n; r++) {
        dup[r] = 0;
        const md_end_t e = md_end(contigs, n_contigs, hits[r * K], strand[r * K]);
        counts[0] += e.contig >= 0;
        uint32_t kind = MD_KIND_FRAGMENT;
        if (paired) {
            const uint64_t m = r ^ 1;
            const md_end_t em = md_end(contigs, n_contigs, hits[m], strand[m]);
            if (e.contig >= 0 && em.contig >= 0) kind = MD_KIND_PAIR_END;
            if (!(r & 1)) pairs[r >> 1] = md_pair_entry(e, em, score[r], score[m], r >> 1);
        }
        ends[r] = md_end_entry(e, kind, score[r], r);
    }
    if (paired) {
        md_entry_t* sorted = sort_entries(pairs, n / 2);
        run_pass(sorted, n / 2, 4, paired, dup, counts);
        free(sorted);
    }
    md_entry_t* sorted = sort_entries(ends, n);
    run_pass(sorted, n, 2, paired, dup, counts);
    free(sorted);

    // ---- keys, the stable sort, the running sum
    uint64_t* key = exact<uint64_t>(n_slots);
    for (uint64_t s = 0; s < n_slots; s++) key[s] = sam_rule_key(key_flags, (uint32_t)K, contigs, n_contigs, hits, strand, s);
    uint64_t* perm = exact<uint64_t>(n_slots);
    std::iota(perm, perm + n_slots, 0);
    std::stable_sort(perm, perm + n_slots, [&](uint64_t a, uint64_t b) { return key[a] < key[b]; });
    uint64_t* out_off = exact<uint64_t>(n_slots + 1);
    out_off[0] = 0;
    for (uint64_t j = 0; j < n_slots; j++) out_off[j + 1] = out_off[j] + (in_off[perm[j] + 1] - in_off[perm[j]]);
    if (out_off[n_slots] != text_bytes) return 2;

    // ---- the copy: a group of SAM_COPY_G lanes a line, or chunks of SAM_CHUNK_VECS vectors by 256 lanes for a long one
    uint8_t* out = exact<uint8_t>(text_bytes);
    const uint8_t* lines = in + prefix;
    for (uint64_t j = 0; j < n_slots; j++) {
        const uint64_t i = perm[j], s = in_off[i], len = in_off[i + 1] - s;
        if (len == 0) continue;
        // the plan covers the line exactly
        const sam_copy_plan_t p = sam_copy_plan((uint32_t)((uintptr_t)(out + out_off[j]) & 15u), len);
        if (p.head + 16 * p.body + p.tail != len || p.head > 15 || p.tail > 15 || (((uintptr_t)(out + out_off[j]) + p.head) & 15u && p.body)) return 3;
        if (len <= SAM_LONG_LINE) {
            for (uint32_t lane = 0; lane < SAM_COPY_G; lane++) sam_copy_line(lines + s, out + out_off[j], len, lane, SAM_COPY_G, 0, UINT64_MAX, true);
        } else {
            for (uint64_t c = 0; c * SAM_CHUNK_VECS <= (len >> 4); c++)
                for (uint32_t lane = 0; lane < 256; lane++)
                    sam_copy_line(lines + s, out + out_off[j], len, lane, 256, c * SAM_CHUNK_VECS, (c + 1) * SAM_CHUNK_VECS, c == 0);
        }
    }

    ASAN_UNPOISON_MEMORY_REGION(in, prefix & ~(uint64_t)7);
    FILE* o = fopen(argv[2], "wb");
    fwrite(dup, 1, n, o);
    fwrite(counts, 8, 4, o);
    fwrite(key, 8, n_slots, o);
    fwrite(perm, 8, n_slots, o);
    fwrite(out_off, 8, n_slots + 1, o);
    fwrite(out, 1, text_bytes, o);
    fclose(o);
    for (void* p : {(void*)contigs, (void*)hits, (void*)strand, (void*)recs, (void*)qual, (void*)in, (void*)in_off, (void*)score, (void*)ends,
                    (void*)pairs, (void*)dup, (void*)key, (void*)perm, (void*)out_off, (void*)out})
        free(p);
    return 0;
}
