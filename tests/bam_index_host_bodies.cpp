// Stand-alone CPU program for tests/test_bam_index_host_bodies.py: the __host__ __device__ bodies of csrc/bam_index_rule.h — the
// decode of a record's fields at any address, the CIGAR walk, the checks, the virtual offset in both forms, the sizes and
// places of a reference's pieces, the stores, the window search — run on the host in the order of bam_index.hip's passes (a
// loop where the device has one lane per element, std::stable_sort where it has the radix sort); the test builds it with
// -fsanitize=address,undefined and compares what it writes with tests/bai_oracle.py.
// Input: uint64 cases; per case uint64 n_contigs and the bg_sam_contig_t table, uint64 n_slots and n_slots + 1 offsets, uint64
// table entries (0: closed form) and the block table, uint64 base, uint64 residue, the records' bytes.
// Every array is a heap allocation of exactly its size; the records and the index lie at an address = residue (mod 16) and end
// where their allocation ends, so that a byte read or written outside one stops the program.  The index is allocated at the
// size the sizing pass gives: a store behind it stops the program as well.
// Output per case: int64 status (0, 1 invalid, 2 unsupported), uint64 first_bad, uint64 bytes, the index.
#include <sanitizer/asan_interface.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rust-bio_amd/csrc/bam_index_rule.h"

template <typename T>
static T* load(FILE* f, size_t count) {
    T* p = (T*)malloc(count * sizeof(T) ? count * sizeof(T) : 1);
    if (count && fread(p, sizeof(T), count, f) != count) exit(2);
    return p;
}
// len bytes at an address = res (mod 16) that end where the allocation ends, the res bytes in front poisoned
static uint8_t* at_residue(size_t len, size_t res) {
    uint8_t* base = (uint8_t*)aligned_alloc(16, (res + len + 15) / 16 * 16);
    ASAN_POISON_MEMORY_REGION(base, res);
    ASAN_POISON_MEMORY_REGION(base + res + len, (res + len + 15) / 16 * 16 - (res + len));
    return base + res;
}
template <typename T>
static T* exact(size_t count) {  // count elements, not one more
    return (T*)malloc(count * sizeof(T) ? count * sizeof(T) : 1);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint64_t* n_cases = load<uint64_t>(f, 1);
    for (uint64_t t = 0; t < *n_cases; t++) {
        uint64_t* hc = load<uint64_t>(f, 1);
        const uint64_t n_contigs = *hc;
        bg_sam_contig_t* contigs = load<bg_sam_contig_t>(f, n_contigs);
        uint64_t* hs = load<uint64_t>(f, 1);
        const uint64_t n = *hs;
        uint64_t* off = load<uint64_t>(f, n + 1);
        uint64_t* ht = load<uint64_t>(f, 1);
        const uint64_t n_table = *ht;
        uint64_t* table = load<uint64_t>(f, n_table);
        const uint64_t* block_off = n_table ? table : nullptr;
        uint64_t* tail = load<uint64_t>(f, 2);
        const uint64_t base = tail[0], res = tail[1], total = off[n];
        if (n_table && n_table != (total + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD + 1) return 3;
        uint8_t* recs = at_residue(total, res);
        if (total && fread(recs, 1, total, f) != total) return 2;

        // 1. records: the non-empty slots, decoded into a dense list
        uint64_t bad = BAI_NONE;
        auto report = [&](uint64_t slot, int kind) { bad = std::min(bad, (slot << 2) | (uint64_t)kind); };
        uint64_t m = 0;
        for (uint64_t i = 0; i < n; i++) m += off[i + 1] > off[i];
        bai_rec_t* rec = exact<bai_rec_t>(m);
        for (uint64_t i = 0, j = 0; i < n; i++) {
            if (off[i + 1] <= off[i]) continue;
            rec[j].slot = i;
            const int kind = bai_decode(recs + off[i], off[i + 1] - off[i], contigs, n_contigs, &rec[j]);
            if (kind) report(i, kind);
            j++;
        }
        // 2. neighbours: the order, run heads, the references' records, the running maximum of (ref, end)
        uint64_t* ref_first = exact<uint64_t>(n_contigs);
        uint64_t* ref_end = exact<uint64_t>(n_contigs);
        uint64_t* chunk_first = exact<uint64_t>(n_contigs);
        uint64_t* chunk_end = exact<uint64_t>(n_contigs);
        for (uint64_t r = 0; r < n_contigs; r++) ref_first[r] = ref_end[r] = chunk_first[r] = chunk_end[r] = 0;
        uint8_t* head = exact<uint8_t>(m);
        uint64_t* unmapped_before = exact<uint64_t>(m + 1);
        uint64_t* end_max = exact<uint64_t>(m);
        uint64_t n_indexed = 0, n_chunks = 0, run = 0;
        unmapped_before[0] = 0;
        for (uint64_t j = 0; j < m; j++) {
            const bai_rec_t& e = rec[j];
            if (j && bai_before(e, rec[j - 1])) report(e.slot, BAI_INVALID);
            const bool placed = e.ref >= 0, last = j + 1 == m;
            const bool ref_head = placed && (j == 0 || rec[j - 1].ref != e.ref);
            if (ref_head) ref_first[e.ref] = j;
            if (placed && (last || rec[j + 1].ref != e.ref)) ref_end[e.ref] = j + 1;
            if (placed && (last || rec[j + 1].ref < 0)) n_indexed = j + 1;
            head[j] = ref_head || (placed && ((rec[j - 1].binf ^ e.binf) & 0xFFFFu));
            n_chunks += head[j];
            unmapped_before[j + 1] = unmapped_before[j] + (placed && (e.binf & BAI_UNMAPPED_BIT) ? 1 : 0);
            run = std::max(run, bai_end_key(e));
            end_max[j] = run;
        }
        int64_t status = 0;
        uint64_t first_bad = BAI_NONE, bytes = 0;
        uint8_t* out = nullptr;
        if (bad != BAI_NONE) {
            status = (int64_t)(bad & 3);
            first_bad = bad >> 2;
        } else {
            // 3. the chunk list, sorted stably by (ref, bin); bins; the references' bytes
            uint64_t* key = exact<uint64_t>(n_chunks);
            uint64_t* head_pos = exact<uint64_t>(n_chunks + 1);
            uint64_t* perm = exact<uint64_t>(n_chunks);
            for (uint64_t j = 0, c = 0; j < m; j++)
                if (head[j]) {
                    key[c] = bai_chunk_key(rec[j].ref, rec[j].binf);
                    if (key[c] >= BAI_KEY_PAD) return 4;
                    head_pos[c] = j;
                    perm[c] = c;
                    c++;
                }
            head_pos[n_chunks] = n_indexed;
            std::stable_sort(perm, perm + n_chunks, [&](uint64_t a, uint64_t b) { return key[a] < key[b]; });
            uint64_t* bins_before = exact<uint64_t>(n_chunks + 1);
            uint8_t* bin_head = exact<uint8_t>(n_chunks);
            uint64_t n_bins = 0;
            for (uint64_t k = 0; k < n_chunks; k++) {
                const uint64_t kk = key[perm[k]], ref = kk >> 16;
                bin_head[k] = k == 0 || key[perm[k - 1]] != kk;
                if (k == 0 || key[perm[k - 1]] >> 16 != ref) chunk_first[ref] = k;
                if (k + 1 == n_chunks || key[perm[k + 1]] >> 16 != ref) chunk_end[ref] = k + 1;
                bins_before[k] = n_bins;
                n_bins += bin_head[k];
            }
            bins_before[n_chunks] = n_bins;
            uint64_t* bin_start = exact<uint64_t>(n_bins + 1);
            for (uint64_t k = 0; k < n_chunks; k++)
                if (bin_head[k]) bin_start[bins_before[k]] = k;
            bin_start[n_bins] = n_chunks;
            uint64_t* ref_base = exact<uint64_t>(n_contigs + 1);
            struct Ref {
                uint64_t n_bins, n_chunks, n_intv;
            };
            auto ref_of = [&](uint64_t r) {
                Ref x = {0, 0, 0};
                if (ref_end[r] <= ref_first[r]) return x;
                x.n_chunks = chunk_end[r] - chunk_first[r];
                x.n_bins = bins_before[chunk_end[r]] - bins_before[chunk_first[r]];
                x.n_intv = bai_n_intv((uint32_t)end_max[ref_end[r] - 1]);
                return x;
            };
            ref_base[0] = 0;
            for (uint64_t r = 0; r < n_contigs; r++) {
                const Ref x = ref_of(r);
                ref_base[r + 1] = ref_base[r] + bai_ref_bytes(ref_end[r] > ref_first[r], x.n_bins, x.n_chunks, x.n_intv);
            }
            bytes = bai_total(ref_base[n_contigs]);
            // 4. the bytes, into an allocation of exactly that size
            out = at_residue(bytes, (res + 6) % 16);
            memset(out, 0xA5, bytes);
            bai_put_head(out, n_contigs);
            bai_put64(out + 8 + ref_base[n_contigs], m - n_indexed);
            for (uint64_t k = 0; k < n_chunks; k++) {
                const uint64_t c = perm[k], j0 = head_pos[c], j1 = head_pos[c + 1], kk = key[c], ref = kk >> 16;
                const uint64_t b = bins_before[k] + bin_head[k] - 1, at = bin_start[b], first = chunk_first[ref];
                uint8_t* bin = out + 8 + ref_base[ref] + bai_bin_at(b - bins_before[first], at - first);
                if (bin_head[k]) bai_put_bin(bin, (uint32_t)(kk & 0xFFFFu), bin_start[b + 1] - at);
                bai_put_chunk(bin + 8 + 16 * (k - at), bai_voff(off[rec[j0].slot], block_off, base), bai_voff(off[rec[j1 - 1].slot + 1], block_off, base));
            }
            for (uint64_t r = 0; r < n_contigs; r++) {
                uint8_t* ref = out + 8 + ref_base[r];
                if (ref_end[r] <= ref_first[r]) {
                    bai_put_empty_ref(ref);
                    continue;
                }
                const Ref x = ref_of(r);
                const uint64_t unmapped = unmapped_before[ref_end[r]] - unmapped_before[ref_first[r]];
                bai_put32(ref, (uint32_t)(x.n_bins + 1));
                bai_put_pseudo(ref + bai_pseudo_at(x.n_bins, x.n_chunks), bai_voff(off[rec[ref_first[r]].slot], block_off, base),
                               bai_voff(off[rec[ref_end[r] - 1].slot + 1], block_off, base), ref_end[r] - ref_first[r] - unmapped, unmapped, x.n_intv);
                uint8_t* intv = ref + bai_intv_at(x.n_bins, x.n_chunks) + 4;
                for (uint64_t w = 0; w < x.n_intv; w++)
                    bai_put64(intv + 8 * w, bai_voff(off[rec[bai_window_first(end_max, ref_first[r], ref_end[r], (uint32_t)r, w)].slot], block_off, base));
            }
            free(key);
            free(head_pos);
            free(perm);
            free(bins_before);
            free(bin_head);
            free(bin_start);
            free(ref_base);
        }
        fwrite(&status, 8, 1, o);
        fwrite(&first_bad, 8, 1, o);
        fwrite(&bytes, 8, 1, o);
        if (bytes) fwrite(out, 1, bytes, o);
        if (out) free(out - (res + 6) % 16);
        free(recs - res);
        free(rec);
        free(ref_first);
        free(ref_end);
        free(chunk_first);
        free(chunk_end);
        free(head);
        free(unmapped_before);
        free(end_max);
        free(hc);
        free(contigs);
        free(hs);
        free(off);
        free(ht);
        free(table);
        free(tail);
    }
    free(n_cases);
    fclose(o);
    fclose(f);
    return 0;
}
