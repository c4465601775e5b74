// Stand-alone CPU program for tests/test_vcf_host_bodies.py: the __host__ __device__ bodies of csrc/vcf_rule.h run on the host, in
// the steps the kernels of csrc/vcf_emit.hip take for bg_vcf_emit_dev.  Pass 1, an element at a time from the last to the
// first (nothing may depend on the order): vcf_site_ok / vcf_event_ok, the smallest refused index, the SNV flag, the line's
// length by vcf_line_of.  The sites compacted by a prefix sum of the flags; pass 2: vcf_events_before / vcf_sites_upto give
// every line its slot; a prefix sum of the slots' lengths gives the offsets.  Pass 3: every line by vcf_put_lane for lanes
// G - 1 .. 0 of G = 8 — a line of at most 256 bytes into a stage of exactly its length and from there into the output, a
// longer one straight into the output.  Stage and output start as zeros and no byte of a line is 0, so a byte that no lane
// wrote is seen as well as one written outside.
// The first test builds it with -fsanitize=address,undefined.  Every list, table, name buffer, text, scratch array, stage and
// output is a heap allocation of exactly its size, so a body that reads or writes one byte outside stops the program.
// With no arguments it checks vcf_ndig and vcf_put_dec at every power of ten up to 2^64 - 1 (one below, at, one above)
// against snprintf, and the two byte tables against their definition.
// Input: uint64 cases; per case uint64 n_sites, n_events, n_seq, n_contigs, name_bytes, n_text; the sites; the events; the
// inserted bases; the contigs; the names; the text.
// Output per case: int64 rc, uint64 first_bad, n_lines, out_bytes; if rc == 0 the text and n_lines + 1 offsets.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rust-bio_amd/csrc/vcf_rule.h"

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
static const uint32_t G = 8, STAGE = 256;

static int numbers() {
    std::vector<uint64_t> v = {0, 1, 9, 0xFFFFFFFFull, 0x100000000ull, 0x1FFFFFFFEull, ~0ull};
    uint64_t p = 1;
    for (int k = 0; k < 20; k++) {  // 10^0 .. 10^19
        v.push_back(p - 1);
        v.push_back(p);
        v.push_back(p + 1);
        if (k < 19) p *= 10;
    }
    for (uint64_t x : v) {
        char want[32];
        const int n = snprintf(want, sizeof want, "%llu", (unsigned long long)x);
        if ((int)vcf_ndig(x) != n) return 3;
        char* got = (char*)malloc(n);  // exactly its digits
        vcf_put_dec(got, x, (uint32_t)n);
        const bool same = memcmp(got, want, n) == 0;
        free(got);
        if (!same) return 4;
    }
    for (int b = 0; b < 256; b++) {
        const int u = b >= 'a' && b <= 'z' ? b - 32 : b;
        const char* at = u ? strchr("ACGTN", u) : nullptr;
        const int want = at ? u : u && strchr("MRWDHV", u) ? 'A' : u && strchr("YSB", u) ? 'C' : u == 'K' ? 'G' : 'N';
        if (vcf_ref_byte((uint8_t)b) != want) return 5;
        if (vcf_ins_byte((uint8_t)b) != (b && strchr("ACGT", b) ? b : 'N')) return 6;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 1) return numbers();
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint64_t* n_cases = load<uint64_t>(f, 1);
    uint8_t* fold = make<uint8_t>(256);
    for (int b = 0; b < 256; b++) fold[b] = vcf_ref_byte((uint8_t)b);
    for (uint64_t c = 0; c < *n_cases; c++) {
        uint64_t* hd = load<uint64_t>(f, 6);
        vcf_args_t a = {};
        a.n_sites = hd[0], a.n_events = hd[1], a.n_seq = hd[2], a.n_contigs = hd[3], a.n_text = hd[5];
        a.sites = load<bg_bam_site_t>(f, a.n_sites);
        a.events = load<bg_bam_indel_t>(f, a.n_events);
        a.seq = load<uint8_t>(f, a.n_seq);
        a.contigs = load<bg_sam_contig_t>(f, a.n_contigs);
        a.names = load<char>(f, hd[4]);
        a.text = load<uint8_t>(f, a.n_text);
        const uint64_t n = a.n_sites + a.n_events;

        // ---- pass 1
        uint64_t bad = VCF_NONE;
        bool too_large = false;
        uint32_t* snv = make<uint32_t>(a.n_sites);
        uint32_t* elem_len = make<uint32_t>(n);
        for (uint64_t e = n; e-- > 0;) {
            const bool site = e < a.n_sites;
            const bool ok = site ? vcf_site_ok(a, e) : vcf_event_ok(a, e - a.n_sites);
            const bool line = ok && (!site || a.sites[e].kind == BG_SITE_SNV);
            uint64_t len = line ? vcf_line_of(a, e).len : 0;
            if (!ok && e < bad) bad = e;
            if (len >> 32) too_large = true, len = 0;
            if (site) snv[e] = line;
            elem_len[e] = (uint32_t)len;
        }
        // ---- pass 2 (run whatever pass 1 found, as the kernels run before the one read-back)
        uint64_t* snv_off = make<uint64_t>(a.n_sites + 1);
        for (uint64_t i = 0; i < a.n_sites; i++) snv_off[i + 1] = snv_off[i] + snv[i];
        uint32_t* line_len = make<uint32_t>(n);
        uint32_t* line_src = make<uint32_t>(n);
        for (uint64_t e = n; e-- > 0;) {
            uint64_t slot;
            if (e < a.n_sites) {
                if (!snv[e]) continue;
                slot = snv_off[e] + vcf_events_before(a.events, a.n_events, a.sites[e].region, a.sites[e].pos);
            } else {
                const bg_bam_indel_t& v = a.events[e - a.n_sites];
                slot = (e - a.n_sites) + snv_off[vcf_sites_upto(a.sites, a.n_sites, v.region, v.pos)];
            }
            line_len[slot] = elem_len[e];
            line_src[slot] = (uint32_t)e;
        }
        uint64_t* off = make<uint64_t>(n + 1);
        for (uint64_t l = 0; l < n; l++) off[l + 1] = off[l] + line_len[l];
        const uint64_t n_lines = snv_off[a.n_sites] + a.n_events, out_bytes = off[n];

        int64_t rc = bad != VCF_NONE ? BG_ERR_INVALID_ARG : too_large ? BG_ERR_TOO_LARGE : BG_OK;
        uint64_t head[3] = {bad, rc ? 0 : n_lines, rc ? 0 : out_bytes};
        fwrite(&rc, 8, 1, o);
        fwrite(head, 8, 3, o);
        if (rc == BG_OK) {
            // ---- pass 3
            char* out = make<char>(out_bytes);
            for (uint64_t l = 0; l < n_lines; l++) {
                const vcf_line_t L = vcf_line_of(a, line_src[l]);
                if (L.len != off[l + 1] - off[l]) return 7;
                const bool staged = L.len <= STAGE;
                char* dst = staged ? make<char>(L.len) : out + off[l];
                for (uint32_t lane = G; lane-- > 0;) vcf_put_lane(a, L, fold, dst, lane, G);
                if (staged) {
                    memcpy(out + off[l], dst, L.len);
                    free(dst);
                }
            }
            for (uint64_t i = 0; i < out_bytes; i++)
                if (!out[i]) return 8;  // a byte no lane wrote
            fwrite(out, 1, out_bytes, o);
            fwrite(off, 8, n_lines + 1, o);
            free(out);
        }
        free(hd), free((void*)a.sites), free((void*)a.events), free((void*)a.seq), free((void*)a.contigs), free((void*)a.names), free((void*)a.text);
        free(snv), free(elem_len), free(snv_off), free(line_len), free(line_src), free(off);
    }
    free(fold);
    free(n_cases);
    fclose(f);
    fclose(o);
    return 0;
}
