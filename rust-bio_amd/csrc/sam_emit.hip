// SAM records from seed-and-extend hits (bg_sam_emit[_dup]_batch[_dev], bg_sam_header[_so]): the record is defined in include/biogpu.h;
// whether a slot is placed and whether it writes a line are decided in sam_rule.h, which the duplicate marker and the sort keys
// (sam_sort.hip) share.
// Two passes over the hit slots.  The length pass (one lane per slot) decides what each line holds, walks the slot's
// operations for the CIGAR, NM and MD lengths and writes the line length; a scan turns the lengths into offsets.  The write
// pass gives every line a fixed group of 16 or 32 lanes: the group stages the line in LDS at the same offset inside a 16-byte
// granule that it has in the output buffer, so that everything but the line's unaligned head and tail leaves with 16-byte
// stores.  A line that is longer than the staging area (reads go up to 65 535 bases) is formatted by the same code straight
// into global memory.  The group leaves the CIGAR and MD strings blank: walking a slot's operations is serial, and with one
// walking lane per group a wavefront spent its time there (measured: 20.8 ms of a 22.6 ms call for 1.25 M lines, against
// 1.8 ms for the whole length pass, which does the same two walks with every lane busy).  So a third kernel, one lane per
// slot like the length pass, writes the two strings into the finished lines.  All passes derive the line from one function
// (sam_line), so they cannot disagree about a length.
#include <algorithm>

#include "dna_complement.h"
#include "fastq_cols.h"
#include "fm_kernels.h"
#include "sam_rule.h"

namespace {

constexpr uint32_t kStage = 1024;             // bytes of a staged line
constexpr uint32_t kStageBuf = kStage + 16;   // ... plus its offset inside the 16-byte granule of the output

struct SamArgs {
    uint64_t n_slots;
    uint32_t K, flags;
    const bg_sam_contig_t* contigs;
    uint64_t n_contigs;
    const char* names;
    const uint8_t* fq;
    const bg_fastq_record_t* recs;
    const uint8_t* seq;
    const uint8_t* qual;
    const bg_seed_hit_t* hits;
    const uint8_t* strand;
    const uint8_t* ops;
    const bg_multi_hit_t* multi;
    const bg_pair_hit_t* pairs;
    const uint8_t* text;
    uint64_t n_text;
    const uint8_t* dup;  // optional: read r's placed lines carry 0x400 where dup[r] != 0
};

struct SamDesc {  // what the length pass learned from a slot's operations, and where the two strings go in the line
    uint32_t cigar_len, md_len, nm;
    uint32_t cigar_at, md_at;  // 0: no such string (a line never starts with either)
    uint32_t reserved;
};

__device__ __forceinline__ uint32_t ndig(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10) {
        v /= 10;
        n++;
    }
    return n;
}
__device__ __forceinline__ uint32_t ndig_signed(int64_t v) { return v < 0 ? 1 + ndig((uint64_t)(-v)) : ndig((uint64_t)v); }
// v in n = ndig(v) decimal digits
__device__ __forceinline__ void put_dec(char* d, uint64_t v, uint32_t n) {
    for (uint32_t i = n; i-- > 0;) {
        d[i] = (char)('0' + v % 10);
        v /= 10;
    }
}
__device__ __forceinline__ uint32_t put_signed(char* d, int64_t v) {
    uint32_t w = 0;
    if (v < 0) d[w++] = '-';
    const uint64_t m = v < 0 ? (uint64_t)(-v) : (uint64_t)v;
    const uint32_t n = ndig(m);
    put_dec(d + w, m, n);
    return w + n;
}

// the contig a slot is placed on, -1 if it is not placed (the rule: sam_rule.h)
__device__ __forceinline__ int64_t sam_place(const SamArgs& a, uint64_t slot) {
    return sam_rule_place(a.contigs, a.n_contigs, a.hits[slot], a.strand[slot]);
}

struct SamLine {
    bool writes, placed, rev, seq_star, qual_star, has_xs;
    uint32_t flag, mapq, qname_len, seq_len;
    int64_t contig;  // RNAME: a contig, or -1 for "*"
    int64_t next;    // RNEXT: a contig, -1 for "*", -2 for "="
    uint64_t pos, pnext;
    int64_t tlen;
    int32_t score, xs;
};

// every field of a slot's line but the three that need the operations
__device__ SamLine sam_line(const SamArgs& a, uint64_t slot) {
    SamLine L = {};
    const uint64_t r = slot / a.K;
    const uint32_t k = (uint32_t)(slot - r * a.K);
    const int64_t own = sam_place(a, slot);
    L.placed = own >= 0;
    L.writes = sam_rule_writes(a.flags, k, L.placed, k == 0 ? L.placed : sam_place(a, r * a.K) >= 0);
    if (!L.writes) return L;
    const bg_seed_hit_t& h = a.hits[slot];
    const bg_fastq_record_t& rec = a.recs[r];
    L.rev = L.placed && a.strand[slot] == BG_HIT_REVERSE;
    L.flag = (L.placed ? 0u : 0x4u) | (L.rev ? 0x10u : 0u) | (k ? 0x100u : 0u) | (a.dup && L.placed && a.dup[r] ? 0x400u : 0u);
    L.contig = own;
    L.pos = L.placed ? h.ref_start - a.contigs[own].start + 1 : 0;
    L.next = -1;
    L.qname_len = rec.id_len;
    if (a.flags & BG_SAM_PAIRED) {  // K == 1: the mate's slot is the neighbouring read's
        const uint64_t m = slot ^ 1;
        const int64_t mate = sam_place(a, m);
        const bg_seed_hit_t& hm = a.hits[m];
        const bool first = !(r & 1);
        L.flag |= 0x1u | (first ? 0x40u : 0x80u) | (mate < 0 ? 0x8u : 0u) | (mate >= 0 && a.strand[m] == BG_HIT_REVERSE ? 0x20u : 0u);
        const uint64_t mpos = mate >= 0 ? hm.ref_start - a.contigs[mate].start + 1 : 0;
        if (L.placed && own == mate) {
            if (a.pairs[r >> 1].proper) L.flag |= 0x2u;
            const uint64_t span = max(h.ref_end, hm.ref_end) - min(h.ref_start, hm.ref_start);
            const bool left = h.ref_start < hm.ref_start || (h.ref_start == hm.ref_start && first);
            L.tlen = left ? (int64_t)span : -(int64_t)span;
        }
        if (!L.placed && mate >= 0) {
            L.contig = mate;
            L.pos = mpos;
        }
        if (L.placed || mate >= 0) {
            const int64_t mate_rname = mate >= 0 ? mate : own;  // the mate's RNAME and POS fields, borrowed ones included
            L.next = mate_rname == L.contig ? -2 : mate_rname;
            L.pnext = mate >= 0 ? mpos : L.pos;
        }
        if (rec.id_len > 2) {
            const uint8_t* q = a.fq + rec.id_off + rec.id_len - 2;
            if (q[0] == '/' && q[1] == (first ? '1' : '2')) L.qname_len -= 2;
        }
    }
    L.mapq = !L.placed || k ? 0u : (a.multi ? a.multi[r].mapq : 255u);
    L.seq_len = rec.seq_len;
    L.seq_star = k > 0 || rec.seq_len == 0;
    L.qual_star = k > 0 || rec.qual_len == 0 || rec.qual_len != rec.seq_len;
    L.score = h.aln.score;
    L.has_xs = L.placed && a.multi && k == 0 && a.multi[r].sub_score != BG_MIN_SCORE;
    L.xs = L.has_xs ? a.multi[r].sub_score : 0;
    return L;
}

// The CIGAR of cigar_kernel (align_text.hip) with soft clips; o == nullptr: only its length.
__device__ uint32_t sam_cigar(const bg_alignment_t& al, const uint8_t* __restrict__ q, char* o) {
    if (!al.n_ops) return 0;
    uint32_t w = 0;
    auto emit = [&](uint32_t n, char c) {
        const uint32_t d = ndig(n);
        if (o) {
            put_dec(o + w, n, d);
            o[w + d] = c;
        }
        w += d + 1;
    };
    auto add = [&](uint32_t kind, uint32_t n) {
        if (kind <= BG_OP_INS) emit(n, kind == BG_OP_MATCH ? '=' : kind == BG_OP_SUBST ? 'X' : kind == BG_OP_DEL ? 'D' : 'I');
    };
    if (al.xstart > 0) emit(al.xstart, 'S');
    uint32_t last = q[0], run = 1;
    for (uint32_t i = 1; i < al.n_ops; i++) {
        const uint32_t op = q[i];
        if (op == last) {
            run++;
        } else {
            add(last, run);
            run = 1;
        }
        last = op;
    }
    add(last, run);
    if (al.xlen > al.xend) emit(al.xlen - al.xend, 'S');
    return w;
}

// The MD string and NM of a hit (rule in include/biogpu.h); o == nullptr: only the length (the text is not read then).
__device__ uint32_t sam_md(const SamArgs& a, const bg_seed_hit_t& h, const uint8_t* __restrict__ q, char* o, uint32_t* nm) {
    uint32_t w = 0, c = 0, n = 0;
    uint64_t t = h.ref_start;
    bool in_del = false;
    auto count = [&]() {
        const uint32_t d = ndig(c);
        if (o) put_dec(o + w, c, d);
        w += d;
        c = 0;
    };
    auto ref = [&]() {
        if (o) o[w] = t < a.n_text ? (char)a.text[t] : '?';
        w++;
        t++;
    };
    for (uint32_t i = 0; i < h.aln.n_ops; i++) {
        const uint32_t op = q[i];
        if (op == BG_OP_DEL) {
            if (!in_del) {
                count();
                if (o) o[w] = '^';
                w++;
            }
            ref();
            n++;
        } else if (op == BG_OP_MATCH) {
            c++;
            t++;
        } else if (op == BG_OP_SUBST) {
            count();
            ref();
            n++;
        } else if (op == BG_OP_INS) {
            n++;
        }
        in_del = op == BG_OP_DEL;
    }
    count();
    *nm = n;
    return w;
}

// where the fields of a line start; [11] is the first byte of the tags (or the final newline), len the whole line
struct SamLayout {
    uint32_t at[12];
    uint32_t len;
};
__device__ SamLayout sam_layout(const SamArgs& a, const SamLine& L, const SamDesc& d) {
    SamLayout y;
    uint32_t w = 0;
    auto field = [&](int i, uint32_t n) {
        y.at[i] = w;
        w += n + 1;  // and its TAB (the newline behind QUAL when there are no tags)
    };
    field(0, L.qname_len ? L.qname_len : 1);
    field(1, ndig(L.flag));
    field(2, L.contig >= 0 ? a.contigs[L.contig].name_len : 1);
    field(3, ndig(L.pos));
    field(4, ndig(L.mapq));
    field(5, L.placed && d.cigar_len ? d.cigar_len : 1);
    field(6, L.next >= 0 ? a.contigs[L.next].name_len : 1);
    field(7, ndig(L.pnext));
    field(8, ndig_signed(L.tlen));
    field(9, L.seq_star ? 1 : L.seq_len);
    field(10, L.qual_star ? 1 : L.seq_len);
    y.at[11] = w - 1;
    if (L.placed) {
        w += 5 + ndig_signed(L.score) + 1;
        if (L.has_xs) w += 5 + ndig_signed(L.xs) + 1;
        if (a.flags & BG_SAM_TAG_NM) w += 5 + ndig(d.nm) + 1;
        if (a.flags & BG_SAM_TAG_MD) w += 5 + d.md_len + 1;
    }
    y.len = w;
    return y;
}

// length pass: one lane per slot
__global__ __launch_bounds__(256) void sam_length_kernel(const SamArgs a, uint32_t* __restrict__ len, SamDesc* __restrict__ desc) {
    const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= a.n_slots) return;
    const SamLine L = sam_line(a, slot);
    SamDesc d = {};
    if (!L.writes) {
        len[slot] = 0;
        desc[slot] = d;
        return;
    }
    if (L.placed) {
        const bg_seed_hit_t& h = a.hits[slot];
        const uint8_t* q = a.ops + h.aln.ops_off;
        d.cigar_len = sam_cigar(h.aln, q, nullptr);
        if (a.flags & (BG_SAM_TAG_NM | BG_SAM_TAG_MD)) d.md_len = sam_md(a, h, q, nullptr, &d.nm);
    }
    const SamLayout y = sam_layout(a, L, d);
    if (L.placed && d.cigar_len) d.cigar_at = y.at[5];
    if (L.placed && (a.flags & BG_SAM_TAG_MD)) d.md_at = y.len - 1 - d.md_len;  // the last tag: the newline follows it
    len[slot] = y.len;
    desc[slot] = d;
}

// third pass: one lane per slot writes the CIGAR and MD strings into the line the write pass left
__global__ __launch_bounds__(256) void sam_ops_kernel(const SamArgs a, const SamDesc* __restrict__ desc, const uint64_t* __restrict__ off,
                                                      char* __restrict__ out) {
    const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= a.n_slots) return;
    const SamDesc d = desc[slot];
    if (!d.cigar_at && !d.md_at) return;
    const bg_seed_hit_t& h = a.hits[slot];
    const uint8_t* q = a.ops + h.aln.ops_off;
    char* line = out + off[slot];
    if (d.cigar_at) sam_cigar(h.aln, q, line + d.cigar_at);
    if (d.md_at) {
        uint32_t nm;
        sam_md(a, h, q, line + d.md_at, &nm);
    }
}

// One line by the G lanes of its group into dst (LDS or global memory): lane 0 the short fields, lane 1 the tags, all of them
// the names, SEQ and QUAL; the CIGAR and MD strings stay blank for sam_ops_kernel.
template <int G>
__device__ void sam_format(const SamArgs& a, uint64_t slot, const SamDesc& d, char* dst, uint32_t lane, const uint8_t* s_comp) {
    const SamLine L = sam_line(a, slot);
    const SamLayout y = sam_layout(a, L, d);
    const uint64_t r = slot / a.K;
    const bg_fastq_record_t& rec = a.recs[r];
    auto copy = [&](uint32_t at, const void* src, uint32_t n) {
        for (uint32_t i = lane; i < n; i += G) dst[at + i] = ((const char*)src)[i];
    };
    auto name = [&](uint32_t at, int64_t contig) {
        if (contig >= 0) copy(at, a.names + a.contigs[contig].name_off, a.contigs[contig].name_len);
        else if (lane == 0) dst[at] = contig == -2 ? '=' : '*';
    };
    if (L.qname_len) copy(y.at[0], a.fq + rec.id_off, L.qname_len);
    name(y.at[2], L.contig);
    name(y.at[6], L.next);
    if (!L.seq_star) {
        const uint8_t* s = a.seq + rec.seq_off;
        const uint32_t n = L.seq_len;
        if (L.rev)
            for (uint32_t i = lane; i < n; i += G) dst[y.at[9] + i] = (char)s_comp[s[n - 1 - i]];
        else
            copy(y.at[9], s, n);
    }
    if (!L.qual_star) {
        const uint8_t* s = a.qual + rec.qual_off;
        const uint32_t n = L.seq_len;
        if (L.rev)
            for (uint32_t i = lane; i < n; i += G) dst[y.at[10] + i] = (char)s[n - 1 - i];
        else
            copy(y.at[10], s, n);
    }
    if (lane == 0) {
        if (!L.qname_len) dst[y.at[0]] = '*';
        put_dec(dst + y.at[1], L.flag, ndig(L.flag));
        put_dec(dst + y.at[3], L.pos, ndig(L.pos));
        put_dec(dst + y.at[4], L.mapq, ndig(L.mapq));
        if (!d.cigar_at) dst[y.at[5]] = '*';
        put_dec(dst + y.at[7], L.pnext, ndig(L.pnext));
        put_signed(dst + y.at[8], L.tlen);
        if (L.seq_star) dst[y.at[9]] = '*';
        if (L.qual_star) dst[y.at[10]] = '*';
        for (int i = 1; i < 11; i++) dst[y.at[i] - 1] = '\t';
        dst[y.len - 1] = '\n';
    }
    if (lane == 1 && L.placed) {
        uint32_t w = y.at[11];
        auto tag = [&](char c0, char c1, char type) {
            dst[w] = '\t';
            dst[w + 1] = c0;
            dst[w + 2] = c1;
            dst[w + 3] = ':';
            dst[w + 4] = type;
            dst[w + 5] = ':';
            w += 6;
        };
        tag('A', 'S', 'i');
        w += put_signed(dst + w, L.score);
        if (L.has_xs) {
            tag('X', 'S', 'i');
            w += put_signed(dst + w, L.xs);
        }
        if (a.flags & BG_SAM_TAG_NM) {
            tag('N', 'M', 'i');
            w += put_signed(dst + w, d.nm);
        }
        if (a.flags & BG_SAM_TAG_MD) tag('M', 'D', 'Z');
    }
}

// write pass: G lanes per slot, 256 / G slots per block
template <int G>
__global__ __launch_bounds__(256) void sam_write_kernel(const SamArgs a, const SamDesc* __restrict__ desc, const uint64_t* __restrict__ off,
                                                        char* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) char s_stage[(256 / G) * kStageBuf];
    __shared__ __attribute__((aligned(4))) uint8_t s_comp[256];
    load_complement(s_comp);
    const uint32_t g = threadIdx.x / G, lane = threadIdx.x % G;
    const uint64_t slot = (uint64_t)blockIdx.x * (256 / G) + g;
    uint64_t o0 = 0;
    uint32_t len = 0;
    if (slot < a.n_slots) {
        o0 = off[slot];
        len = (uint32_t)(off[slot + 1] - o0);
    }
    char* line = out + o0;
    const uint32_t mis = (uint32_t)((uintptr_t)line & 15);
    const bool staged = len && mis + len <= kStageBuf;
    char* stage = s_stage + g * kStageBuf + mis;
    if (len) sam_format<G>(a, slot, desc[slot], staged ? stage : line, lane, s_comp);
    __syncthreads();
    if (!staged) return;
    // head up to the first 16-byte boundary and tail behind the last one byte by byte, everything between as 16-byte stores
    const uint32_t head = min(len, (16 - mis) & 15);
    const uint32_t body = (len - head) >> 4, tail = (len - head) & 15;
    if (lane < head) line[lane] = stage[lane];
    for (uint32_t i = lane; i < body; i += G) *(uint4*)(line + head + 16 * i) = *(const uint4*)(stage + head + 16 * i);
    if (lane < tail) line[head + 16 * body + lane] = stage[head + 16 * body + lane];
}

int sam_check(const bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, uint64_t n_contigs, const void* pairs) {
    if (!fm || !sp) return BG_ERR_INVALID_ARG;
    if (sp->flags & ~(uint32_t)(BG_SAM_PAIRED | BG_SAM_SECONDARY | BG_SAM_TAG_NM | BG_SAM_TAG_MD)) return BG_ERR_INVALID_ARG;
    if (sp->max_hits == 0 || sp->max_hits > BG_SEED_MAX_HITS || n_contigs == 0) return BG_ERR_INVALID_ARG;
    if ((sp->flags & BG_SAM_PAIRED) && ((n_reads & 1) || sp->max_hits != 1 || !pairs)) return BG_ERR_INVALID_ARG;
    if ((sp->flags & BG_SAM_TAG_MD) && !fm->d_text) return BG_ERR_INVALID_ARG;
    return BG_OK;
}

}  // namespace

extern "C" int bg_sam_header_so(const bg_sam_contig_t* contigs, uint64_t n_contigs, const char* names, int sort_order, char* out,
                                uint64_t out_cap, uint64_t* out_bytes) {
    if (!out_bytes || (n_contigs && (!contigs || !names)) || (!out && out_cap)) return BG_ERR_INVALID_ARG;
    if (sort_order != BG_SAM_SO_UNSORTED && sort_order != BG_SAM_SO_COORDINATE) return BG_ERR_INVALID_ARG;
    std::string s = sort_order == BG_SAM_SO_COORDINATE ? "@HD\tVN:1.6\tSO:coordinate\n" : "@HD\tVN:1.6\tSO:unsorted\n";
    for (uint64_t c = 0; c < n_contigs; c++) {
        s += "@SQ\tSN:";
        s.append(names + contigs[c].name_off, contigs[c].name_len);
        s += "\tLN:" + std::to_string(contigs[c].len) + "\n";
    }
    s += "@PG\tID:biogpu\tPN:biogpu\n";
    *out_bytes = s.size();
    if (!out) return BG_OK;
    if (s.size() > out_cap) return BG_ERR_OPS_CAP;
    memcpy(out, s.data(), s.size());
    return BG_OK;
}

extern "C" int bg_sam_header(const bg_sam_contig_t* contigs, uint64_t n_contigs, const char* names, char* out, uint64_t out_cap,
                             uint64_t* out_bytes) {
    return bg_sam_header_so(contigs, n_contigs, names, BG_SAM_SO_UNSORTED, out, out_cap, out_bytes);
}

extern "C" int bg_sam_emit_dup_batch_dev(bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* d_contigs,
                                         uint64_t n_contigs, const char* d_names, const uint8_t* d_fastq_text, const bg_fastq_record_t* d_recs,
                                         const uint8_t* d_seq, const uint8_t* d_qual, const bg_seed_hit_t* d_hits, const uint8_t* d_strand,
                                         const uint8_t* d_ops, const bg_multi_hit_t* d_multi, const bg_pair_hit_t* d_pairs, const uint8_t* d_dup,
                                         char* d_out, uint64_t out_cap, uint64_t* d_out_off, uint64_t* out_bytes, void* stream) {
    if (!d_out_off || !out_bytes) return BG_ERR_INVALID_ARG;
    *out_bytes = 0;
    int rc = sam_check(fm, sp, n_reads, n_contigs, d_pairs);
    if (rc) return rc;
    if (!d_out && out_cap) return BG_ERR_INVALID_ARG;
    if (n_reads && (!d_contigs || !d_names || !d_fastq_text || !d_recs || !d_seq || !d_qual || !d_hits || !d_strand || !d_ops))
        return BG_ERR_INVALID_ARG;
    bg_ctx* ctx = fm->ctx;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    if (n_reads == 0) {
        const uint64_t z = 0;
        BG_HIP(hipMemcpyAsync(d_out_off, &z, 8, hipMemcpyHostToDevice, st));
        BG_HIP(hipStreamSynchronize(st));
        return BG_OK;
    }
    bg_scratch_guard guard(ctx, st);
    const uint64_t n_slots = n_reads * sp->max_hits;
    uint32_t* d_len;
    SamDesc* d_desc;
    uint64_t* d_sums;
    if ((rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_len = cv.take<uint32_t>(n_slots);
        d_desc = cv.take<SamDesc>(n_slots);
        d_sums = cv.take<uint64_t>(bg_scan_sums_words(n_slots));
    }))) return rc;
    const SamArgs a = {n_slots, sp->max_hits, sp->flags, d_contigs, n_contigs, d_names, d_fastq_text, d_recs, d_seq, d_qual, d_hits,
                       d_strand, d_ops, d_multi, (sp->flags & BG_SAM_PAIRED) ? d_pairs : nullptr, (const uint8_t*)fm->d_text, fm->n_text, d_dup};
    sam_length_kernel<<<dim3((uint32_t)((n_slots + 255) / 256)), dim3(256), 0, st>>>(a, d_len, d_desc);
    BG_HIP(hipGetLastError());
    if ((rc = bg_scan_u32(d_len, n_slots, d_out_off, d_sums, st))) return rc;
    uint64_t total = 0;
    BG_HIP(hipMemcpyAsync(&total, d_out_off + n_slots, 8, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    *out_bytes = total;
    if (!d_out) return BG_OK;
    if (total > out_cap) return BG_ERR_OPS_CAP;
    if (ctx->sam_lanes == 32)
        sam_write_kernel<32><<<dim3((uint32_t)((n_slots + 7) / 8)), dim3(256), 0, st>>>(a, d_desc, d_out_off, d_out);
    else
        sam_write_kernel<16><<<dim3((uint32_t)((n_slots + 15) / 16)), dim3(256), 0, st>>>(a, d_desc, d_out_off, d_out);
    sam_ops_kernel<<<dim3((uint32_t)((n_slots + 255) / 256)), dim3(256), 0, st>>>(a, d_desc, d_out_off, d_out);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

extern "C" int bg_sam_emit_batch_dev(bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* d_contigs,
                                     uint64_t n_contigs, const char* d_names, const uint8_t* d_fastq_text, const bg_fastq_record_t* d_recs,
                                     const uint8_t* d_seq, const uint8_t* d_qual, const bg_seed_hit_t* d_hits, const uint8_t* d_strand,
                                     const uint8_t* d_ops, const bg_multi_hit_t* d_multi, const bg_pair_hit_t* d_pairs, char* d_out,
                                     uint64_t out_cap, uint64_t* d_out_off, uint64_t* out_bytes, void* stream) {
    return bg_sam_emit_dup_batch_dev(fm, sp, n_reads, d_contigs, n_contigs, d_names, d_fastq_text, d_recs, d_seq, d_qual, d_hits, d_strand, d_ops,
                                     d_multi, d_pairs, nullptr, d_out, out_cap, d_out_off, out_bytes, stream);
}

// the host flavour of a writer: `dev` (this file's, or bam_emit.hip's) between an upload and a download
typedef int (*sam_emit_dev_fn)(bg_fm*, const bg_sam_params_t*, uint64_t, const bg_sam_contig_t*, uint64_t, const char*, const uint8_t*,
                               const bg_fastq_record_t*, const uint8_t*, const uint8_t*, const bg_seed_hit_t*, const uint8_t*, const uint8_t*,
                               const bg_multi_hit_t*, const bg_pair_hit_t*, const uint8_t*, char*, uint64_t, uint64_t*, uint64_t*, void*);
static int sam_emit_host(sam_emit_dev_fn dev, bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* contigs,
                         uint64_t n_contigs, const char* names, const uint8_t* fastq_text, const bg_fastq_record_t* recs, const uint8_t* seq,
                         const uint8_t* qual, const bg_seed_hit_t* hits, const uint8_t* strand, const uint8_t* ops, const bg_multi_hit_t* multi,
                         const bg_pair_hit_t* pairs, const uint8_t* dup, char* out, uint64_t out_cap, uint64_t* out_off, uint64_t* out_bytes) {
    if (!out_off || !out_bytes) return BG_ERR_INVALID_ARG;
    *out_bytes = 0;
    int rc = sam_check(fm, sp, n_reads, n_contigs, pairs);
    if (rc) return rc;
    if (!out && out_cap) return BG_ERR_INVALID_ARG;
    if (n_reads && (!contigs || !names || !fastq_text || !recs || !seq || !qual || !hits || !strand || !ops)) return BG_ERR_INVALID_ARG;
    out_off[0] = 0;
    if (n_reads == 0) return BG_OK;
    const uint64_t n_slots = n_reads * sp->max_hits;
    // the buffers the records, the hits and the contigs point into end where the last of them ends (no description is written)
    const fq_extents e = fq_record_extents(recs, n_reads);
    uint64_t ops_bytes = 0, name_bytes = 0;
    for (uint64_t s = 0; s < n_slots; s++)
        if (hits[s].aln.score != BG_MIN_SCORE) ops_bytes = std::max<uint64_t>(ops_bytes, hits[s].aln.ops_off + hits[s].aln.n_ops);
    for (uint64_t c = 0; c < n_contigs; c++) name_bytes = std::max<uint64_t>(name_bytes, contigs[c].name_off + contigs[c].name_len);
    bg_stage s(fm->ctx, fm->ctx->stream);
    const bg_sam_contig_t* d_contigs = s.up(contigs, n_contigs);
    const char* d_names = s.up(names, name_bytes);
    const uint8_t* d_fq = s.up(fastq_text, e.id);
    const bg_fastq_record_t* d_recs = s.up(recs, n_reads);
    const uint8_t* d_seq = s.up(seq, e.seq);
    const uint8_t* d_qual = s.up(qual, e.qual);
    const bg_seed_hit_t* d_hits = s.up(hits, n_slots);
    const uint8_t* d_strand = s.up(strand, n_slots);
    const uint8_t* d_ops = s.up(ops, ops_bytes);
    const bg_multi_hit_t* d_multi = multi ? s.up(multi, n_reads) : nullptr;
    const bg_pair_hit_t* d_pairs = pairs ? s.up(pairs, n_reads / 2) : nullptr;
    const uint8_t* d_dup = dup ? s.up(dup, n_reads) : nullptr;
    uint64_t* d_off = s.out<uint64_t>(n_slots + 1);
    char* d_out = out ? s.out<char>(out_cap) : nullptr;  // null: a sizing call
    if (s.rc) return s.rc;
    rc = dev(fm, sp, n_reads, d_contigs, n_contigs, d_names, d_fq, d_recs, d_seq, d_qual, d_hits, d_strand, d_ops, d_multi, d_pairs, d_dup, d_out,
             out_cap, d_off, out_bytes, s.st);
    if (rc && rc != BG_ERR_OPS_CAP) return rc;
    s.down(out_off, d_off, n_slots + 1);
    if (!rc && out) s.down(out, d_out, *out_bytes);
    return s.sync() ? s.rc : rc;
}

extern "C" int bg_sam_emit_dup_batch(bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* contigs, uint64_t n_contigs,
                                     const char* names, const uint8_t* fastq_text, const bg_fastq_record_t* recs, const uint8_t* seq,
                                     const uint8_t* qual, const bg_seed_hit_t* hits, const uint8_t* strand, const uint8_t* ops,
                                     const bg_multi_hit_t* multi, const bg_pair_hit_t* pairs, const uint8_t* dup, char* out, uint64_t out_cap,
                                     uint64_t* out_off, uint64_t* out_bytes) {
    return sam_emit_host(bg_sam_emit_dup_batch_dev, fm, sp, n_reads, contigs, n_contigs, names, fastq_text, recs, seq, qual, hits, strand, ops, multi,
                         pairs, dup, out, out_cap, out_off, out_bytes);
}

extern "C" int bg_sam_emit_batch(bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* contigs, uint64_t n_contigs,
                                 const char* names, const uint8_t* fastq_text, const bg_fastq_record_t* recs, const uint8_t* seq,
                                 const uint8_t* qual, const bg_seed_hit_t* hits, const uint8_t* strand, const uint8_t* ops,
                                 const bg_multi_hit_t* multi, const bg_pair_hit_t* pairs, char* out, uint64_t out_cap, uint64_t* out_off,
                                 uint64_t* out_bytes) {
    return bg_sam_emit_dup_batch(fm, sp, n_reads, contigs, n_contigs, names, fastq_text, recs, seq, qual, hits, strand, ops, multi, pairs, nullptr,
                                 out, out_cap, out_off, out_bytes);
}
