// BAM records from seed-and-extend hits (bg_bam_emit_batch[_dev], bg_bam_header): the record of a slot is the BAM encoding
// (SAM v1.6, section 4.2; the rule is in include/biogpu.h) of the line the SAM writer gives that slot, so every field comes
// from the writer's own sam_line() and sam_md() and from sam_rule.h.  Those live in sam_emit.hip, whose line numbers
// tests/test_gpu_dev_pointer_alignment.py cites; rather than move them, this unit includes that file and is compiled in
// its place: one translation unit holds both writers and one definition of a line.
// The passes are the SAM writer's.  The length pass (one lane per slot) walks the slot's operations once for the number of
// CIGAR operations, the reference bases they consume (the bin, and the N of an over-long CIGAR), NM and the MD length,
// counts the slots BAM cannot hold, and writes the record length; a scan turns lengths into offsets.  The write pass gives a
// record a group of 16 or 32 lanes that stage it in LDS at its offset inside the output's 16-byte granule and store it 16
// bytes wide: lane 0 the fixed fields, lane 1 the tags, all of them the name, the packed bases and the qualities.  The
// serial walks — CIGAR words, MD — are left to a third kernel with one lane per slot, for the reason and at the measured
// cost sam_emit.hip's opening comment gives.  bam_layout() places every field for all three, so they cannot disagree.
#include "sam_emit.hip"

#include "bam_rule.h"

namespace {

struct BamDesc {  // what the length pass learned from a slot's operations, and where the third pass writes
    uint32_t n_cigar, ref_len, md_len, nm;
    uint32_t cigar_at, md_at;  // 0: nothing to write there (a record never starts with either)
};

// The operations sam_cigar() writes as letters, counted and (o != nullptr) written as BAM words at any address; ref_len
// receives the reference bases they consume.
__device__ uint32_t bam_cigar(const bg_alignment_t& al, const uint8_t* __restrict__ q, uint8_t* o, uint32_t* ref_len) {
    *ref_len = 0;
    if (!al.n_ops) return 0;
    uint32_t w = 0, ref = 0;
    auto emit = [&](uint32_t n, uint32_t op) {
        if (o) bam_put32(o + 4 * (size_t)w, bam_cigar_word(n, op));
        w++;
    };
    auto add = [&](uint32_t kind, uint32_t n) {
        if (kind > BG_OP_INS) return;
        emit(n, kind == BG_OP_MATCH ? BAM_CIGAR_EQ : kind == BG_OP_SUBST ? BAM_CIGAR_X : kind == BG_OP_DEL ? BAM_CIGAR_D : BAM_CIGAR_I);
        if (kind != BG_OP_INS) ref += n;
    };
    if (al.xstart > 0) emit(al.xstart, BAM_CIGAR_S);
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
    if (al.xlen > al.xend) emit(al.xlen - al.xend, BAM_CIGAR_S);
    *ref_len = ref;
    return w;
}

// where the parts of a record start, its length, and whether BAM can hold it
struct BamLayout {
    uint32_t name_len;   // l_read_name: the NUL included
    uint32_t n_cigar;    // the n_cigar_op field: 2 where the operations go into the CG tag
    uint32_t l_seq;
    uint32_t cigar_at, seq_at, qual_at, tags_at;
    uint32_t md_at, cg_at;  // the MD string; the CG tag's words (0: no such tag)
    uint32_t len;
    bool bad;
};
__device__ BamLayout bam_layout(const SamArgs& a, const SamLine& L, const BamDesc& d) {
    BamLayout y = {};
    const uint32_t ops = L.placed ? d.n_cigar : 0;
    const bool big = ops > BAM_MAX_CIGAR;
    y.name_len = (L.qname_len ? L.qname_len : 1) + 1;
    y.n_cigar = big ? 2 : ops;
    y.l_seq = L.seq_star ? 0 : L.seq_len;
    y.cigar_at = BAM_FIXED + y.name_len;
    y.seq_at = y.cigar_at + 4 * y.n_cigar;
    y.qual_at = y.seq_at + (y.l_seq + 1) / 2;
    y.tags_at = y.qual_at + y.l_seq;
    uint32_t w = y.tags_at;
    if (L.placed) {
        w += 3 + bam_int_size(L.score);
        if (L.has_xs) w += 3 + bam_int_size(L.xs);
        if (a.flags & BG_SAM_TAG_NM) w += 3 + bam_int_size(d.nm);
        if (a.flags & BG_SAM_TAG_MD) {
            y.md_at = w + 3;
            w += 3 + d.md_len + 1;
        }
        if (big) {
            y.cg_at = w + 8;
            w += 8 + 4 * ops;
        }
    }
    y.len = w;
    y.bad = L.qname_len > BAM_MAX_QNAME || (L.contig >= 0 && a.contigs[L.contig].len > BAM_MAX_REF) ||
            (L.next >= 0 && a.contigs[L.next].len > BAM_MAX_REF);
    return y;
}

// length pass: one lane per slot
__global__ __launch_bounds__(256) void bam_length_kernel(const SamArgs a, uint32_t* __restrict__ len, BamDesc* __restrict__ desc,
                                                         unsigned long long* __restrict__ n_bad) {
    const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= a.n_slots) return;
    const SamLine L = sam_line(a, slot);
    BamDesc d = {};
    if (!L.writes) {
        len[slot] = 0;
        desc[slot] = d;
        return;
    }
    if (L.placed) {
        const bg_seed_hit_t& h = a.hits[slot];
        const uint8_t* q = a.ops + h.aln.ops_off;
        d.n_cigar = bam_cigar(h.aln, q, nullptr, &d.ref_len);
        if (a.flags & (BG_SAM_TAG_NM | BG_SAM_TAG_MD)) d.md_len = sam_md(a, h, q, nullptr, &d.nm);
    }
    const BamLayout y = bam_layout(a, L, d);
    if (L.placed && d.n_cigar) d.cigar_at = y.cg_at ? y.cg_at : y.cigar_at;
    d.md_at = y.md_at;
    if (y.bad) atomicAdd(n_bad, 1ull);
    len[slot] = y.bad ? 0 : y.len;
    desc[slot] = d;
}

// the total and the number of slots BAM cannot hold side by side, for one read-back
__global__ void bam_tail_kernel(const uint64_t* __restrict__ total, unsigned long long* __restrict__ tail) { tail[0] = *total; }

// third pass: one lane per slot writes the CIGAR words and the MD string into the record the write pass left
__global__ __launch_bounds__(256) void bam_ops_kernel(const SamArgs a, const BamDesc* __restrict__ desc, const uint64_t* __restrict__ off,
                                                      uint8_t* __restrict__ out) {
    const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= a.n_slots) return;
    const BamDesc d = desc[slot];
    if (!d.cigar_at && !d.md_at) return;
    const bg_seed_hit_t& h = a.hits[slot];
    const uint8_t* q = a.ops + h.aln.ops_off;
    uint8_t* rec = out + off[slot];
    if (d.cigar_at) {
        uint32_t ref_len;
        bam_cigar(h.aln, q, rec + d.cigar_at, &ref_len);
    }
    if (d.md_at) {
        uint32_t nm;
        sam_md(a, h, q, (char*)rec + d.md_at, &nm);
    }
}

// One record by the G lanes of its group into dst (LDS or global memory): lane 0 the fixed fields, lane 1 the tags, all of
// them the name, SEQ and QUAL; the CIGAR words and the MD string stay blank for bam_ops_kernel.
template <int G>
__device__ void bam_format(const SamArgs& a, uint64_t slot, const BamDesc& d, uint8_t* dst, uint32_t lane, const uint8_t* s_comp,
                           const uint8_t* s_code) {
    const SamLine L = sam_line(a, slot);
    const BamLayout y = bam_layout(a, L, d);
    const uint64_t r = slot / a.K;
    const bg_fastq_record_t& rec = a.recs[r];
    if (L.qname_len) {
        const uint8_t* s = a.fq + rec.id_off;
        for (uint32_t i = lane; i < L.qname_len; i += G) dst[BAM_FIXED + i] = s[i];
    }
    if (y.l_seq) {
        const uint8_t* s = a.seq + rec.seq_off;
        const uint32_t n = y.l_seq;
        auto code = [&](uint32_t j) -> uint32_t { return j >= n ? 0u : L.rev ? s_code[s_comp[s[n - 1 - j]]] : s_code[s[j]]; };
        for (uint32_t i = lane; i < (n + 1) / 2; i += G) dst[y.seq_at + i] = (uint8_t)((code(2 * i) << 4) | code(2 * i + 1));
        if (L.qual_star) {
            for (uint32_t i = lane; i < n; i += G) dst[y.qual_at + i] = 0xFF;
        } else {
            const uint8_t* ql = a.qual + rec.qual_off;
            for (uint32_t i = lane; i < n; i += G) dst[y.qual_at + i] = (uint8_t)(ql[L.rev ? n - 1 - i : i] - 33);
        }
    }
    if (lane == 0) {
        const int64_t pos = (int64_t)L.pos - 1;
        bam_put32(dst, y.len - 4);
        bam_put32(dst + 4, (uint32_t)(int32_t)L.contig);
        bam_put32(dst + 8, (uint32_t)(int32_t)pos);
        dst[12] = (uint8_t)y.name_len;
        dst[13] = (uint8_t)L.mapq;
        bam_put16(dst + 14, bam_bin(pos, y.n_cigar ? d.ref_len : 0));
        bam_put16(dst + 16, y.n_cigar);
        bam_put16(dst + 18, L.flag);
        bam_put32(dst + 20, y.l_seq);
        bam_put32(dst + 24, (uint32_t)(int32_t)(L.next == -2 ? L.contig : L.next));
        bam_put32(dst + 28, (uint32_t)(int32_t)((int64_t)L.pnext - 1));
        bam_put32(dst + 32, (uint32_t)(int32_t)L.tlen);
        if (!L.qname_len) dst[BAM_FIXED] = '*';
        dst[BAM_FIXED + y.name_len - 1] = 0;
        if (y.cg_at) {  // the real operations are in the CG tag: <l_seq>S<reference length>N stands in for them
            bam_put32(dst + y.cigar_at, bam_cigar_word(y.l_seq, BAM_CIGAR_S));
            bam_put32(dst + y.cigar_at + 4, bam_cigar_word(d.ref_len, BAM_CIGAR_N));
        }
    }
    if (lane == 1 && L.placed) {
        uint8_t* t = dst + y.tags_at;
        t += bam_put_int(t, 'A', 'S', L.score);
        if (L.has_xs) t += bam_put_int(t, 'X', 'S', L.xs);
        if (a.flags & BG_SAM_TAG_NM) t += bam_put_int(t, 'N', 'M', d.nm);
        if (a.flags & BG_SAM_TAG_MD) {
            t[0] = 'M';
            t[1] = 'D';
            t[2] = 'Z';
            t[3 + d.md_len] = 0;
        }
        if (y.cg_at) {
            uint8_t* g = dst + y.cg_at - 8;
            g[0] = 'C';
            g[1] = 'G';
            g[2] = 'B';
            g[3] = 'I';
            bam_put32(g + 4, d.n_cigar);
        }
    }
}

// write pass: G lanes per slot, 256 / G slots per block
template <int G>
__global__ __launch_bounds__(256) void bam_write_kernel(const SamArgs a, const BamDesc* __restrict__ desc, const uint64_t* __restrict__ off,
                                                        uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[(256 / G) * kStageBuf];
    __shared__ __attribute__((aligned(4))) uint8_t s_comp[256];
    __shared__ uint8_t s_code[256];
    s_code[threadIdx.x] = (uint8_t)bam_base_code((uint8_t)threadIdx.x);
    load_complement(s_comp);
    const uint32_t g = threadIdx.x / G, lane = threadIdx.x % G;
    const uint64_t slot = (uint64_t)blockIdx.x * (256 / G) + g;
    uint64_t o0 = 0;
    uint32_t len = 0;
    if (slot < a.n_slots) {
        o0 = off[slot];
        len = (uint32_t)(off[slot + 1] - o0);
    }
    uint8_t* rec = out + o0;
    const uint32_t mis = (uint32_t)((uintptr_t)rec & 15);
    const bool staged = len && mis + len <= kStageBuf;
    uint8_t* stage = s_stage + g * kStageBuf + mis;
    if (len) bam_format<G>(a, slot, desc[slot], staged ? stage : rec, lane, s_comp, s_code);
    __syncthreads();
    if (!staged) return;
    // head up to the first 16-byte boundary and tail behind the last one byte by byte, everything between as 16-byte stores
    const sam_copy_plan_t p = sam_copy_plan(mis, len);
    const uint32_t body = (uint32_t)p.body;
    if (lane < p.head) rec[lane] = stage[lane];
    for (uint32_t i = lane; i < body; i += G) *(uint4*)(rec + p.head + 16 * i) = *(const uint4*)(stage + p.head + 16 * i);
    if (lane < p.tail) rec[p.head + 16 * body + lane] = stage[p.head + 16 * body + lane];
}

void put_i32(std::string& s, int64_t v) {
    for (int i = 0; i < 4; i++) s.push_back((char)((uint64_t)v >> (8 * i)));
}

}  // namespace

extern "C" int bg_bam_header(const bg_sam_contig_t* contigs, uint64_t n_contigs, const char* names, int sort_order, uint8_t* out,
                             uint64_t out_cap, uint64_t* out_bytes) {
    if (!out_bytes || (!out && out_cap)) return BG_ERR_INVALID_ARG;
    uint64_t n_text = 0;
    int rc = bg_sam_header_so(contigs, n_contigs, names, sort_order, nullptr, 0, &n_text);
    if (rc) return rc;
    if (n_text > BAM_MAX_REF || n_contigs > BAM_MAX_REF) return BG_ERR_UNSUPPORTED;
    for (uint64_t c = 0; c < n_contigs; c++)
        if (contigs[c].len > BAM_MAX_REF) return BG_ERR_UNSUPPORTED;
    std::string s("BAM\1", 4);
    put_i32(s, (int64_t)n_text);
    s.resize(8 + n_text);
    if ((rc = bg_sam_header_so(contigs, n_contigs, names, sort_order, &s[8], n_text, &n_text))) return rc;
    put_i32(s, (int64_t)n_contigs);
    for (uint64_t c = 0; c < n_contigs; c++) {
        put_i32(s, (int64_t)contigs[c].name_len + 1);
        s.append(names + contigs[c].name_off, contigs[c].name_len);
        s.push_back('\0');
        put_i32(s, (int64_t)contigs[c].len);
    }
    *out_bytes = s.size();
    if (!out) return BG_OK;
    if (s.size() > out_cap) return BG_ERR_OPS_CAP;
    memcpy(out, s.data(), s.size());
    return BG_OK;
}

extern "C" int bg_bam_emit_batch_dev(bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* d_contigs, uint64_t n_contigs,
                                     const char* d_names, const uint8_t* d_fastq_text, const bg_fastq_record_t* d_recs, const uint8_t* d_seq,
                                     const uint8_t* d_qual, const bg_seed_hit_t* d_hits, const uint8_t* d_strand, const uint8_t* d_ops,
                                     const bg_multi_hit_t* d_multi, const bg_pair_hit_t* d_pairs, const uint8_t* d_dup, uint8_t* d_out,
                                     uint64_t out_cap, uint64_t* d_out_off, uint64_t* out_bytes, void* stream) {
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
    BamDesc* d_desc;
    uint64_t* d_sums;
    unsigned long long* d_tail;  // total, slots BAM cannot hold
    if ((rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_len = cv.take<uint32_t>(n_slots);
        d_desc = cv.take<BamDesc>(n_slots);
        d_sums = cv.take<uint64_t>(bg_scan_sums_words(n_slots));
        d_tail = cv.take<unsigned long long>(2);
    }))) return rc;
    const SamArgs a = {n_slots, sp->max_hits, sp->flags, d_contigs, n_contigs, d_names, d_fastq_text, d_recs, d_seq, d_qual, d_hits,
                       d_strand, d_ops, d_multi, (sp->flags & BG_SAM_PAIRED) ? d_pairs : nullptr, (const uint8_t*)fm->d_text, fm->n_text, d_dup};
    const dim3 per_slot((uint32_t)((n_slots + 255) / 256));
    BG_HIP(hipMemsetAsync(d_tail, 0, 16, st));
    bam_length_kernel<<<per_slot, dim3(256), 0, st>>>(a, d_len, d_desc, d_tail + 1);
    BG_HIP(hipGetLastError());
    if ((rc = bg_scan_u32(d_len, n_slots, d_out_off, d_sums, st))) return rc;
    bam_tail_kernel<<<dim3(1), dim3(1), 0, st>>>(d_out_off + n_slots, d_tail);
    unsigned long long tail[2] = {0, 0};
    BG_HIP(hipMemcpyAsync(tail, d_tail, 16, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    *out_bytes = tail[0];
    if (tail[1]) {
        bg_tls_error = std::to_string(tail[1]) + " slot(s) with a QNAME above 254 bytes or on a contig longer than 2^31 - 1";
        return BG_ERR_UNSUPPORTED;
    }
    if (!d_out) return BG_OK;
    if (tail[0] > out_cap) return BG_ERR_OPS_CAP;
    if (ctx->sam_lanes == 32)
        bam_write_kernel<32><<<dim3((uint32_t)((n_slots + 7) / 8)), dim3(256), 0, st>>>(a, d_desc, d_out_off, d_out);
    else
        bam_write_kernel<16><<<dim3((uint32_t)((n_slots + 15) / 16)), dim3(256), 0, st>>>(a, d_desc, d_out_off, d_out);
    bam_ops_kernel<<<per_slot, dim3(256), 0, st>>>(a, d_desc, d_out_off, d_out);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

static int bam_emit_dev_chars(bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* d_contigs, uint64_t n_contigs,
                              const char* d_names, const uint8_t* d_fastq_text, const bg_fastq_record_t* d_recs, const uint8_t* d_seq,
                              const uint8_t* d_qual, const bg_seed_hit_t* d_hits, const uint8_t* d_strand, const uint8_t* d_ops,
                              const bg_multi_hit_t* d_multi, const bg_pair_hit_t* d_pairs, const uint8_t* d_dup, char* d_out, uint64_t out_cap,
                              uint64_t* d_out_off, uint64_t* out_bytes, void* stream) {
    return bg_bam_emit_batch_dev(fm, sp, n_reads, d_contigs, n_contigs, d_names, d_fastq_text, d_recs, d_seq, d_qual, d_hits, d_strand, d_ops,
                                 d_multi, d_pairs, d_dup, (uint8_t*)d_out, out_cap, d_out_off, out_bytes, stream);
}

extern "C" int bg_bam_emit_batch(bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* contigs, uint64_t n_contigs,
                                 const char* names, const uint8_t* fastq_text, const bg_fastq_record_t* recs, const uint8_t* seq,
                                 const uint8_t* qual, const bg_seed_hit_t* hits, const uint8_t* strand, const uint8_t* ops,
                                 const bg_multi_hit_t* multi, const bg_pair_hit_t* pairs, const uint8_t* dup, uint8_t* out, uint64_t out_cap,
                                 uint64_t* out_off, uint64_t* out_bytes) {
    return sam_emit_host(bam_emit_dev_chars, fm, sp, n_reads, contigs, n_contigs, names, fastq_text, recs, seq, qual, hits, strand, ops, multi, pairs,
                         dup, (char*)out, out_cap, out_off, out_bytes);
}
