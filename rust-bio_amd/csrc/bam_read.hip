// Reading BAM on the device (bg_bam_header_parse, bg_bam_records[_dev], bg_bam_reads[_dev], bg_bam_sort_keys[_dev]; the
// rules are in include/biogpu.h, the bodies in bam_read_rule.h).
//
// The record table.  Records are a serial chain like BGZF members (a record's start is its predecessor's + 4 + block_size),
// so the method is the block table's (bgzf_inflate.hip): candidates — every position from body_off on at which an accepted
// record stands (bamr_verdict) — counted per chunk of 2048 positions, the counts scanned, the positions compacted in order;
// a candidate's successor by binary search; membership of the chain from candidate 0 marked by doubling; the marked ones
// counted, scanned, written; one thread judges the chain's end.  Two things differ and are NOT copied from there.  Records
// carry no signature, so accepted positions have no minimum distance (4 bytes apart is possible: the second's block_size is
// the first's refID): a thread counts and writes every one of its 8 positions, not one.  And nothing bounds the candidates
// by the input's length short of one a position: they are counted first, the total is read back, and the scratch (18 bytes
// a candidate) is sized from it — one synchronisation more than bg_bgzf_blocks.  The per-chunk counts live in ctx->aux, the
// candidate arrays in ctx->tb: bg_reserve frees what it grows, and the first must survive the second's allocation.
// The kernels are second copies of blk_succ / blk_double / blk_rows: those sit in bgzf_inflate.hip's unnamed namespace and
// read BSIZE / ISIZE; only the ten lines of the doubling kernel are the same text.
//
// The reads.  A length pass with one lane a record (the slot check, the filter, the lengths), three scans (the rank among the
// kept records, the base and the quality offsets), one read-back of the totals and the first bad slot, and a write pass that
// gives a record 16 lanes, as bam_emit.hip's write pass does: bases unpacked from two-a-byte, qualities + 33, reversed and
// complemented under BG_BAM_READS_ORIGINAL, stored 16 bytes wide between the destination's own 16-byte boundaries
// (bamr_column_lane); lane 0 writes the record once the group's flags are in.
#include "bg_common.h"
#include "dna_complement.h"
#include "bam_read_rule.h"

namespace {

constexpr bool rc_table_agrees() {
    const ComplementTable t = make_complement();
    for (int c = 0; c < 16; c++)
        if (t.v[(uint8_t)BAMR_BASES[c]] != (uint8_t)BAMR_BASES_RC[c]) return false;
    return true;
}
static_assert(rc_table_agrees(), "BAMR_BASES_RC is not dna::complement of BAMR_BASES");

constexpr uint32_t REC_CHUNK = 2048;  // positions (candidates) a workgroup of 256 takes: 8 consecutive ones a thread
struct rec_result_t {
    uint64_t err, n_records, first_bad, tail;
};

// exclusive prefix of v over the 256 threads of the workgroup; *total: the sum
__device__ uint32_t rec_scan256(uint32_t v, uint32_t* s /* [256] */, uint32_t* total) {
    const uint32_t t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint32_t u = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += u;
        __syncthreads();
    }
    const uint32_t incl = s[t];
    *total = s[255];
    __syncthreads();
    return incl - v;
}

// chunk c of the positions from body_off on: WRITE false: cnt[c] = its candidates; WRITE true: their positions to
// pos[base[c] ..), every one (up to 8 a thread), below n_cand
template <bool WRITE>
__global__ __launch_bounds__(256) void rec_cand_kernel(const uint8_t* __restrict__ in, uint64_t in_bytes, uint64_t body_off, uint64_t n_ref,
                                                       uint32_t* __restrict__ cnt, const uint64_t* __restrict__ base, uint64_t* __restrict__ pos,
                                                       uint64_t n_cand) {
    __shared__ uint32_t s[256];
    const uint64_t p0 = body_off + (uint64_t)blockIdx.x * REC_CHUNK + 8ull * threadIdx.x;
    uint32_t mask = 0;
    uint64_t size;
    for (uint32_t i = 0; i < 8; i++)
        if (p0 + i < in_bytes && bamr_verdict(in, in_bytes, p0 + i, n_ref, &size) == BG_OK) mask |= 1u << i;
    uint32_t total;
    const uint32_t before = rec_scan256((uint32_t)__popc(mask), s, &total);
    if (!WRITE) {
        if (threadIdx.x == 0) cnt[blockIdx.x] = total;
        return;
    }
    uint64_t at = base[blockIdx.x] + before;
    for (uint32_t i = 0; i < 8; i++)
        if ((mask >> i) & 1u) {
            if (at < n_cand) pos[at] = p0 + i;  // (always: the same verdicts were counted)
            at++;
        }
}

// candidate i: its successor (BAMR_NONE: none, then it is a tail), the chain's first mark
__global__ __launch_bounds__(256) void rec_succ_kernel(const uint8_t* __restrict__ in, uint64_t body_off, uint64_t n, const uint64_t* __restrict__ pos,
                                                       uint32_t* __restrict__ jump, uint8_t* __restrict__ chain, uint8_t* __restrict__ tail) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint64_t target = pos[i] + 4 + bai_get32(in + pos[i]);
        uint64_t lo = i + 1, hi = n;  // the first candidate at or behind target
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (pos[mid] < target) lo = mid + 1;
            else hi = mid;
        }
        const bool found = lo < n && pos[lo] == target;
        jump[i] = found ? (uint32_t)lo : BAMR_NONE;
        tail[i] = !found;
        chain[i] = i == 0 && pos[0] == body_off;
    }
}
__global__ __launch_bounds__(256) void rec_double_kernel(uint64_t n, const uint32_t* __restrict__ jin, uint32_t* __restrict__ jout, uint8_t* chain) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t j = jin[i];
        if (j == BAMR_NONE) {
            jout[i] = BAMR_NONE;
            continue;
        }
        if (chain[i]) chain[j] = 1;  // (a mark set in this round may already mark on: it marks members only)
        jout[i] = jin[j];
    }
}
// chunk c of the candidates: WRITE false: cnt_m[c] = its members, and the chain's tail is noted; WRITE true (no error, a table
// given): the members' rows of off, and the closing row
template <bool WRITE>
__global__ __launch_bounds__(256) void rec_rows_kernel(uint64_t in_bytes, uint64_t n, const uint64_t* __restrict__ pos, const uint8_t* __restrict__ chain,
                                                       const uint8_t* __restrict__ tail, uint32_t* __restrict__ cnt_m, const uint64_t* __restrict__ base_m,
                                                       rec_result_t* __restrict__ res, uint64_t* __restrict__ off) {
    __shared__ uint32_t s[256];
    if (WRITE && res->err) return;
    const uint64_t i0 = (uint64_t)blockIdx.x * REC_CHUNK + 8ull * threadIdx.x;
    uint32_t m = 0;
    for (uint32_t k = 0; k < 8; k++)
        if (i0 + k < n && chain[i0 + k]) {
            m++;
            if (!WRITE && tail[i0 + k]) res->tail = i0 + k;  // the one member without a successor
        }
    uint32_t total_m;
    const uint32_t before_m = rec_scan256(m, s, &total_m);
    if (!WRITE) {
        if (threadIdx.x == 0) cnt_m[blockIdx.x] = total_m;
        return;
    }
    uint64_t row = base_m[blockIdx.x] + before_m;
    for (uint32_t k = 0; k < 8; k++)
        if (i0 + k < n && chain[i0 + k]) off[row++] = pos[i0 + k];
    if (blockIdx.x == 0 && threadIdx.x == 0) off[res->n_records] = in_bytes;
}
// one thread: the total, where the chain ends, the error
__global__ void rec_finish_kernel(const uint8_t* __restrict__ in, uint64_t in_bytes, uint64_t body_off, const uint64_t* __restrict__ pos,
                                  const uint64_t* __restrict__ total_m, uint64_t cap_records, uint32_t tables, rec_result_t* __restrict__ res) {
    res->n_records = *total_m;
    res->first_bad = UINT64_MAX;
    res->err = BG_OK;
    const uint64_t end = res->tail == UINT64_MAX ? body_off : pos[res->tail] + 4 + bai_get32(in + pos[res->tail]);
    if (end != in_bytes) {  // what stands there was not accepted (it would be a candidate, and the tail's successor)
        res->err = (uint64_t)(int64_t)BG_ERR_INVALID_ARG;
        res->first_bad = *total_m;
    } else if (tables && *total_m > cap_records) {
        res->err = (uint64_t)(int64_t)BG_ERR_OPS_CAP;
    }
}

int records_args(const bg_ctx* ctx, const void* in, uint64_t in_bytes, uint64_t body_off, const void* off, uint64_t cap_records, const uint64_t* n_records) {
    if (!ctx || !n_records || (in_bytes && !in) || body_off > in_bytes || (!off && cap_records)) return BG_ERR_INVALID_ARG;
    return in_bytes >> 35 ? BG_ERR_TOO_LARGE : BG_OK;
}

// ---- the reads and the keys -------------------------------------------------------------------------------------------------
constexpr int READ_G = 16;  // lanes a record in the write pass
struct ReadArgs {
    uint64_t n;  // slots
    const uint8_t* bam;
    const uint64_t* off;
    uint64_t n_ref;
    bg_bam_reads_t prm;
};
// the four words read back
struct read_result_t {
    unsigned long long first_bad, n_reads, seq_bytes, qual_bytes;
};

// length pass: one lane a slot
__global__ __launch_bounds__(256) void read_length_kernel(const ReadArgs a, uint32_t* __restrict__ keep, uint32_t* __restrict__ slen,
                                                          uint32_t* __restrict__ qlen, read_result_t* __restrict__ res) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t o0 = a.off[i], o1 = a.off[i + 1];
    uint32_t k = 0, sl = 0, ql = 0;
    if (o1 != o0) {
        if (!bamr_slot_ok(a.bam, o0, o1, a.n_ref)) {
            atomicMin(&res->first_bad, (unsigned long long)i);
        } else {
            const uint8_t* r = a.bam + o0;
            const bamr_fields_t f = bamr_fields(r);
            if (bamr_kept(f.flag, a.prm)) {
                k = 1;
                sl = f.l_seq;
                ql = bamr_qual_len(r, f);
            }
        }
    }
    keep[i] = k;
    slen[i] = sl;
    qlen[i] = ql;
}
__global__ void read_tail_kernel(uint64_t n, const uint64_t* __restrict__ rank, const uint64_t* __restrict__ soff, const uint64_t* __restrict__ qoff,
                                 read_result_t* __restrict__ res) {
    res->n_reads = rank[n];
    res->seq_bytes = soff[n];
    res->qual_bytes = qoff[n];
}
// write pass: READ_G lanes a slot, 256 / READ_G slots a block
__global__ __launch_bounds__(256) void read_write_kernel(const ReadArgs a, const uint32_t* __restrict__ keep, const uint64_t* __restrict__ rank,
                                                         const uint64_t* __restrict__ soff, const uint64_t* __restrict__ qoff,
                                                         bg_fastq_record_t* __restrict__ recs, uint8_t* __restrict__ seq, uint64_t* __restrict__ seq_off,
                                                         uint8_t* __restrict__ qual, uint64_t* __restrict__ qual_off, uint64_t* __restrict__ src) {
    const uint32_t lane = threadIdx.x % READ_G;
    const uint64_t i = (uint64_t)blockIdx.x * (256 / READ_G) + threadIdx.x / READ_G;
    const bool live = i < a.n && keep[i];  // (uniform over the lanes of a record)
    uint32_t flags = 0, ql = 0;
    uint64_t o = 0, so = 0, qo = 0;
    bamr_fields_t f = {};
    if (live) {
        o = a.off[i];
        so = soff[i];
        qo = qoff[i];
        const uint8_t* r = a.bam + o;
        f = bamr_fields(r);
        ql = bamr_qual_len(r, f);
        const bool rev = bamr_reversed(f.flag, a.prm);
        flags = bamr_column_lane<true>(r + f.seq_at, f.l_seq, rev, seq + so, lane, READ_G);
        if (ql) flags |= bamr_column_lane<false>(r + f.qual_at, ql, rev, qual + qo, lane, READ_G) << 1;
    }
    // "any" over the lanes of the record
    const uint32_t sh = (threadIdx.x & 63u) / READ_G * READ_G;
    const uint64_t gm = ((1ull << READ_G) - 1) << sh;
    const uint32_t eq = (__ballot(flags & 1u) & gm) != 0, hi = (__ballot(flags & 2u) & gm) != 0;
    if (live && lane == 0) {
        const uint64_t j = rank[i];
        recs[j] = bamr_read_record(a.bam + o, o, f, ql, so, qo, eq, hi);
        seq_off[j] = so;
        qual_off[j] = qo;
        if (src) src[j] = i;
    }
    if (i == 0 && lane == 0) {  // the closing rows (slot 0 exists: the pass is not launched without slots)
        seq_off[rank[a.n]] = soff[a.n];
        qual_off[rank[a.n]] = qoff[a.n];
    }
}

// one lane a slot
__global__ __launch_bounds__(256) void read_keys_kernel(const ReadArgs a, const bg_sam_contig_t* __restrict__ contigs, uint64_t* __restrict__ key,
                                                        read_result_t* __restrict__ res) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t o0 = a.off[i], o1 = a.off[i + 1];
    if (o1 != o0 && !bamr_slot_ok(a.bam, o0, o1, a.n_ref)) {
        atomicMin(&res->first_bad, (unsigned long long)i);
        key[i] = UINT64_MAX;
        return;
    }
    key[i] = bamr_key(a.bam + o0, o1 - o0, contigs);
}

int reads_args(const bg_ctx* ctx, const bg_bam_reads_t* prm, uint64_t n, const void* bam, const void* off, const void* recs, uint64_t cap_reads,
               const void* seq, uint64_t seq_cap, const void* seq_off, const void* qual, uint64_t qual_cap, const void* qual_off, const void* src,
               const uint64_t* n_reads, const uint64_t* seq_bytes, const uint64_t* qual_bytes) {
    if (!ctx || !prm || !n_reads || !seq_bytes || !qual_bytes || (n && (!bam || !off))) return BG_ERR_INVALID_ARG;
    if (prm->flags & ~(uint32_t)BG_BAM_READS_ORIGINAL) return BG_ERR_INVALID_ARG;
    if (!recs && (cap_reads || seq_cap || qual_cap || seq || seq_off || qual || qual_off || src)) return BG_ERR_INVALID_ARG;
    if (recs && (!seq_off || !qual_off || (!seq && seq_cap) || (!qual && qual_cap))) return BG_ERR_INVALID_ARG;
    return n >= 0xFFFFFFFFull ? BG_ERR_TOO_LARGE : BG_OK;
}

}  // namespace

extern "C" int bg_bam_header_parse(const uint8_t* in, uint64_t bytes, bg_sam_contig_t* contigs, uint64_t cap_contigs, char* names, uint64_t names_cap,
                                   uint64_t* n_contigs, uint64_t* names_bytes, uint64_t* text_off, uint64_t* text_len, uint64_t* body_off,
                                   uint64_t* need) {
    if (!n_contigs || !names_bytes || !text_off || !text_len || !body_off || !need || (bytes && !in) || (!contigs && cap_contigs) ||
        (!names && names_cap) || (!contigs != !names && (cap_contigs || names_cap)))
        return BG_ERR_INVALID_ARG;
    *n_contigs = *names_bytes = *text_off = *text_len = *body_off = *need = 0;
    bamr_header_t h;
    int rc = bamr_header_parse(in, bytes, nullptr, nullptr, &h);
    *need = h.need;
    if (rc == BG_ERR_INVALID_ARG) return bg_refuse("bg_bam_header_parse: no BAM magic, a negative l_text, n_ref or l_ref, an l_name below 1 or a name without its NUL");
    if (rc) return rc;
    *n_contigs = h.n_contigs;
    *names_bytes = h.names_bytes;
    *text_off = h.text_off;
    *text_len = h.text_len;
    *body_off = h.body_off;
    if (!contigs && !names) return BG_OK;
    if (h.n_contigs > cap_contigs || h.names_bytes > names_cap) return BG_ERR_OPS_CAP;  // (*need == 0: the prefix is long enough)
    return bamr_header_parse(in, bytes, contigs, names, &h);
}

extern "C" int bg_bam_records_dev(bg_ctx* ctx, const uint8_t* d_bam, uint64_t in_bytes, uint64_t body_off, uint64_t n_ref, uint64_t* d_off,
                                  uint64_t cap_records, uint64_t* n_records, uint64_t* n_candidates, uint64_t* first_bad, void* stream) {
    int rc = records_args(ctx, d_bam, in_bytes, body_off, d_off, cap_records, n_records);
    if (rc) return rc;
    *n_records = 0;
    if (n_candidates) *n_candidates = 0;
    if (first_bad) *first_bad = UINT64_MAX;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    if (body_off == in_bytes) {  // no record: the closing row alone
        if (d_off) BG_HIP(hipMemcpyAsync(d_off, &in_bytes, 8, hipMemcpyHostToDevice, st));
        BG_HIP(hipStreamSynchronize(st));
        return BG_OK;
    }
    bg_scratch_guard guard(ctx, st);
    // the count
    const uint64_t n_pos = in_bytes - body_off, n_chunks = (n_pos + REC_CHUNK - 1) / REC_CHUNK;
    uint64_t *d_off1, *d_sums1;
    rec_result_t* d_res;
    uint32_t* d_cnt1;
    if ((rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_off1 = cv.take<uint64_t>(n_chunks + 1), d_sums1 = cv.take<uint64_t>(bg_scan_sums_words(n_chunks));
        d_res = cv.take<rec_result_t>(1);
        d_cnt1 = cv.take<uint32_t>(n_chunks);
    }))) return rc;
    BG_HIP(hipMemsetAsync(d_res, 0xFF, sizeof(rec_result_t), st));
    rec_cand_kernel<false><<<dim3((uint32_t)n_chunks), dim3(256), 0, st>>>(d_bam, in_bytes, body_off, n_ref, d_cnt1, nullptr, nullptr, 0);
    BG_HIP(hipGetLastError());
    if ((rc = bg_scan_u32(d_cnt1, n_chunks, d_off1, d_sums1, st))) return rc;
    uint64_t n_cand = 0;
    BG_HIP(hipMemcpyAsync(&n_cand, d_off1 + n_chunks, 8, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    if (n_candidates) *n_candidates = n_cand;
    if (n_cand >= BAMR_NONE) return BG_ERR_TOO_LARGE;
    // the candidates: 18 bytes each
    const uint64_t cap = n_cand ? n_cand : 1, c_chunks = (cap + REC_CHUNK - 1) / REC_CHUNK;
    uint64_t *d_pos, *d_offm, *d_sums2;
    uint32_t *d_jumps, *d_cntm;
    uint8_t *d_chain, *d_tail;
    if ((rc = bg_reserve_carved(&ctx->tb, &ctx->tb_bytes, [&](bg_carve& cv) {
        d_pos = cv.take<uint64_t>(cap), d_offm = cv.take<uint64_t>(c_chunks + 1), d_sums2 = cv.take<uint64_t>(bg_scan_sums_words(c_chunks));
        d_jumps = cv.take<uint32_t>(2 * cap);  // one piece: the two halves the doubling rounds swap
        d_cntm = cv.take<uint32_t>(c_chunks);
        d_chain = cv.take<uint8_t>(cap), d_tail = cv.take<uint8_t>(cap);
    }))) return rc;
    uint32_t* d_jump[2] = {d_jumps, d_jumps + cap};
    const uint32_t tables = d_off ? 1u : 0u;
    const uint32_t grid = (uint32_t)((cap + 255) / 256 < 2048 ? (cap + 255) / 256 : 2048);
    if (n_cand) {
        rec_cand_kernel<true><<<dim3((uint32_t)n_chunks), dim3(256), 0, st>>>(d_bam, in_bytes, body_off, n_ref, nullptr, d_off1, d_pos, n_cand);
        rec_succ_kernel<<<dim3(grid), dim3(256), 0, st>>>(d_bam, body_off, n_cand, d_pos, d_jump[0], d_chain, d_tail);
        const uint32_t rounds = bamr_rounds(n_pos);
        for (uint32_t k = 0; k < rounds; k++) rec_double_kernel<<<dim3(grid), dim3(256), 0, st>>>(n_cand, d_jump[k & 1], d_jump[(k + 1) & 1], d_chain);
    }
    rec_rows_kernel<false><<<dim3((uint32_t)c_chunks), dim3(256), 0, st>>>(in_bytes, n_cand, d_pos, d_chain, d_tail, d_cntm, nullptr, d_res, nullptr);
    BG_HIP(hipGetLastError());
    if ((rc = bg_scan_u32(d_cntm, c_chunks, d_offm, d_sums2, st))) return rc;
    rec_finish_kernel<<<dim3(1), dim3(1), 0, st>>>(d_bam, in_bytes, body_off, d_pos, d_offm + c_chunks, cap_records, tables, d_res);
    if (tables) rec_rows_kernel<true><<<dim3((uint32_t)c_chunks), dim3(256), 0, st>>>(in_bytes, n_cand, d_pos, d_chain, d_tail, nullptr, d_offm, d_res, d_off);
    BG_HIP(hipGetLastError());
    rec_result_t r;
    BG_HIP(hipMemcpyAsync(&r, d_res, sizeof r, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    *n_records = r.n_records;
    if (first_bad) *first_bad = r.first_bad;
    rc = (int)(int64_t)r.err;
    if (rc == BG_ERR_INVALID_ARG)
        return bg_refuse(("bg_bam_records: no BAM record where the chain arrives behind " + std::to_string(r.n_records) + " record(s), or one that leaves the input").c_str());
    return rc;
}

extern "C" int bg_bam_records(bg_ctx* ctx, const uint8_t* bam, uint64_t in_bytes, uint64_t body_off, uint64_t n_ref, uint64_t* off,
                              uint64_t cap_records, uint64_t* n_records, uint64_t* n_candidates, uint64_t* first_bad) {
    int rc = records_args(ctx, bam, in_bytes, body_off, off, cap_records, n_records);
    if (rc) return rc;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_bam = s.up(bam, in_bytes);
    uint64_t* d_off = off ? s.out<uint64_t>(cap_records + 1) : nullptr;
    if (s.rc) return s.rc;
    if ((rc = bg_bam_records_dev(ctx, d_bam, in_bytes, body_off, n_ref, d_off, cap_records, n_records, n_candidates, first_bad, s.st))) return rc;
    if (off) s.down(off, d_off, *n_records + 1);
    return s.sync();
}

extern "C" int bg_bam_reads_dev(bg_ctx* ctx, const bg_bam_reads_t* prm, uint64_t n_records, const uint8_t* d_bam, const uint64_t* d_off, uint64_t n_ref,
                                bg_fastq_record_t* d_recs, uint64_t cap_reads, uint8_t* d_seq, uint64_t seq_cap, uint64_t* d_seq_off, uint8_t* d_qual,
                                uint64_t qual_cap, uint64_t* d_qual_off, uint64_t* d_src, uint64_t* n_reads, uint64_t* seq_bytes,
                                uint64_t* qual_bytes, uint64_t* first_bad, void* stream) {
    if (first_bad) *first_bad = UINT64_MAX;
    int rc = reads_args(ctx, prm, n_records, d_bam, d_off, d_recs, cap_reads, d_seq, seq_cap, d_seq_off, d_qual, qual_cap, d_qual_off, d_src, n_reads,
                        seq_bytes, qual_bytes);
    if (rc) return rc;
    *n_reads = *seq_bytes = *qual_bytes = 0;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    const uint64_t n = n_records;
    if (!n) {
        if (d_recs) {
            BG_HIP(hipMemsetAsync(d_seq_off, 0, 8, st));
            BG_HIP(hipMemsetAsync(d_qual_off, 0, 8, st));
            BG_HIP(hipStreamSynchronize(st));
        }
        return BG_OK;
    }
    bg_scratch_guard guard(ctx, st);
    uint64_t *d_rank, *d_soff, *d_qoff, *d_sums;
    read_result_t* d_res;
    uint32_t *d_keep, *d_slen, *d_qlen;
    if ((rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_rank = cv.take<uint64_t>(n + 1), d_soff = cv.take<uint64_t>(n + 1), d_qoff = cv.take<uint64_t>(n + 1);
        d_sums = cv.take<uint64_t>(bg_scan_sums_words(n));
        d_res = cv.take<read_result_t>(1);
        d_keep = cv.take<uint32_t>(n), d_slen = cv.take<uint32_t>(n), d_qlen = cv.take<uint32_t>(n);
    }))) return rc;
    const ReadArgs a = {n, d_bam, d_off, n_ref, *prm};
    BG_HIP(hipMemsetAsync(d_res, 0xFF, 8, st));
    read_length_kernel<<<lanes(n), dim3(256), 0, st>>>(a, d_keep, d_slen, d_qlen, d_res);
    BG_HIP(hipGetLastError());
    if ((rc = bg_scan_u32(d_keep, n, d_rank, d_sums, st))) return rc;
    if ((rc = bg_scan_u32(d_slen, n, d_soff, d_sums, st))) return rc;
    if ((rc = bg_scan_u32(d_qlen, n, d_qoff, d_sums, st))) return rc;
    read_tail_kernel<<<dim3(1), dim3(1), 0, st>>>(n, d_rank, d_soff, d_qoff, d_res);
    read_result_t r;
    BG_HIP(hipMemcpyAsync(&r, d_res, sizeof r, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    if (r.first_bad != UINT64_MAX) {
        if (first_bad) *first_bad = r.first_bad;
        return bg_refuse(("bg_bam_reads: slot " + std::to_string(r.first_bad) + " is no BAM record").c_str());
    }
    *n_reads = r.n_reads;
    *seq_bytes = r.seq_bytes;
    *qual_bytes = r.qual_bytes;
    if (!d_recs) return BG_OK;
    if (r.n_reads > cap_reads || r.seq_bytes > seq_cap || r.qual_bytes > qual_cap) return BG_ERR_OPS_CAP;
    read_write_kernel<<<dim3((uint32_t)((n + 256 / READ_G - 1) / (256 / READ_G))), dim3(256), 0, st>>>(a, d_keep, d_rank, d_soff, d_qoff, d_recs, d_seq,
                                                                                                      d_seq_off, d_qual, d_qual_off, d_src);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

extern "C" int bg_bam_reads(bg_ctx* ctx, const bg_bam_reads_t* prm, uint64_t n_records, const uint8_t* bam, const uint64_t* off, uint64_t n_ref,
                            bg_fastq_record_t* recs, uint64_t cap_reads, uint8_t* seq, uint64_t seq_cap, uint64_t* seq_off, uint8_t* qual,
                            uint64_t qual_cap, uint64_t* qual_off, uint64_t* src, uint64_t* n_reads, uint64_t* seq_bytes, uint64_t* qual_bytes,
                            uint64_t* first_bad) {
    if (first_bad) *first_bad = UINT64_MAX;
    int rc = reads_args(ctx, prm, n_records, bam, off, recs, cap_reads, seq, seq_cap, seq_off, qual, qual_cap, qual_off, src, n_reads, seq_bytes,
                        qual_bytes);
    if (rc) return rc;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_bam = s.up(bam, n_records ? off[n_records] : 0);
    const uint64_t* d_off = s.up(off, n_records ? n_records + 1 : 0);
    bg_fastq_record_t* d_recs = recs ? s.out<bg_fastq_record_t>(cap_reads) : nullptr;
    uint8_t* d_seq = recs ? s.out<uint8_t>(seq_cap) : nullptr;
    uint8_t* d_qual = recs ? s.out<uint8_t>(qual_cap) : nullptr;
    uint64_t* d_seq_off = recs ? s.out<uint64_t>(cap_reads + 1) : nullptr;
    uint64_t* d_qual_off = recs ? s.out<uint64_t>(cap_reads + 1) : nullptr;
    uint64_t* d_src = src ? s.out<uint64_t>(cap_reads) : nullptr;
    if (s.rc) return s.rc;
    if ((rc = bg_bam_reads_dev(ctx, prm, n_records, d_bam, d_off, n_ref, d_recs, cap_reads, d_seq, seq_cap, d_seq_off, d_qual, qual_cap, d_qual_off, d_src,
                               n_reads, seq_bytes, qual_bytes, first_bad, s.st)))
        return rc;
    if (recs) {
        s.down(recs, d_recs, *n_reads);
        s.down(seq, d_seq, *seq_bytes);
        s.down(qual, d_qual, *qual_bytes);
        s.down(seq_off, d_seq_off, *n_reads + 1);
        s.down(qual_off, d_qual_off, *n_reads + 1);
        if (src) s.down(src, d_src, *n_reads);
    }
    return s.sync();
}

extern "C" int bg_bam_sort_keys_dev(bg_ctx* ctx, uint64_t n_records, const uint8_t* d_bam, const uint64_t* d_off, const bg_sam_contig_t* d_contigs,
                                    uint64_t n_contigs, uint64_t* d_key, uint64_t* first_bad, void* stream) {
    if (first_bad) *first_bad = UINT64_MAX;
    if (!ctx || (n_records && (!d_bam || !d_off || !d_key)) || (n_contigs && !d_contigs)) return BG_ERR_INVALID_ARG;
    if (n_records >= 0xFFFFFFFFull) return BG_ERR_TOO_LARGE;
    if (!n_records) return BG_OK;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);
    int rc = bg_reserve(&ctx->aux, &ctx->aux_bytes, sizeof(read_result_t));
    if (rc) return rc;
    read_result_t* d_res = (read_result_t*)ctx->aux;
    const ReadArgs a = {n_records, d_bam, d_off, n_contigs, bg_bam_reads_t{}};
    BG_HIP(hipMemsetAsync(d_res, 0xFF, 8, st));
    read_keys_kernel<<<lanes(n_records), dim3(256), 0, st>>>(a, d_contigs, d_key, d_res);
    BG_HIP(hipGetLastError());
    unsigned long long bad = 0;
    BG_HIP(hipMemcpyAsync(&bad, d_res, 8, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    if (bad == UINT64_MAX) return BG_OK;
    if (first_bad) *first_bad = bad;
    return bg_refuse(("bg_bam_sort_keys: slot " + std::to_string(bad) + " is no BAM record of this contig table").c_str());
}

extern "C" int bg_bam_sort_keys(bg_ctx* ctx, uint64_t n_records, const uint8_t* bam, const uint64_t* off, const bg_sam_contig_t* contigs,
                                uint64_t n_contigs, uint64_t* key, uint64_t* first_bad) {
    if (first_bad) *first_bad = UINT64_MAX;
    if (!ctx || (n_records && (!bam || !off || !key)) || (n_contigs && !contigs)) return BG_ERR_INVALID_ARG;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_bam = s.up(bam, n_records ? off[n_records] : 0);
    const uint64_t* d_off = s.up(off, n_records ? n_records + 1 : 0);
    const bg_sam_contig_t* d_contigs = s.up(contigs, n_contigs);
    uint64_t* d_key = s.out<uint64_t>(n_records);
    if (s.rc) return s.rc;
    int rc = bg_bam_sort_keys_dev(ctx, n_records, d_bam, d_off, d_contigs, n_contigs, d_key, first_bad, s.st);
    if (rc) return rc;
    s.down(key, d_key, n_records);
    return s.sync();
}
