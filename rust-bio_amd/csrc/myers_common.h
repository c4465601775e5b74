// What the two Myers variants share (myers.hip: Myers<u64>; myers_long.hip: myers::long, blocks of 64 bits): the walk of a
// lane over its own text, the hit / no-hit records, the compaction of the 256 text bytes into classes, the pinned upload
// of a call's tables, and the host flavour (device copies in through a bg_stage, the device call, results back).
#ifndef BG_MYERS_COMMON_H
#define BG_MYERS_COMMON_H
#include <map>

#include "bg_common.h"

// the last call's tables: pinned on the host (what the device copy was made from) and on the device
struct bg_myers_scratch {
    uint8_t* h = nullptr;  // pinned
    uint8_t* d = nullptr;
    size_t cap = 0, used = 0;
    bool valid = false;
    int kind = 0;  // whose layout the blob has: 0 myers.hip, 1 myers_long.hip
    int* d_flag = nullptr;
};

namespace {

constexpr uint32_t MY_BLOCK = 256;

// a lane's walk over its own text [p, end): bytes to the first 8-byte boundary, aligned words, bytes to the end
struct MyText {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t w;
    uint32_t have;
    __host__ __device__ __forceinline__ MyText(const uint8_t* b, const uint8_t* e) : p(b), end(e), w(0), have(0) {}
    __host__ __device__ __forceinline__ uint32_t next() {  // the caller takes exactly end - p bytes
        if (have == 0) {
            if (((uintptr_t)p & 7) == 0 && end - p >= 8) {
                w = *(const uint64_t*)p;
                have = 8;
                p += 8;
            } else {
                w = *p;
                have = 1;
                p += 1;
            }
        }
        const uint32_t c = (uint32_t)w & 0xFFu;
        w >>= 8;
        have--;
        return c;
    }
};

__host__ __device__ __forceinline__ bg_alignment_t my_no_hit(uint32_t m, uint32_t ylen) {
    bg_alignment_t r = {};
    r.score = BG_MIN_SCORE;
    r.xlen = m;
    r.ylen = ylen;
    r.mode = BG_MODE_SEMIGLOBAL;
    return r;
}
__host__ __device__ __forceinline__ bg_alignment_t my_hit(uint32_t m, uint32_t ylen, uint32_t start, uint32_t end1, uint32_t dist) {
    bg_alignment_t r = {};  // update_aln, helpers.rs:83-99
    r.score = (int32_t)dist;
    r.xend = m;
    r.xlen = m;
    r.ylen = ylen;
    r.yend = end1;
    r.ystart = start;
    r.mode = BG_MODE_SEMIGLOBAL;
    return r;
}
// the record of a best hit with its path of n_ops operations in the job's slot
__host__ __device__ __forceinline__ void my_set_ops(bg_alignment_t& r, uint32_t n_ops, bool broken, const uint8_t* ops, uint64_t ops_stride,
                                                    uint64_t job, int* flag) {
    r.n_ops = n_ops;
    if (broken) r.status = (int8_t)BG_ERR_TRACEBACK;
    if (ops) {
        if (n_ops > ops_stride) {
            r.status = (int8_t)BG_ERR_OPS_CAP;
            r.ops_off = job * ops_stride;
            *flag = 1;
        } else {
            r.ops_off = (job + 1) * ops_stride - n_ops;
        }
    }
}

// bytes into classes: two bytes share one when their words (under each row's mask) agree in every row — a row is a
// pattern's peq (myers.hip) or one 64-symbol block of it (myers_long.hip).  Returns the classes' columns: cols[class][row].
struct MyRow {
    const uint64_t* peq;  // [256]
    uint64_t mask;
};
inline void my_classes(const std::vector<MyRow>& rows, uint8_t cls[256], std::vector<std::vector<uint64_t>>& cols) {
    std::map<std::vector<uint64_t>, uint32_t> seen;
    std::vector<uint64_t> col(rows.size());
    cols.clear();
    for (int c = 0; c < 256; c++) {
        for (size_t r = 0; r < rows.size(); r++) col[r] = rows[r].peq[c] & rows[r].mask;
        auto it = seen.find(col);
        if (it == seen.end()) {
            it = seen.emplace(col, (uint32_t)cols.size()).first;
            cols.push_back(col);
        }
        cls[c] = (uint8_t)it->second;
    }
}

// a call's tables on the device; nothing moves when they are those of the previous call
inline int my_upload(bg_ctx* ctx, const std::vector<uint8_t>& blob, int kind, hipStream_t st) {
    if (!ctx->myers) ctx->myers = new bg_myers_scratch;
    bg_myers_scratch* M = ctx->myers;
    if (!M->d_flag) BG_HIP(hipMalloc(&M->d_flag, sizeof(int)));
    const size_t need = blob.size();
    if (M->valid && M->kind == kind && M->used == need && !memcmp(M->h, blob.data(), need)) return BG_OK;
    // the pinned copy may still be the source of an earlier call's transfer
    BG_HIP(hipStreamSynchronize(st));
    if (ctx->scratch_used && ctx->scratch_stream != st) BG_HIP(hipStreamSynchronize(ctx->scratch_stream));
    M->valid = false;
    if (M->cap < need) {
        if (M->h) hipHostFree(M->h);
        hipFree(M->d);
        M->h = M->d = nullptr;
        M->cap = 0;
        const size_t cap = need + need / 2 + 4096;
        BG_HIP(hipHostMalloc(&M->h, cap));
        BG_HIP(hipMalloc(&M->d, cap));
        M->cap = cap;
    }
    memcpy(M->h, blob.data(), need);
    M->used = need;
    M->kind = kind;
    BG_HIP(hipMemcpyAsync(M->d, M->h, need, hipMemcpyHostToDevice, st));
    M->valid = true;
    return BG_OK;
}

struct MyCall {
    bool find_all = false, ends_only = false;
    uint32_t k = 0, max_hits = 0;
    uint64_t n_texts = 0;
    const uint8_t* d_text = nullptr;
    const uint64_t* d_off = nullptr;
    bg_alignment_t* d_aln = nullptr;
    uint32_t* d_count = nullptr;
    uint8_t* d_ops = nullptr;
    uint64_t ops_stride = 0;
};

// host flavours: device copies of the texts the offsets span (text + off[0] on, with the offsets rebased to it), the device
// call `run(call, stream)` on the ctx's stream, the results back
template <class Run>
int my_host(bg_ctx* ctx, uint32_t n_pat, MyCall c, const uint8_t* text, const uint64_t* off, bg_alignment_t* aln, uint32_t* count,
            uint8_t* ops, Run run) {
    if (c.n_texts == 0) return BG_OK;
    if (!text || !off || !aln) return BG_ERR_INVALID_ARG;
    const uint64_t t0 = off[0];
    const uint64_t n_rec = c.n_texts * n_pat * (c.find_all ? c.max_hits : 1), n_jobs = c.n_texts * n_pat;
    std::vector<uint64_t> rel(c.n_texts + 1);
    for (uint64_t i = 0; i <= c.n_texts; i++) rel[i] = off[i] - t0;
    bg_stage s(ctx, ctx->stream);
    c.d_text = s.up(text + t0, rel.back());
    c.d_off = s.up(rel.data(), rel.size());
    c.d_aln = s.out<bg_alignment_t>(n_rec);
    c.d_count = c.find_all ? s.out<uint32_t>(n_jobs) : nullptr;
    c.d_ops = ops ? s.out<uint8_t>(n_jobs * c.ops_stride) : nullptr;
    if (s.sync()) return s.rc;
    const int rc = run(c, s.st);
    if (rc != BG_OK && rc != BG_ERR_OPS_CAP) return rc;
    s.down(aln, c.d_aln, n_rec);
    if (c.find_all) s.down(count, c.d_count, n_jobs);
    if (ops) s.down(ops, c.d_ops, n_jobs * c.ops_stride);
    return s.sync() ? s.rc : rc;
}

}  // namespace

#endif
