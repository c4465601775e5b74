// The text forms of an alignment, for a batch of alignment records: bio-types 1.0 Alignment::cigar(hard_clip)
// (bg_cigar_batch[_dev]) and Alignment::pretty(x, y, ncol) (bg_pretty_batch).  One thread per alignment in both.
#include <algorithm>
#include <vector>

#include "bg_common.h"

namespace {

__device__ __forceinline__ uint32_t put_num(char* o, uint32_t v) {
    char tmp[10];
    uint32_t n = 0;
    do {
        tmp[n++] = (char)('0' + v % 10);
        v /= 10;
    } while (v);
    for (uint32_t i = 0; i < n; i++) o[i] = tmp[n - 1 - i];
    return n;
}
// one thread per alignment; out slot of `stride` chars per alignment, len[p] = chars written or a negative status
__global__ __launch_bounds__(256) void cigar_kernel(const bg_alignment_t* __restrict__ aln, const uint8_t* __restrict__ ops, uint64_t n, int hard_clip,
                                                    char* __restrict__ out, uint64_t stride, int32_t* __restrict__ len) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const bg_alignment_t a = aln[p];
    if (a.mode == BG_MODE_CUSTOM) {  // bio-types: "Cigar fn not supported for custom alignment mode" (panic)
        len[p] = BG_ERR_UNSUPPORTED;
        return;
    }
    char* o = out + p * stride;
    uint64_t w = 0;
    const char clip = hard_clip ? 'H' : 'S';
    bool overflow = false;
    auto emit = [&](uint32_t k, char c) {
        if (w + 11 > stride) {
            overflow = true;
            return;
        }
        w += put_num(o + w, k);
        o[w++] = c;
    };
    auto add = [&](uint32_t kind, uint32_t k) {
        if (kind == BG_OP_MATCH) emit(k, '=');
        else if (kind == BG_OP_SUBST) emit(k, 'X');
        else if (kind == BG_OP_DEL) emit(k, 'D');
        else if (kind == BG_OP_INS) emit(k, 'I');
    };
    if (a.n_ops) {
        const uint8_t* q = ops + a.ops_off;
        uint32_t last = q[0], k = 1;
        if (a.xstart > 0) emit(a.xstart, clip);
        for (uint32_t i = 1; i < a.n_ops; i++) {
            const uint32_t op = q[i];
            if (op == last) {
                k++;
            } else {
                add(last, k);
                k = 1;
            }
            last = op;
        }
        add(last, k);
        if (a.xlen > a.xend) emit(a.xlen - a.xend, clip);
    }
    len[p] = overflow ? BG_ERR_OPS_CAP : (int32_t)w;
}

// Alignment::pretty(x, y, ncol) (bio-types): three rows — x, the operation marks ('|' match, '\\' mismatch, '+' insertion,
// 'x' deletion, ' ' clipped), y — cut into blocks of ncol columns, every block "x row\n marks\n y row\n\n\n".  The standard
// modes print the clipped prefixes / suffixes of x and y around the operations, AlignmentMode::Custom walks its
// Xclip / Yclip operations instead (the crate prints the FIRST len symbols of the sequence for a clip operation,
// wherever the clip sits: reproduced).  One thread per alignment; two passes over the operations (length, then text).
__global__ __launch_bounds__(256) void pretty_kernel(const bg_alignment_t* __restrict__ aln, const uint8_t* __restrict__ ops, uint64_t n,
                                                     const uint8_t* __restrict__ xs, const uint64_t* __restrict__ x_off,
                                                     const uint8_t* __restrict__ ys, const uint64_t* __restrict__ y_off, uint32_t ncol,
                                                     char* __restrict__ out, uint64_t stride, int64_t* __restrict__ len) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const bg_alignment_t a = aln[p];
    const uint8_t* x = xs + x_off[p];
    const uint8_t* y = ys + y_off[p];
    const uint64_t xl = x_off[p + 1] - x_off[p], yl = y_off[p + 1] - y_off[p];
    char* o = out + p * stride;
    bool bad = xl != a.xlen || yl != a.ylen;  // not the sequences this alignment was computed from
    uint64_t ml = 0;
    for (int pass = 0; pass < 2 && !bad; pass++) {
        uint64_t col = 0;
        auto put = [&](uint8_t cx, char ci, uint8_t cy) {
            if (pass == 1) {
                const uint64_t blk = col / ncol, w = col - blk * ncol;
                const uint64_t bl = min((uint64_t)ncol, ml - blk * ncol);
                char* b = o + blk * (3ull * ncol + 5);
                b[w] = (char)cx;
                b[bl + 1 + w] = ci;
                b[2 * (bl + 1) + w] = (char)cy;
            }
            bad = bad || cx >= 0x80 || cy >= 0x80;  // from_utf8_lossy widens such a byte: the crate's length assert fires
            col++;
        };
        if (a.n_ops) {
            uint64_t xi = 0, yi = 0;
            const uint8_t* q = ops + a.ops_off;
            uint32_t clip = 0;
            if (a.mode != BG_MODE_CUSTOM) {
                xi = a.xstart;
                yi = a.ystart;
                for (uint64_t k = 0; k < a.xstart && k < xl; k++) put(x[k], ' ', ' ');
                for (uint64_t k = 0; k < a.ystart && k < yl; k++) put(' ', ' ', y[k]);
            }
            for (uint32_t i = 0; i < a.n_ops && !bad; i++) {
                const uint32_t op = q[i];
                if (op == BG_OP_MATCH || op == BG_OP_SUBST) {
                    if (xi >= xl || yi >= yl) { bad = true; break; }
                    put(x[xi++], op == BG_OP_MATCH ? '|' : '\\', y[yi++]);
                } else if (op == BG_OP_DEL) {
                    if (yi >= yl) { bad = true; break; }
                    put('-', 'x', y[yi++]);
                } else if (op == BG_OP_INS) {
                    if (xi >= xl) { bad = true; break; }
                    put(x[xi++], '+', '-');
                } else {
                    const uint32_t cl = clip < 4 ? a.clip_len[clip] : 0;
                    clip++;
                    if (op == BG_OP_XCLIP) {
                        for (uint64_t k = 0; k < cl && k < xl; k++, xi++) put(x[k], ' ', ' ');
                    } else {
                        for (uint64_t k = 0; k < cl && k < yl; k++, yi++) put(' ', ' ', y[k]);
                    }
                }
            }
            if (a.mode != BG_MODE_CUSTOM) {
                for (uint64_t k = xi; k < xl; k++) put(x[k], ' ', ' ');
                for (uint64_t k = yi; k < yl; k++) put(' ', ' ', y[k]);
            }
        }
        if (pass == 0) {
            ml = col;
            const uint64_t nb = (ml + ncol - 1) / ncol;
            if (3 * ml + 5 * nb > stride) {
                len[p] = BG_ERR_OPS_CAP;
                return;
            }
        }
    }
    if (bad) {
        len[p] = BG_ERR_UNSUPPORTED;
        return;
    }
    const uint64_t nb = (ml + ncol - 1) / ncol;
    for (uint64_t blk = 0; blk < nb; blk++) {
        const uint64_t bl = min((uint64_t)ncol, ml - blk * ncol);
        char* b = o + blk * (3ull * ncol + 5);
        b[bl] = b[2 * bl + 1] = b[3 * bl + 2] = b[3 * bl + 3] = b[3 * bl + 4] = '\n';
    }
    len[p] = (int64_t)(3 * ml + 5 * nb);
}

}  // namespace

extern "C" int bg_cigar_batch_dev(bg_ctx* ctx, uint64_t n, const bg_alignment_t* d_aln, const uint8_t* d_ops, int hard_clip, char* d_out,
                                  uint64_t stride, int32_t* d_len, void* stream) {
    if (!ctx) return BG_ERR_INVALID_ARG;
    if (n == 0) return BG_OK;
    if (!d_aln || !d_out || !d_len || stride < 24) return BG_ERR_INVALID_ARG;
    BG_HIP(hipSetDevice(ctx->device));
    cigar_kernel<<<dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(d_aln, d_ops, n, hard_clip, d_out, stride, d_len);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

extern "C" int bg_pretty_batch(bg_ctx* ctx, uint64_t n, const bg_alignment_t* aln, const uint8_t* ops, uint64_t ops_bytes, const uint8_t* x,
                               const uint64_t* x_off, const uint8_t* y, const uint64_t* y_off, uint32_t ncol, char* out, uint64_t out_cap,
                               uint64_t* out_off) {
    if (!ctx || !out_off || ncol == 0) return BG_ERR_INVALID_ARG;
    out_off[0] = 0;
    if (n == 0) return BG_OK;
    if (!aln || (!ops && ops_bytes) || !x_off || !y_off || !out) return BG_ERR_INVALID_ARG;
    uint64_t max_ml = 0;
    for (uint64_t p = 0; p < n; p++) {
        if (aln[p].n_ops && aln[p].ops_off + aln[p].n_ops > ops_bytes) return BG_ERR_INVALID_ARG;
        max_ml = std::max<uint64_t>(max_ml, (x_off[p + 1] - x_off[p]) + (y_off[p + 1] - y_off[p]));
    }
    const uint64_t stride = (3 * max_ml + 5 * ((max_ml + ncol - 1) / ncol) + 15) & ~15ull;
    std::vector<char> h((size_t)(n * stride));
    std::vector<int64_t> hl(n);
    {
        bg_stage s(ctx, ctx->stream);
        const bg_alignment_t* d_aln = s.up(aln, n);
        const uint8_t* d_ops = s.up(ops, ops_bytes);
        const uint8_t* d_x = s.up(x, x_off[n]);
        const uint64_t* d_x_off = s.up(x_off, n + 1);
        const uint8_t* d_y = s.up(y, y_off[n]);
        const uint64_t* d_y_off = s.up(y_off, n + 1);
        char* d_text = s.out<char>(n * stride);
        int64_t* d_len = s.out<int64_t>(n);
        if (s.rc) return s.rc;
        pretty_kernel<<<dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s.st>>>(d_aln, d_ops, n, d_x, d_x_off, d_y, d_y_off, ncol, d_text, stride,
                                                                                d_len);
        BG_HIP(hipGetLastError());
        s.down(h.data(), d_text, n * stride);
        s.down(hl.data(), d_len, n);
        if (s.sync()) return s.rc;
    }
    uint64_t used = 0;
    int status = BG_OK;
    for (uint64_t p = 0; p < n; p++) {
        if (hl[p] < 0) {
            status = (int)hl[p];
            out_off[p + 1] = used;
            continue;
        }
        if (used + (uint64_t)hl[p] > out_cap) return BG_ERR_OPS_CAP;
        memcpy(out + used, h.data() + p * stride, (size_t)hl[p]);
        used += (uint64_t)hl[p];
        out_off[p + 1] = used;
    }
    return status;
}

extern "C" int bg_cigar_batch(bg_ctx* ctx, uint64_t n, const bg_alignment_t* aln, const uint8_t* ops, uint64_t ops_bytes, int hard_clip, char* out,
                              uint64_t out_cap, uint64_t* out_off) {
    if (!ctx || !out_off) return BG_ERR_INVALID_ARG;
    out_off[0] = 0;
    if (n == 0) return BG_OK;
    if (!aln || (!ops && ops_bytes) || !out) return BG_ERR_INVALID_ARG;
    BG_HIP(hipSetDevice(ctx->device));
    uint32_t max_ops = 0;
    for (uint64_t p = 0; p < n; p++) {
        if (aln[p].n_ops && aln[p].ops_off + aln[p].n_ops > ops_bytes) return BG_ERR_INVALID_ARG;
        max_ops = std::max(max_ops, aln[p].n_ops);
    }
    const uint64_t stride = ((uint64_t)max_ops * 2 + 24 + 11 + 15) & ~15ull;  // every run is at least "1=": two chars per op, + two clips
    int rc;
    const size_t need[4] = {n * sizeof(bg_alignment_t), std::max<uint64_t>(ops_bytes, 16), n * stride, n * 4};
    for (int i = 0; i < 4; i++)
        if ((rc = bg_reserve(&ctx->io[i], &ctx->io_cap[i], need[i]))) return rc;
    hipStream_t st = ctx->stream;
    BG_HIP(hipMemcpyAsync(ctx->io[0], aln, need[0], hipMemcpyHostToDevice, st));
    if (ops_bytes) BG_HIP(hipMemcpyAsync(ctx->io[1], ops, ops_bytes, hipMemcpyHostToDevice, st));
    rc = bg_cigar_batch_dev(ctx, n, (const bg_alignment_t*)ctx->io[0], (const uint8_t*)ctx->io[1], hard_clip, (char*)ctx->io[2], stride,
                            (int32_t*)ctx->io[3], st);
    if (rc) return rc;
    std::vector<char> h((size_t)(n * stride));
    std::vector<int32_t> hl(n);
    BG_HIP(hipMemcpyAsync(h.data(), ctx->io[2], n * stride, hipMemcpyDeviceToHost, st));
    BG_HIP(hipMemcpyAsync(hl.data(), ctx->io[3], n * 4, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    uint64_t used = 0;
    int status = BG_OK;
    for (uint64_t p = 0; p < n; p++) {
        if (hl[p] < 0) {
            status = hl[p];  // BG_ERR_UNSUPPORTED: AlignmentMode::Custom (the reference panics)
            out_off[p + 1] = used;
            continue;
        }
        if (used + (uint64_t)hl[p] > out_cap) return BG_ERR_OPS_CAP;
        memcpy(out + used, h.data() + p * stride, (size_t)hl[p]);
        used += (uint64_t)hl[p];
        out_off[p + 1] = used;
    }
    return status;
}
