// Reading BGZF on the device (bg_bgzf_blocks[_dev], bg_bgzf_inflate[_dev]; the rules are in include/biogpu.h, the bodies in
// bgzf_inflate_rule.h).
//
// The block table.  The chain of members is serial by nature (a member's start is known from its predecessor's BSIZE); no
// lane walks it.  Candidates: every position at which a complete accepted member stands (bgzf_member_verdict), counted per
// chunk of 2048 positions, the counts scanned (scan.hip), the positions compacted in ascending order.  Two candidates lie
// at least 16 bytes apart, and that rests on the WHOLE verdict, not on the 16 signature bytes: for a second header k bytes
// behind the first, k = 1 .. 5 and 7 .. 15 put one of its fixed bytes on a different fixed byte of the first, but k = 6 is
// consistent with every fixed byte (its bytes 0 .. 3 fall on MTIME / XFL / OS, its XLEN on the first's BSIZE) and is excluded
// only because it forces the first's BSIZE to 0x0006, which bgzf_member_verdict refuses (28 <= BSIZE + 1).  Whoever loosens
// the verdict (flags on the signature alone, say) breaks what rests on it: in_bytes / 16 + 1 slots hold all candidates (the
// scratch bound and blk_cand_kernel's guard on it), and a thread's 8 positions hold at most one (it keeps one).  A candidate's successor is the candidate at its position + BSIZE + 1, found by
// binary search in the compacted positions.  Membership of the chain from candidate 0 is marked by doubling: in round k every
// marked candidate marks its 2^k-th successor, then the jump table is squared into its other copy; ceil(log2(in_bytes / 28
// + 1)) rounds mark the longest chain the input can hold.  The marked candidates are counted and their ISIZE summed per chunk
// of 2048 candidates, both scanned, and a last pass writes block_off and out_off.  One thread looks at the chain's end: the
// marked candidate without a successor must end at in_bytes; otherwise the verdict on what stands there is the error.
// Fakes inside payloads are candidates like any other and simply never get marked.
//
// The payloads.  One wavefront a block (a workgroup of 64 lanes): Huffman decoding is serial inside a deflate stream, so the
// parallelism is across blocks, and inside a block in the tables, the copies and the CRC (bgzf_inflate_rule.h).  LDS holds
// the tables, the token queue and the CRC's slicing table, 8.5 KB a workgroup, not the payload: output goes straight to its
// place in d_out and match copies read it back from there (L2).  __syncthreads() between a batch's stores and the loads of
// a later match is the workgroup-scope fence plus the wait on the store counter; the workgroup's lanes share one CU's L1.
#include "bg_common.h"
#include "bgzf_inflate_rule.h"

namespace {

constexpr uint32_t BLK_CHUNK = 2048;  // positions (candidates) a workgroup of 256 takes: 8 consecutive ones a thread
struct blk_result_t {
    uint64_t err, n_blocks, out_bytes, first_bad, tail;
};

// exclusive prefix of v over the 256 threads of the workgroup; *total: the sum
__device__ uint32_t blk_scan256(uint32_t v, uint32_t* s /* [256] */, uint32_t* total) {
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

// chunk c: WRITE false: cnt[c] = its candidates; WRITE true: their positions to pos[base[c] ..)
template <bool WRITE>
__global__ __launch_bounds__(256) void blk_cand_kernel(const uint8_t* __restrict__ in, uint64_t in_bytes, uint32_t* __restrict__ cnt,
                                                       const uint64_t* __restrict__ base, uint64_t* __restrict__ pos, uint64_t cap) {
    __shared__ uint32_t s[256];
    const uint64_t p0 = (uint64_t)blockIdx.x * BLK_CHUNK + 8ull * threadIdx.x;
    uint64_t mine = 0;
    uint32_t have = 0, size, isize;
    for (uint32_t i = 0; i < 8; i++)
        if (p0 + i < in_bytes && bgzf_member_verdict(in, in_bytes, p0 + i, &size, &isize) == BG_OK) {
            mine = p0 + i;
            have = 1;
        }
    uint32_t total;
    const uint32_t before = blk_scan256(have, s, &total);
    if (!WRITE) {
        if (threadIdx.x == 0) cnt[blockIdx.x] = total;
    } else if (have && base[blockIdx.x] + before < cap) {  // (always: candidates lie 16 bytes apart)
        pos[base[blockIdx.x] + before] = mine;
    }
}

// candidate i: its successor (INF_NONE: none, then it is a tail), the chain's first mark
__global__ __launch_bounds__(256) void blk_succ_kernel(const uint8_t* __restrict__ in, uint64_t in_bytes, const uint64_t* __restrict__ n_cand,
                                                       const uint64_t* __restrict__ pos, uint32_t* __restrict__ jump, uint8_t* __restrict__ chain,
                                                       uint8_t* __restrict__ tail) {
    const uint64_t n = *n_cand;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint64_t target = pos[i] + bgzf_le16(in + pos[i] + 16) + 1;
        uint64_t lo = i + 1, hi = n;  // the first candidate at or behind target
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (pos[mid] < target) lo = mid + 1;
            else hi = mid;
        }
        const bool found = lo < n && pos[lo] == target;
        jump[i] = found ? (uint32_t)lo : INF_NONE;
        tail[i] = !found;
        chain[i] = i == 0 && pos[0] == 0;
    }
}
__global__ __launch_bounds__(256) void blk_double_kernel(const uint64_t* __restrict__ n_cand, const uint32_t* __restrict__ jin,
                                                         uint32_t* __restrict__ jout, uint8_t* chain) {
    const uint64_t n = *n_cand;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t j = jin[i];
        if (j == INF_NONE) {
            jout[i] = INF_NONE;
            continue;
        }
        if (chain[i]) chain[j] = 1;  // (a mark set in this round may already mark on: it marks members only)
        jout[i] = jin[j];
    }
}

__device__ uint32_t blk_isize(const uint8_t* in, uint64_t p) { return bgzf_le32(in + p + bgzf_le16(in + p + 16) + 1 - 4); }

// chunk c of the candidates: WRITE false: cnt_m[c] = its members, cnt_s[c] = their ISIZE sum, and the chain's tail is noted;
// WRITE true (no error, tables given): the members' rows of block_off and out_off, and the closing row
template <bool WRITE>
__global__ __launch_bounds__(256) void blk_rows_kernel(const uint8_t* __restrict__ in, uint64_t in_bytes, const uint64_t* __restrict__ n_cand,
                                                       const uint64_t* __restrict__ pos, const uint8_t* __restrict__ chain,
                                                       const uint8_t* __restrict__ tail, uint32_t* __restrict__ cnt_m, uint32_t* __restrict__ cnt_s,
                                                       const uint64_t* __restrict__ base_m, const uint64_t* __restrict__ base_s,
                                                       blk_result_t* __restrict__ res, uint64_t* __restrict__ block_off,
                                                       uint64_t* __restrict__ out_off) {
    __shared__ uint32_t s[256];
    if (WRITE && res->err) return;
    const uint64_t n = *n_cand, i0 = (uint64_t)blockIdx.x * BLK_CHUNK + 8ull * threadIdx.x;
    uint32_t m = 0, bytes = 0;
    for (uint32_t k = 0; k < 8; k++)
        if (i0 + k < n && chain[i0 + k]) {
            m++;
            bytes += blk_isize(in, pos[i0 + k]);
            if (!WRITE && tail[i0 + k]) res->tail = i0 + k;  // the one member without a successor
        }
    uint32_t total_m, total_s;
    const uint32_t before_m = blk_scan256(m, s, &total_m), before_s = blk_scan256(bytes, s, &total_s);
    if (!WRITE) {
        if (threadIdx.x == 0) {
            cnt_m[blockIdx.x] = total_m;
            cnt_s[blockIdx.x] = total_s;
        }
        return;
    }
    uint64_t row = base_m[blockIdx.x] + before_m, at = base_s[blockIdx.x] + before_s;
    for (uint32_t k = 0; k < 8; k++)
        if (i0 + k < n && chain[i0 + k]) {
            block_off[row] = pos[i0 + k];
            out_off[row++] = at;
            at += blk_isize(in, pos[i0 + k]);
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        block_off[res->n_blocks] = in_bytes;
        out_off[res->n_blocks] = res->out_bytes;
    }
}
// one thread: the totals, where the chain ends, the error
__global__ void blk_finish_kernel(const uint8_t* __restrict__ in, uint64_t in_bytes, const uint64_t* __restrict__ pos,
                                  const uint64_t* __restrict__ total_m, const uint64_t* __restrict__ total_s, uint64_t cap_blocks, uint32_t tables,
                                  blk_result_t* __restrict__ res) {
    res->n_blocks = *total_m;
    res->out_bytes = *total_s;
    res->first_bad = UINT64_MAX;
    res->err = BG_OK;
    const uint64_t end = res->tail == UINT64_MAX ? 0 : pos[res->tail] + bgzf_le16(in + pos[res->tail] + 16) + 1;
    if (end != in_bytes) {
        uint32_t size, isize;
        const int v = bgzf_member_verdict(in, in_bytes, end, &size, &isize);
        res->err = (uint64_t)(int64_t)(v ? v : BG_ERR_INVALID_ARG);
        res->first_bad = *total_m;
    } else if (tables && *total_m > cap_blocks) {
        res->err = (uint64_t)(int64_t)BG_ERR_OPS_CAP;
    }
}

uint32_t blk_rounds(uint64_t in_bytes) {
    uint32_t r = 0;
    while ((1ull << r) < in_bytes / BGZF_MIN_MEMBER + 1) r++;
    return r;
}

// ---- the payloads ---------------------------------------------------------------------------------------------------------
struct inf_result_t {
    uint64_t bad_table, no_room, first_bad;  // each UINT64_MAX until something is found
};
__global__ __launch_bounds__(256) void inf_check_kernel(uint64_t in_bytes, uint64_t n_blocks, const uint64_t* __restrict__ block_off,
                                                        const uint64_t* __restrict__ out_off, uint64_t out_cap, inf_result_t* __restrict__ res) {
    for (uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x; b < n_blocks; b += (uint64_t)gridDim.x * 256) {
        const uint64_t m0 = block_off[b], m1 = block_off[b + 1], o0 = out_off[b], o1 = out_off[b + 1];
        if (m1 < m0 || m1 - m0 < BGZF_MIN_MEMBER || m1 - m0 > 65536 || m1 > in_bytes || o1 < o0 || o1 - o0 > BGZF_MAX_ISIZE) atomicMin((unsigned long long*)&res->bad_table, (unsigned long long)b);
        else if (o1 > out_cap) atomicMin((unsigned long long*)&res->no_room, (unsigned long long)b);
    }
}
// (37 VGPRs, 78 SGPRs, 8 600 bytes of LDS: the LDS admits 19 workgroups a CU, 5 waves a SIMD)
__global__ __launch_bounds__(INF_LANES) void bgzf_inflate_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ block_off,
                                                                   const uint64_t* __restrict__ out_off, uint8_t* out, uint8_t* __restrict__ status,
                                                                   inf_result_t* __restrict__ res) {
    __shared__ uint16_t s_lit[1u << INF_LROOT], s_dst[1u << INF_DROOT], s_sorted[INF_NLIT + INF_NDIST], s_meta[96];
    __shared__ uint8_t s_lens[INF_NLIT + INF_NDIST], s_clens[INF_NCODE + 1];
    __shared__ uint32_t s_q[2 * INF_QUEUE], s_T[1024], s_part[INF_LANES], s_word[1];
    if (res->bad_table != UINT64_MAX || res->no_room != UINT64_MAX) return;  // nothing is written
    const uint64_t b = blockIdx.x;
    const inf_ws_t w = {s_lit, s_dst, s_sorted, s_meta, s_lens, s_clens, s_q, s_T, s_part, s_word};
    const uint64_t m0 = block_off[b], o0 = out_off[b];
    const uint32_t st = inf_block(w, in + m0, (uint32_t)(block_off[b + 1] - m0), out + o0, (uint32_t)(out_off[b + 1] - o0));
    if (threadIdx.x == 0) {
        if (status) status[b] = (uint8_t)st;
        if (st) atomicMin((unsigned long long*)&res->first_bad, (unsigned long long)b);
    }
}

int blocks_args(const bg_ctx* ctx, const void* in, uint64_t in_bytes, const void* block_off, const void* out_off, uint64_t cap_blocks,
                const uint64_t* n_blocks, const uint64_t* out_bytes) {
    if (!ctx || !n_blocks || !out_bytes || (in_bytes && !in) || (!block_off != !out_off) || (!block_off && cap_blocks)) return BG_ERR_INVALID_ARG;
    return in_bytes >> 35 ? BG_ERR_TOO_LARGE : BG_OK;
}
// (a null out with out_cap == 0 is legal: a file of empty members has nothing to write, and any range that wants a byte is then
// BG_ERR_OPS_CAP by the check kernel)
int inflate_args(const bg_ctx* ctx, const void* in, uint64_t n_blocks, const void* block_off, const void* out_off, const void* out, uint64_t out_cap) {
    if (!ctx || (n_blocks && (!in || !block_off || !out_off || (!out && out_cap)))) return BG_ERR_INVALID_ARG;
    return n_blocks >> 31 ? BG_ERR_TOO_LARGE : BG_OK;
}
// bg_bgzf_inflate_dev; *wrote: whether the kernel ran over the blocks (false: nothing was written)
int inflate_dev(bg_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes, uint64_t n_blocks, const uint64_t* d_block_off, const uint64_t* d_out_off,
                uint8_t* d_out, uint64_t out_cap, uint8_t* d_status, uint64_t* first_bad, hipStream_t st, bool* wrote) {
    *wrote = false;
    if (first_bad) *first_bad = UINT64_MAX;
    int rc = inflate_args(ctx, d_in, n_blocks, d_block_off, d_out_off, d_out, out_cap);
    if (rc || !n_blocks) return rc;
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);
    if ((rc = bg_reserve(&ctx->aux, &ctx->aux_bytes, sizeof(inf_result_t)))) return rc;
    inf_result_t* d_res = (inf_result_t*)ctx->aux;
    BG_HIP(hipMemsetAsync(d_res, 0xFF, sizeof(inf_result_t), st));
    const uint32_t grid = (uint32_t)((n_blocks + 255) / 256 < 2048 ? (n_blocks + 255) / 256 : 2048);
    inf_check_kernel<<<dim3(grid), dim3(256), 0, st>>>(in_bytes, n_blocks, d_block_off, d_out_off, out_cap, d_res);
    bgzf_inflate_kernel<<<dim3((uint32_t)n_blocks), dim3(INF_LANES), 0, st>>>(d_in, d_block_off, d_out_off, d_out, d_status, d_res);
    BG_HIP(hipGetLastError());
    inf_result_t r;
    BG_HIP(hipMemcpyAsync(&r, d_res, sizeof r, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    if (r.bad_table != UINT64_MAX) {
        if (first_bad) *first_bad = r.bad_table;
        return bg_refuse("bg_bgzf_inflate: the tables are not ascending, leave the input, or hold a member outside 28 .. 65 536 bytes or a payload above 65 536");
    }
    if (r.no_room != UINT64_MAX) return BG_ERR_OPS_CAP;
    *wrote = true;
    if (r.first_bad == UINT64_MAX) return BG_OK;
    if (first_bad) *first_bad = r.first_bad;
    return bg_refuse("bg_bgzf_inflate: a block does not inflate to its payload (status, first_bad)");
}

}  // namespace

extern "C" int bg_bgzf_blocks_dev(bg_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes, uint64_t* d_block_off, uint64_t* d_out_off,
                                  uint64_t cap_blocks, uint64_t* n_blocks, uint64_t* out_bytes, uint64_t* first_bad, void* stream) {
    int rc = blocks_args(ctx, d_in, in_bytes, d_block_off, d_out_off, cap_blocks, n_blocks, out_bytes);
    if (rc) return rc;
    *n_blocks = *out_bytes = 0;
    if (first_bad) *first_bad = UINT64_MAX;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    if (!in_bytes) {  // no block: the closing row alone
        if (d_block_off) {
            BG_HIP(hipMemsetAsync(d_block_off, 0, 8, st));
            BG_HIP(hipMemsetAsync(d_out_off, 0, 8, st));
        }
        return BG_OK;
    }
    bg_scratch_guard guard(ctx, st);
    const uint64_t n_chunks = (in_bytes + BLK_CHUNK - 1) / BLK_CHUNK, cap = in_bytes / 16 + 1, c_chunks = (cap + BLK_CHUNK - 1) / BLK_CHUNK;
    uint64_t *d_pos, *d_off1, *d_offm, *d_offs, *d_sums;
    blk_result_t* d_res;
    uint32_t *d_jumps, *d_cnt1, *d_cntm, *d_cnts;
    uint8_t *d_chain, *d_tail;
    if ((rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_pos = cv.take<uint64_t>(cap), d_off1 = cv.take<uint64_t>(n_chunks + 1);
        d_offm = cv.take<uint64_t>(c_chunks + 1), d_offs = cv.take<uint64_t>(c_chunks + 1);
        d_sums = cv.take<uint64_t>(bg_scan_sums_words(n_chunks > c_chunks ? n_chunks : c_chunks));
        d_res = cv.take<blk_result_t>(1);
        d_jumps = cv.take<uint32_t>(2 * cap);  // one piece: the two halves the doubling rounds swap
        d_cnt1 = cv.take<uint32_t>(n_chunks), d_cntm = cv.take<uint32_t>(c_chunks), d_cnts = cv.take<uint32_t>(c_chunks);
        d_chain = cv.take<uint8_t>(cap), d_tail = cv.take<uint8_t>(cap);
    }))) return rc;
    uint32_t* d_jump[2] = {d_jumps, d_jumps + cap};
    const uint64_t* d_ncand = d_off1 + n_chunks;
    const uint32_t tables = d_block_off ? 1u : 0u;
    const uint32_t grid = (uint32_t)((cap + 255) / 256 < 2048 ? (cap + 255) / 256 : 2048);

    BG_HIP(hipMemsetAsync(d_res, 0xFF, sizeof(blk_result_t), st));
    blk_cand_kernel<false><<<dim3((uint32_t)n_chunks), dim3(256), 0, st>>>(d_in, in_bytes, d_cnt1, nullptr, nullptr, cap);
    if ((rc = bg_scan_u32(d_cnt1, n_chunks, d_off1, d_sums, st))) return rc;
    blk_cand_kernel<true><<<dim3((uint32_t)n_chunks), dim3(256), 0, st>>>(d_in, in_bytes, nullptr, d_off1, d_pos, cap);
    blk_succ_kernel<<<dim3(grid), dim3(256), 0, st>>>(d_in, in_bytes, d_ncand, d_pos, d_jump[0], d_chain, d_tail);
    const uint32_t rounds = blk_rounds(in_bytes);
    for (uint32_t k = 0; k < rounds; k++) blk_double_kernel<<<dim3(grid), dim3(256), 0, st>>>(d_ncand, d_jump[k & 1], d_jump[(k + 1) & 1], d_chain);
    blk_rows_kernel<false><<<dim3((uint32_t)c_chunks), dim3(256), 0, st>>>(d_in, in_bytes, d_ncand, d_pos, d_chain, d_tail, d_cntm, d_cnts, nullptr,
                                                                          nullptr, d_res, nullptr, nullptr);
    if ((rc = bg_scan_u32(d_cntm, c_chunks, d_offm, d_sums, st))) return rc;
    if ((rc = bg_scan_u32(d_cnts, c_chunks, d_offs, d_sums, st))) return rc;
    blk_finish_kernel<<<dim3(1), dim3(1), 0, st>>>(d_in, in_bytes, d_pos, d_offm + c_chunks, d_offs + c_chunks, cap_blocks, tables, d_res);
    if (tables)
        blk_rows_kernel<true><<<dim3((uint32_t)c_chunks), dim3(256), 0, st>>>(d_in, in_bytes, d_ncand, d_pos, d_chain, d_tail, nullptr, nullptr, d_offm,
                                                                             d_offs, d_res, d_block_off, d_out_off);
    BG_HIP(hipGetLastError());
    blk_result_t r;
    BG_HIP(hipMemcpyAsync(&r, d_res, sizeof r, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    *n_blocks = r.n_blocks;
    *out_bytes = r.out_bytes;
    if (first_bad) *first_bad = r.first_bad;
    rc = (int)(int64_t)r.err;
    if (rc == BG_ERR_INVALID_ARG) return bg_refuse("bg_bgzf_blocks: no BGZF member where the chain arrives (first_bad), or one that leaves the input");
    if (rc == BG_ERR_UNSUPPORTED) return bg_refuse("bg_bgzf_blocks: a gzip member that is not BGZF (FLG, XLEN or the subfield)", rc);
    return rc;
}

extern "C" int bg_bgzf_blocks(bg_ctx* ctx, const uint8_t* in, uint64_t in_bytes, uint64_t* block_off, uint64_t* out_off, uint64_t cap_blocks,
                              uint64_t* n_blocks, uint64_t* out_bytes, uint64_t* first_bad) {
    int rc = blocks_args(ctx, in, in_bytes, block_off, out_off, cap_blocks, n_blocks, out_bytes);
    if (rc) return rc;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_in = s.up(in, in_bytes);
    uint64_t* d_block_off = block_off ? s.out<uint64_t>(cap_blocks + 1) : nullptr;
    uint64_t* d_out_off = block_off ? s.out<uint64_t>(cap_blocks + 1) : nullptr;
    if (s.rc) return s.rc;
    if ((rc = bg_bgzf_blocks_dev(ctx, d_in, in_bytes, d_block_off, d_out_off, cap_blocks, n_blocks, out_bytes, first_bad, s.st))) return rc;
    if (block_off) {
        s.down(block_off, d_block_off, *n_blocks + 1);
        s.down(out_off, d_out_off, *n_blocks + 1);
    }
    return s.sync();
}

extern "C" int bg_bgzf_inflate_dev(bg_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes, uint64_t n_blocks, const uint64_t* d_block_off,
                                   const uint64_t* d_out_off, uint8_t* d_out, uint64_t out_cap, uint8_t* d_status, uint64_t* first_bad,
                                   void* stream) {
    bool wrote;
    return inflate_dev(ctx, d_in, in_bytes, n_blocks, d_block_off, d_out_off, d_out, out_cap, d_status, first_bad, (hipStream_t)stream, &wrote);
}

extern "C" int bg_bgzf_inflate(bg_ctx* ctx, const uint8_t* in, uint64_t in_bytes, uint64_t n_blocks, const uint64_t* block_off,
                               const uint64_t* out_off, uint8_t* out, uint64_t out_cap, uint8_t* status, uint64_t* first_bad) {
    if (first_bad) *first_bad = UINT64_MAX;
    int rc = inflate_args(ctx, in, n_blocks, block_off, out_off, out, out_cap);
    if (rc || !n_blocks) return rc;
    const uint64_t need = out_off[n_blocks] < out_cap ? out_off[n_blocks] : out_cap;  // (more than out_cap: the device call refuses)
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_in = s.up(in, in_bytes);
    const uint64_t* d_block_off = s.up(block_off, n_blocks + 1);
    const uint64_t* d_out_off = s.up(out_off, n_blocks + 1);
    uint8_t* d_out = s.out<uint8_t>(need);
    uint8_t* d_status = status ? s.out<uint8_t>(n_blocks) : nullptr;
    if (s.rc) return s.rc;
    bool wrote;
    rc = inflate_dev(ctx, d_in, in_bytes, n_blocks, d_block_off, d_out_off, d_out, need, d_status, first_bad, s.st, &wrote);
    if (!wrote) return rc;
    s.down(out + out_off[0], d_out + out_off[0], out_off[n_blocks] - out_off[0]);  // (the tables were found ascending and inside out_cap)
    if (status) s.down(status, d_status, n_blocks);
    const int rs = s.sync();
    return rs ? rs : rc;
}
