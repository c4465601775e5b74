// BGZF blocks with deflate-compressed payloads (bg_bgzf_deflate[_dev]; the rule is in include/biogpu.h, the bodies and the
// algorithm in bgzf_deflate_rule.h).  The input is cut as bg_bgzf_frame cuts it; one workgroup of 256 lanes takes one payload
// through the phases of dfl_phase with a barrier behind each and leaves the finished block in a slot of the ctx's scratch
// and its length in an array.  Blocks no longer have closed-form sizes, so they are placed afterwards: a scan of the lengths
// (scan.hip), then a workgroup a block copies it from its slot to its final offset, 16 bytes wide and destination-aligned
// (sam_copy_line).
// Scratch does not grow with the input: the call runs sub-batches of BGZF_DFL_BATCH blocks, and the output base of the next
// sub-batch stays on the device.  A slot holds the block (65 312 bytes) and the two per-position arrays of the parse
// (m: 4 bytes a position, f: 2): DFL_SLOT_BYTES = 456 992, 234 MB for a full sub-batch.  The payload itself is read where it
// lies (L2): with the 64 KiB of the hash table / block image in LDS there is no room for it at two workgroups a CU.
// The total is read back once, with one synchronisation.
#include "bg_common.h"
#include "bgzf_deflate_rule.h"

namespace {

constexpr uint32_t BGZF_DFL_BATCH = 512;                     // blocks of a sub-batch
constexpr size_t DFL_SLOT_BLOCK = 65312;                     // the finished block, rounded up to 16
constexpr size_t DFL_SLOT_M = DFL_SLOT_BLOCK;                // m behind it
constexpr size_t DFL_SLOT_F = DFL_SLOT_M + 4 * BGZF_PAYLOAD; // f behind that
constexpr size_t DFL_SLOT_BYTES = DFL_SLOT_F + 2 * BGZF_PAYLOAD;
static_assert(DFL_SLOT_BYTES % 16 == 0, "slots stay 16-byte aligned");

// (two waves a SIMD: the 79 KiB of LDS allow two workgroups a CU, and the register budget must not be what forbids them)
__global__ __launch_bounds__(BGZF_LANES, 2) void bgzf_deflate_kernel(const uint8_t* __restrict__ in, uint64_t in_bytes, uint64_t b0,
                                                                  uint8_t* __restrict__ slots, uint32_t* __restrict__ d_len) {
    __shared__ uint32_t s_tab[DFL_TAB];  // the hash table; behind the matches the trees' work; then the block's image
    __shared__ uint32_t s_near[DFL_NEAR];  // ... then the CRC's slicing table
    __shared__ uint32_t s_far[1024];
    __shared__ uint32_t s_hsh[BGZF_LANES];  // ... then the run-length coded header
    __shared__ uint32_t s_entry[BGZF_LANES], s_crcp[BGZF_LANES], s_bits[BGZF_LANES];
    __shared__ uint32_t s_hist[DFL_SYMS], s_code[DFL_SYMS];
    __shared__ uint8_t s_lens[DFL_SYMS];
    __shared__ dfl_state_t s_st;
    static_assert(DFL_TAB == DFL_IMAGE_WORDS && DFL_WORK + DFL_SYMS / 2 <= DFL_TAB, "what shares the table's memory fits");
    const uint32_t lane = threadIdx.x;
    const uint64_t at = (b0 + blockIdx.x) * BGZF_PAYLOAD;
    uint8_t* slot = slots + (size_t)blockIdx.x * DFL_SLOT_BYTES;
    dfl_ws_t w;
    w.src = in + at;
    w.len = in_bytes - at < BGZF_PAYLOAD ? (uint32_t)(in_bytes - at) : BGZF_PAYLOAD;
    w.slot = slot;
    w.m = (uint32_t*)(slot + DFL_SLOT_M);
    w.f = (uint16_t*)(slot + DFL_SLOT_F);
    w.tab = s_tab;
    w.img = s_tab;
    w.work = s_tab;
    w.srt = (uint16_t*)(s_tab + DFL_WORK);
    w.near = s_near;
    w.T = s_near;
    w.K = s_far;
    w.hsh = s_hsh;
    w.tok = (uint16_t*)s_hsh;
    w.entry = s_entry;
    w.crcp = s_crcp;
    w.bits = s_bits;
    w.hist = s_hist;
    w.code = s_code;
    w.lens = s_lens;
    w.st = &s_st;
#ifdef DFL_KO_TAIL  // knock-out build (tools/exp/ko_build.sh; timing only): the matches alone, no block is made
    const uint32_t n = DFL_PHASES_HEAD + 3 * dfl_tiles(w.len);
    s_st.total = 0;
#else
    const uint32_t n = dfl_phases(w.len);
#endif
    for (uint32_t k = 0; k < n; k++) {
        dfl_phase(w, k, lane);
        __syncthreads();
    }
    if (lane == 0) d_len[blockIdx.x] = s_st.total;
}

// block b of the sub-batch from its slot to *d_base + d_off[b]; its start goes to d_block_off[b] (if given)
__global__ __launch_bounds__(BGZF_LANES) void bgzf_place_kernel(const uint8_t* __restrict__ slots, const uint64_t* __restrict__ d_off,
                                                                const uint64_t* __restrict__ d_base, uint8_t* __restrict__ out,
                                                                uint64_t* __restrict__ d_block_off) {
    const uint64_t start = *d_base + d_off[blockIdx.x];
    sam_copy_line(slots + (size_t)blockIdx.x * DFL_SLOT_BYTES, out + start, d_off[blockIdx.x + 1] - d_off[blockIdx.x], threadIdx.x, BGZF_LANES, 0,
                  UINT64_MAX, true);
    if (d_block_off && threadIdx.x == 0) d_block_off[blockIdx.x] = start;
}
__global__ void bgzf_advance_kernel(uint64_t* __restrict__ d_base, const uint64_t* __restrict__ d_batch_bytes) { *d_base += *d_batch_bytes; }
// behind the last block: the closing offset, the end-of-file block
__global__ __launch_bounds__(64) void bgzf_close_kernel(uint64_t* __restrict__ d_base, uint8_t* __restrict__ out, uint64_t* __restrict__ d_close,
                                                        uint32_t eof) {
    const uint64_t end = *d_base;
    if (eof && threadIdx.x < BGZF_EOF_BYTES) out[end + threadIdx.x] = bgzf_eof_byte(threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (d_close) *d_close = end;
        if (eof) *d_base = end + BGZF_EOF_BYTES;
    }
}

int dfl_check(const bg_ctx* ctx, const void* in, uint64_t in_bytes, uint32_t flags, const void* out, uint64_t out_cap, uint64_t* out_bytes) {
    if (!ctx || !out_bytes || (flags & ~(uint32_t)BG_BGZF_EOF) || (in_bytes && !in) || (!out && out_cap)) return BG_ERR_INVALID_ARG;
    const uint64_t n_blocks = (in_bytes + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD;
    if (n_blocks > 0x7FFFFFFEull) return BG_ERR_TOO_LARGE;
    *out_bytes = in_bytes + BGZF_EXTRA * n_blocks + ((flags & BG_BGZF_EOF) ? BGZF_EOF_BYTES : 0);  // the stored bound
    return BG_OK;
}

}  // namespace

extern "C" int bg_bgzf_deflate_dev(bg_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes, uint32_t flags, uint8_t* d_out, uint64_t out_cap,
                                   uint64_t* d_block_off, uint64_t* out_bytes, void* stream) {
    int rc = dfl_check(ctx, d_in, in_bytes, flags, d_out, out_cap, out_bytes);
    if (rc || !d_out) return rc;  // null with a capacity of 0: a sizing call
    if (*out_bytes > out_cap) return BG_ERR_OPS_CAP;
    const uint64_t n_blocks = (in_bytes + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD;
    const uint32_t eof = (flags & BG_BGZF_EOF) ? 1u : 0u;
    *out_bytes = 0;
    if (!n_blocks && !eof && !d_block_off) return BG_OK;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);
    const uint64_t batch = n_blocks < BGZF_DFL_BATCH ? n_blocks : BGZF_DFL_BATCH;
    uint8_t* d_slots;
    uint32_t* d_len;
    uint64_t *d_off, *d_sums, *d_base;
    if ((rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_slots = cv.take<uint8_t>(batch * DFL_SLOT_BYTES);
        d_len = cv.take<uint32_t>(batch);
        d_off = cv.take<uint64_t>(batch + 2);
        d_sums = cv.take<uint64_t>(bg_scan_sums_words(batch));
        d_base = cv.take<uint64_t>(1);  // where the next sub-batch starts
    }))) return rc;
    BG_HIP(hipMemsetAsync(d_base, 0, 8, st));
    for (uint64_t b0 = 0; b0 < n_blocks; b0 += batch) {
        const uint32_t nb = (uint32_t)(n_blocks - b0 < batch ? n_blocks - b0 : batch);
        bgzf_deflate_kernel<<<dim3(nb), dim3(BGZF_LANES), 0, st>>>(d_in, in_bytes, b0, d_slots, d_len);
        BG_HIP(hipGetLastError());
        if ((rc = bg_scan_u32(d_len, nb, d_off, d_sums, st))) return rc;
        bgzf_place_kernel<<<dim3(nb), dim3(BGZF_LANES), 0, st>>>(d_slots, d_off, d_base, d_out, d_block_off ? d_block_off + b0 : nullptr);
        bgzf_advance_kernel<<<dim3(1), dim3(1), 0, st>>>(d_base, d_off + nb);
    }
    bgzf_close_kernel<<<dim3(1), dim3(64), 0, st>>>(d_base, d_out, d_block_off ? d_block_off + n_blocks : nullptr, eof);
    BG_HIP(hipGetLastError());
    uint64_t total = 0;
    BG_HIP(hipMemcpyAsync(&total, d_base, 8, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    *out_bytes = total;
    return BG_OK;
}

extern "C" int bg_bgzf_deflate(bg_ctx* ctx, const uint8_t* in, uint64_t in_bytes, uint32_t flags, uint8_t* out, uint64_t out_cap,
                               uint64_t* block_off, uint64_t* out_bytes) {
    int rc = dfl_check(ctx, in, in_bytes, flags, out, out_cap, out_bytes);
    if (rc || !out) return rc;
    const uint64_t bound = *out_bytes, n_blocks = (in_bytes + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD;
    if (bound > out_cap) return BG_ERR_OPS_CAP;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_in = s.up(in, in_bytes);
    uint8_t* d_out = s.out<uint8_t>(bound);
    uint64_t* d_block_off = block_off ? s.out<uint64_t>(n_blocks + 1) : nullptr;
    if (s.rc) return s.rc;
    if ((rc = bg_bgzf_deflate_dev(ctx, d_in, in_bytes, flags, d_out, bound, d_block_off, out_bytes, s.st))) return rc;
    s.down(out, d_out, *out_bytes);
    if (block_off) s.down(block_off, d_block_off, n_blocks + 1);
    return s.sync();
}
