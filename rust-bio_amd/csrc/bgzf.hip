// BGZF framing of a byte stream (bg_bgzf_frame[_dev]; the container is defined in include/biogpu.h, the bodies in bam_rule.h).
// The call knows nothing of BAM: it cuts any buffer into payloads of 65 280 bytes and writes each as one gzip member that
// holds a stored deflate block.  Every size and offset is closed-form (block b starts at 65 311 b, its payload 23 bytes on),
// so nothing is read back and the device flavour is asynchronous.
// One workgroup of 256 lanes takes one payload and passes over it once: lane l loads the destination-aligned vectors l,
// l + 256, ... (sam_rule.h's plan and sam_copy_vec: the destination is at every residue mod 16, the source mostly at
// another), all of them before the first store, stores them, and feeds the same registers to the CRC-32: a raw register
// from 0 over each vector with the slicing-by-4 table in LDS, joined to the lane's register by a multiplication by
// x^(8 * 4096) mod P (four lookups in a second table), and the lane's register multiplied by x^(8 t) for the t payload
// bytes behind its last vector.  CRC is linear, so the XOR of the lanes' registers is the payload's raw register; one lane
// turns it into the CRC-32 (bam_crc_finish) and writes the trailer.  A short last payload needs nothing special: lanes
// without bytes contribute 0.
#include "bam_rule.h"
#include "bg_common.h"

namespace {

__global__ __launch_bounds__(BGZF_LANES) void bgzf_frame_kernel(const uint8_t* __restrict__ in, uint64_t in_bytes, uint64_t n_blocks,
                                                                uint8_t* __restrict__ out) {
    __shared__ uint32_t s_table[1024];
    __shared__ uint32_t s_far[1024];
    __shared__ uint32_t s_part[BGZF_LANES / 64];
    const uint32_t lane = threadIdx.x;
    const uint64_t b = blockIdx.x;
    if (b == n_blocks) {  // the end-of-file block behind the last payload
        if (lane < BGZF_EOF_BYTES) out[n_blocks * BGZF_EXTRA + in_bytes + lane] = bgzf_eof_byte(lane);
        return;
    }
    s_table[lane] = bam_crc_byte_entry(lane);
    for (uint32_t k = 0; k < 4; k++) s_far[256 * k + lane] = bam_crc_far_entry(256 * k + lane);
    __syncthreads();
    bam_crc_slices(s_table, lane);
    __syncthreads();
    const uint64_t at = b * BGZF_PAYLOAD;
    const uint32_t len = in_bytes - at < BGZF_PAYLOAD ? (uint32_t)(in_bytes - at) : BGZF_PAYLOAD;
    uint8_t* block = out + b * (BGZF_PAYLOAD + BGZF_EXTRA);
    if (lane < BGZF_HEAD) block[lane] = bgzf_head_byte(lane, len);
    uint32_t c = bgzf_lane(s_table, s_far, in + at, block + BGZF_HEAD, len, lane);
    for (int m = 32; m > 0; m >>= 1) c ^= __shfl_xor(c, m);
    if ((lane & 63u) == 0) s_part[lane >> 6] = c;
    __syncthreads();
    if (lane == 0) {
        uint32_t raw = 0;
        for (uint32_t w = 0; w < BGZF_LANES / 64; w++) raw ^= s_part[w];
        bam_put32(block + BGZF_HEAD + len, bam_crc_finish(raw, len));
        bam_put32(block + BGZF_HEAD + len + 4, len);
    }
}

int bgzf_check(const bg_ctx* ctx, const void* in, uint64_t in_bytes, uint32_t flags, const void* out, uint64_t out_cap, uint64_t* out_bytes) {
    if (!ctx || !out_bytes || (flags & ~(uint32_t)BG_BGZF_EOF) || (in_bytes && !in) || (!out && out_cap)) return BG_ERR_INVALID_ARG;
    const uint64_t n_blocks = (in_bytes + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD;
    if (n_blocks > 0x7FFFFFFEull) return BG_ERR_TOO_LARGE;  // one workgroup a block
    *out_bytes = in_bytes + BGZF_EXTRA * n_blocks + ((flags & BG_BGZF_EOF) ? BGZF_EOF_BYTES : 0);
    return BG_OK;
}

}  // namespace

extern "C" int bg_bgzf_frame_dev(bg_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes, uint32_t flags, uint8_t* d_out, uint64_t out_cap,
                                 uint64_t* out_bytes, void* stream) {
    int rc = bgzf_check(ctx, d_in, in_bytes, flags, d_out, out_cap, out_bytes);
    if (rc || !d_out) return rc;  // null with a capacity of 0: a sizing call
    if (*out_bytes > out_cap) return BG_ERR_OPS_CAP;
    const uint64_t n_blocks = (in_bytes + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD;
    const uint64_t grid = n_blocks + ((flags & BG_BGZF_EOF) ? 1 : 0);
    if (!grid) return BG_OK;
    BG_HIP(hipSetDevice(ctx->device));
    bgzf_frame_kernel<<<dim3((uint32_t)grid), dim3(BGZF_LANES), 0, (hipStream_t)stream>>>(d_in, in_bytes, n_blocks, d_out);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

extern "C" int bg_bgzf_frame(bg_ctx* ctx, const uint8_t* in, uint64_t in_bytes, uint32_t flags, uint8_t* out, uint64_t out_cap,
                             uint64_t* out_bytes) {
    int rc = bgzf_check(ctx, in, in_bytes, flags, out, out_cap, out_bytes);
    if (rc || !out) return rc;
    if (*out_bytes > out_cap) return BG_ERR_OPS_CAP;
    if (!*out_bytes) return BG_OK;
    bg_stage s(ctx, ctx->stream);
    const uint8_t* d_in = s.up(in, in_bytes);
    uint8_t* d_out = s.out<uint8_t>(*out_bytes);
    if (s.rc) return s.rc;
    if ((rc = bg_bgzf_frame_dev(ctx, d_in, in_bytes, flags, d_out, *out_bytes, out_bytes, s.st))) return rc;
    s.down(out, d_out, *out_bytes);
    return s.sync();
}
