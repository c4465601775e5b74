// bg_scan_u32: the library's general device scan — n uint32 counts into n + 1 uint64 offsets (the last one is the total).
// Its callers: the FASTQ reader's general path (newline counts per chunk, sequence and quality lengths), the operation
// compaction behind every host-buffer aligner call (bg_compact_ops_dev, core.hip), seed-and-extend (votes, candidate /
// x-byte / y-byte counts, re-seed flags: up to seven scans a pass) and the SAM line lengths (sam_emit.hip).
//
// Three kernels over blocks of 2048 items: sums per block, one block scanning those sums, every block scanning its own
// items on top of its base.  (One block scanning the ~79 000 chunk counts of a 323 MB FASTQ text by itself took 148 us;
// block sums + their scan + apply: 20.)
#include "bg_common.h"

namespace {

__global__ __launch_bounds__(256) void scan_block_sums_kernel(const uint32_t* __restrict__ in, uint64_t n, uint64_t* __restrict__ sums) {
    const uint64_t b0 = (uint64_t)blockIdx.x * 2048;
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) {
        const uint64_t j = b0 + (uint64_t)i * 256 + threadIdx.x;
        if (j < n) v += in[j];
    }
    __shared__ uint64_t s[4];
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}
// exclusive scan of up to 2^32 items by one block (items are per-block partial sums: few).  4096 items per trip: four per
// thread, wavefront scans by shuffles, the sixteen wavefront totals scanned by the first wavefront — three barriers a trip.
// (Until round 6 a Hillis-Steele scan in LDS, twenty barriers per 1024 items: 320 us for the 14 000 partial sums of a
// seed-and-extend pass, four times per pass.)
__global__ __launch_bounds__(1024) void scan_small_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint64_t n) {
    __shared__ uint64_t s_w[16], s_wb[17];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto shfl_up64 = [](uint64_t v, int o) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, o), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), o);
        return (uint64_t)hi << 32 | lo;
    };
    uint64_t carry = 0;
    for (uint64_t b = 0; b < n; b += 4096) {
        const uint64_t i0 = b + (uint64_t)tid * 4;
        uint64_t v[4], tsum = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[k] = i0 + k < n ? in[i0 + k] : 0;
            tsum += v[k];
        }
        uint64_t incl = tsum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t u = shfl_up64(incl, o);
            if ((int)lane >= o) incl += u;
        }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        if (wave == 0) {
            const uint64_t w = lane < 16 ? s_w[lane] : 0;
            uint64_t wi = w;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const uint64_t u = shfl_up64(wi, o);
                if ((int)lane >= o) wi += u;
            }
            if (lane < 16) s_wb[lane] = wi - w;
            if (lane == 15) s_wb[16] = wi;
        }
        __syncthreads();
        uint64_t run = carry + s_wb[wave] + incl - tsum;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i0 + k < n) out[i0 + k] = run;
            run += v[k];
        }
        carry += s_wb[16];
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void scan_apply_kernel(const uint32_t* __restrict__ in, uint64_t n, const uint64_t* __restrict__ base,
                                                         uint64_t* __restrict__ out) {
    __shared__ uint64_t s[256];
    const uint64_t b0 = (uint64_t)blockIdx.x * 2048 + (uint64_t)threadIdx.x * 8;
    uint64_t loc[8], v = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        loc[i] = b0 + i < n ? in[b0 + i] : 0;
        v += loc[i];
    }
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const uint64_t u = threadIdx.x >= (unsigned)o ? s[threadIdx.x - o] : 0;
        __syncthreads();
        s[threadIdx.x] += u;
        __syncthreads();
    }
    uint64_t run = base[blockIdx.x] + s[threadIdx.x] - v;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (b0 + i <= n) out[b0 + i] = run;  // index n: the closing offset
        run += loc[i];
    }
}

}  // namespace

int bg_scan_u32(const uint32_t* d_len, uint64_t n, uint64_t* d_off, uint64_t* d_sums, hipStream_t st) {
    const uint32_t nb = (uint32_t)(n / 2048 + 1);  // one more block than items need: it writes the closing offset
    scan_block_sums_kernel<<<dim3(nb), dim3(256), 0, st>>>(d_len, n, d_sums);
    scan_small_kernel<<<dim3(1), dim3(1024), 0, st>>>(d_sums, d_sums + nb, nb);
    scan_apply_kernel<<<dim3(nb), dim3(256), 0, st>>>(d_len, n, d_sums + nb, d_off);
    BG_HIP(hipGetLastError());
    return BG_OK;
}
