// The FM index builder: one front end and one device builder for both layouts (fm_index.hip: 32-bit positions, fm_wide.hip:
// 64-bit positions).  bg_fm_build uploads the caller's BWT and keeps the caller's less[]; bg_fm_build_dev takes a BWT in HBM
// and derives less[] (bwt.rs:186-199).  Both run fm_build_on_device:
//   front     alphabet -> histogram kernel -> out-of-alphabet check -> less -> symbol classes (assign_classes) -> handle
//   blocks    one thread per 192 symbols packs the 12 words of a 2-bit block and counts its four codes (both layouts)
//   narrow    32-bit scans of the counts -> block heads; one-hot bit vectors of the dense symbols and their heads; the raw BWT
//             kept when dense symbols exist
//   wide      64-bit scans -> superblock bases and heads relative to them (no dense symbols: BG_ERR_UNSUPPORTED)
//   sparse    the exception (position, byte) pairs collected by a kernel, sorted on the host (at most kMaxExcLds), for
//             either position width
//   2-step rank blocks (fm_step2.hip) behind the finished index when less[] is the BWT's own cumulative counts.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "fm_kernels.h"

using namespace bgfm;

namespace {

// Alphabet (alphabets/mod.rs:49-60): a set of bytes; Occ tabulates max_symbol + 1 of them (bwt.rs:96-99)
struct FmAlphabet {
    bool in_alpha[256] = {};
    uint32_t max_symbol = 0;
    uint32_t less_len = 0;  // max_symbol + 2 (bwt.rs:186-199)
};
FmAlphabet fm_parse_alphabet(const uint8_t* alphabet, uint32_t n_sym) {
    FmAlphabet a;
    for (uint32_t i = 0; i < n_sym; i++) {
        a.in_alpha[alphabet[i]] = true;
        a.max_symbol = std::max<uint32_t>(a.max_symbol, alphabet[i]);
    }
    if ((uint32_t)'$' <= a.max_symbol) a.in_alpha['$'] = true;  // bwt.rs:101-104: '$' is always tabulated
    a.less_len = a.max_symbol + 2;
    return a;
}

// How every byte value is ranked, decided from the BWT's histogram.
struct FmClasses {
    bool gen = false;  // dense symbols exist: three coded bytes, code 0 = "something else"
    int n_codes = 0;
    int code_of[256], sparse_of[256], dense_of[256];
    std::vector<int> sparse_syms, dense_syms;
    uint16_t cls[256];
};
void assign_classes(const uint64_t hist[256], const bool in_alpha[256], FmClasses& k) {
    // the most frequent byte values get the 2-bit codes (ties: smaller byte first)
    int order[256];
    std::iota(order, order + 256, 0);
    std::stable_sort(order, order + 256, [&](int a, int b) { return hist[a] > hist[b]; });
    uint64_t beyond4 = 0;
    for (int i = 4; i < 256; i++) beyond4 += hist[order[i]];
    k.gen = beyond4 > kMaxExcLds;  // too many exceptions for the LDS list: dense symbols get bit vectors
    std::fill(k.code_of, k.code_of + 256, -1);
    std::fill(k.sparse_of, k.sparse_of + 256, -1);
    std::fill(k.dense_of, k.dense_of + 256, -1);
    k.n_codes = 0;
    if (!k.gen) {
        for (int i = 0; i < 4 && hist[order[i]] > 0; i++) k.code_of[order[i]] = k.n_codes++;
        for (int c = 0; c < 256; c++)
            if (hist[c] && k.code_of[c] < 0) k.sparse_syms.push_back(c);
    } else {
        for (int i = 0; i < 3; i++) k.code_of[order[i]] = 1 + k.n_codes++;  // code 0 = "none of the three"
        uint64_t cum = 0;
        for (int i = 255; i >= 3; i--) {  // ascending frequency: the rare ones stay lists while they fit
            const int c = order[i];
            if (!hist[c]) continue;
            if (k.dense_syms.empty() && cum + hist[c] <= kMaxExcLds) {
                cum += hist[c];
                k.sparse_syms.push_back(c);
            } else {
                k.dense_syms.push_back(c);
            }
        }
        std::sort(k.sparse_syms.begin(), k.sparse_syms.end());
        std::sort(k.dense_syms.begin(), k.dense_syms.end());
    }
    for (size_t e = 0; e < k.sparse_syms.size(); e++) k.sparse_of[k.sparse_syms[e]] = (int)e;
    for (size_t d = 0; d < k.dense_syms.size(); d++) k.dense_of[k.dense_syms[d]] = (int)d;
    for (int c = 0; c < 256; c++) {
        if (!in_alpha[c])
            k.cls[c] = kClsPanic;
        else if (k.code_of[c] >= 0)
            k.cls[c] = (uint16_t)k.code_of[c];
        else if (hist[c] == 0)
            k.cls[c] = kClsZero;
        else if (k.sparse_of[c] >= 0)
            k.cls[c] = (uint16_t)(kClsSparse + k.sparse_of[c]);
        else
            k.cls[c] = (uint16_t)(kClsDense + k.dense_of[c]);
    }
}

__global__ __launch_bounds__(256) void fmb_hist_kernel(const uint8_t* __restrict__ b, uint64_t n, unsigned long long* __restrict__ hist) {
    __shared__ uint32_t s[256];
    s[threadIdx.x] = 0;
    __syncthreads();
    // (a block's share of a 2^40-symbol text stays below 2^32: at most 2^40 / 8192 blocks' worth per block)
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) atomicAdd(&s[b[i]], 1u);
    __syncthreads();
    if (s[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)s[threadIdx.x]);
}

struct ClsTab {
    uint8_t code[256];    // 2-bit code of the byte in the packed stream (0 for everything without one)
    uint8_t sparse[256];  // 1: sparse exception
};

// one thread per 2-bit block: 192 symbols -> 12 words + how many of each code it holds
__global__ __launch_bounds__(256) void fmb_blocks_kernel(const uint8_t* __restrict__ b, uint64_t n, uint64_t nblk, const ClsTab* __restrict__ tab,
                                                         uint32_t* __restrict__ blocks, uint32_t* __restrict__ cnt /* [4][nblk] */) {
    __shared__ uint8_t s_code[256];
    s_code[threadIdx.x] = tab->code[threadIdx.x];
    __syncthreads();
    const uint64_t blk = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (blk >= nblk) return;
    const uint64_t lo = blk * kSymPerBlock;
    uint32_t c[4] = {0, 0, 0, 0};
    for (uint32_t w = 0; w < 12; w++) {
        uint32_t word = 0;
        for (uint32_t t = 0; t < 16; t++) {
            const uint64_t i = lo + 16 * w + t;
            if (i < n) {
                const uint32_t code = s_code[b[i]];
                word |= code << (2 * t);
                c[code]++;
            }
        }
        blocks[blk * 16 + 4 + w] = word;
    }
    for (int k = 0; k < 4; k++) cnt[(uint64_t)k * nblk + blk] = c[k];
}
// narrow: the scanned counts are the block's counters
__global__ __launch_bounds__(256) void fmb_block_heads_kernel(uint64_t nblk, const uint32_t* __restrict__ scanned, uint32_t* __restrict__ blocks) {
    const uint64_t blk = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (blk >= nblk) return;
    for (int k = 0; k < 4; k++) blocks[blk * 16 + k] = scanned[(uint64_t)k * nblk + blk];
}
// wide: absolute counts (64-bit exclusive scan of cnt) -> the superblock's base and the block's counter relative to it
__global__ __launch_bounds__(256) void fmw_heads_kernel(uint64_t nblk, uint32_t sb_shift, const uint64_t* __restrict__ scanned /* [4][nblk] */,
                                                        uint32_t* __restrict__ blocks, uint64_t* __restrict__ sb) {
    const uint64_t blk = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (blk >= nblk) return;
    const uint64_t first = (blk >> sb_shift) << sb_shift;
    for (int k = 0; k < 4; k++) {
        const uint64_t base = scanned[(uint64_t)k * nblk + first];
        blocks[blk * 16 + k] = (uint32_t)(scanned[(uint64_t)k * nblk + blk] - base);
        if (blk == first) sb[(blk >> sb_shift) * 4 + k] = base;
    }
}
// one thread per (dense symbol, bit-vector block): 480 symbols -> 15 words + their population
__global__ __launch_bounds__(256) void fmb_bitvec_kernel(const uint8_t* __restrict__ b, uint64_t n, uint64_t nbv, uint32_t n_dense,
                                                         const uint8_t* __restrict__ dense_byte, uint32_t* __restrict__ bv,
                                                         uint32_t* __restrict__ cnt /* [n_dense][nbv] */) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (uint64_t)n_dense * nbv) return;
    const uint32_t d = (uint32_t)(idx / nbv);
    const uint64_t blk = idx - (uint64_t)d * nbv;
    const uint32_t sym = dense_byte[d];
    const uint64_t lo = blk * kBvBits;
    uint32_t total = 0;
    for (uint32_t w = 0; w < 15; w++) {
        uint32_t word = 0;
        for (uint32_t t = 0; t < 32; t++) {
            const uint64_t i = lo + 32 * w + t;
            if (i < n && b[i] == sym) word |= 1u << t;
        }
        bv[idx * 16 + 1 + w] = word;
        total += (uint32_t)__popc(word);
    }
    cnt[idx] = total;
}
__global__ __launch_bounds__(256) void fmb_bitvec_heads_kernel(uint64_t total, const uint32_t* __restrict__ scanned, uint32_t* __restrict__ bv) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < total) bv[idx * 16] = scanned[idx];
}
// sparse exceptions: (position, byte) appended in any order; the host sorts the few of them
template <typename Pos>
struct FmExc {
    Pos pos, byte;
};
template <typename Pos>
__global__ __launch_bounds__(256) void fmb_sparse_kernel(const uint8_t* __restrict__ b, uint64_t n, const ClsTab* __restrict__ tab,
                                                         uint32_t cap, uint32_t* __restrict__ n_out, FmExc<Pos>* __restrict__ out) {
    // (grid-stride: a launch may not exceed 2^32 threads)
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t ch = b[i];
        if (tab->sparse[ch]) {
            const uint32_t k = atomicAdd(n_out, 1u);
            if (k < cap) out[k] = FmExc<Pos>{(Pos)i, (Pos)ch};
        }
    }
}

struct U32ToU64 {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return (uint64_t)v; }
};

unsigned grid_for(uint64_t threads, uint64_t max_blocks = 0xFFFFFFFFull) { return (unsigned)std::min<uint64_t>((threads + 255) / 256, max_blocks); }

// One build: the BWT in HBM, the handle under construction and the device temporaries (freed with the builder).
struct FmBuilder {
    bg_ctx* ctx;
    const uint8_t* d_bwt;
    uint64_t n;
    hipStream_t st;
    bg_fm* fm = nullptr;
    std::vector<void*> tmp;
    uint64_t hist[256] = {};
    std::vector<uint64_t> less;  // [less_len]: the caller's, or the BWT's own cumulative counts
    bool consistent = true;      // less[] is the BWT's own: 2-step rank blocks may be built behind the index
    FmClasses K;
    ClsTab tab = {};
    ClsTab* d_tab = nullptr;

    FmBuilder(bg_ctx* c, const uint8_t* b, uint64_t n_, hipStream_t s) : ctx(c), d_bwt(b), n(n_), st(s) {}
    ~FmBuilder() { free_temps(); }
    void free_temps() {
        for (void* p : tmp) hipFree(p);
        tmp.clear();
    }
    int temp(void** p, size_t bytes) {  // a device temporary
        BG_HIP(hipMalloc(p, std::max<size_t>(bytes, 16)));
        tmp.push_back(*p);
        return BG_OK;
    }
    int keep(void** p, size_t bytes) {  // device memory the handle owns
        const size_t alloc = std::max<size_t>(bytes, 16);
        BG_HIP(hipMalloc(p, alloc));
        fm->bytes += alloc;
        return BG_OK;
    }
    int upload(void** p, const void* src, size_t bytes) {
        const int rc = keep(p, bytes);
        if (rc) return rc;
        if (bytes) BG_HIP(hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice));
        return BG_OK;
    }

    // everything that does not depend on the layout, up to the handle and the class table on the device
    int front(const FmAlphabet& al, const uint64_t* less_in, bool wide) {
        int rc;
        unsigned long long* d_hist = nullptr;
        if ((rc = temp((void**)&d_hist, sizeof(hist)))) return rc;
        BG_HIP(hipMemsetAsync(d_hist, 0, sizeof(hist), st));
        fmb_hist_kernel<<<dim3(grid_for(n, 8192)), dim3(256), 0, st>>>(d_bwt, n, d_hist);
        BG_HIP(hipMemcpyAsync(hist, d_hist, sizeof(hist), hipMemcpyDeviceToHost, st));
        BG_HIP(hipStreamSynchronize(st));
        for (uint32_t c = al.max_symbol + 1; c < 256; c++)
            if (hist[c]) return BG_ERR_OUT_OF_ALPHABET;  // Occ::new: curr_occ[c] out of bounds
        // less(bwt, alphabet) (bwt.rs:186-199) falls out of the histogram; a caller's own is taken as it is.  2-step rank
        // blocks (fm_step2.hip) lean on less[] being the BWT's own cumulative counts (LF maps the occurrences of a symbol to
        // the rows from less[symbol] on); a caller's less that says otherwise keeps single steps, where the reference's
        // arithmetic on whatever it was given is reproduced as it is
        less.assign(al.less_len, 0);
        uint64_t run = 0;
        for (uint32_t c = 0; c < al.less_len; c++) {
            less[c] = less_in ? less_in[c] : run;
            if (c <= al.max_symbol) {
                if (hist[c] && less[c] != run) consistent = false;
                run += hist[c];
            }
        }
        assign_classes(hist, al.in_alpha, K);
        if (wide && K.gen) return BG_ERR_UNSUPPORTED;  // would need rank bit vectors: not on 64-bit positions

        fm = new bg_fm;
        fm->ctx = ctx;
        fm->wide = wide;
        fm->less_len = al.less_len;
        fm->fmd_ok = true;  // the BWT is a word over dna::n_alphabet() + '$' (FMDIndex::from, fmindex.rs:323-327)
        for (int c = 0; c < 256; c++)
            if (hist[c] && (c == 0 || !strchr("ACGTNacgtn$", c))) fm->fmd_ok = false;
        for (int c = 0; c < 256; c++)
            if (K.code_of[c] >= 0) fm->code_byte[K.code_of[c]] = (uint8_t)c;
        fm->n_codes = K.gen ? 3 : K.n_codes;
        memcpy(fm->h_class, K.cls, sizeof(fm->h_class));

        for (int c = 0; c < 256; c++) {
            tab.code[c] = K.code_of[c] >= 0 ? (uint8_t)K.code_of[c] : 0;
            tab.sparse[c] = K.sparse_of[c] >= 0 ? 1 : 0;
        }
        if ((rc = temp((void**)&d_tab, sizeof(ClsTab)))) return rc;
        BG_HIP(hipMemcpyAsync(d_tab, &tab, sizeof(tab), hipMemcpyHostToDevice, st));
        return BG_OK;
    }

    // the sparse exceptions (at most kMaxExcLds positions by construction of the classes), the class table and less[]
    template <typename Pos>
    int lists(uint32_t& ns) {
        int rc;
        uint32_t* d_ns = nullptr;
        FmExc<Pos>* d_sp = nullptr;
        if ((rc = temp((void**)&d_ns, 4))) return rc;
        if ((rc = temp((void**)&d_sp, (size_t)(kMaxExcLds + 8) * sizeof(FmExc<Pos>)))) return rc;
        BG_HIP(hipMemsetAsync(d_ns, 0, 4, st));
        fmb_sparse_kernel<Pos><<<dim3(grid_for(n, 1u << 22)), dim3(256), 0, st>>>(d_bwt, n, d_tab, kMaxExcLds + 8, d_ns, d_sp);
        BG_HIP(hipGetLastError());
        BG_HIP(hipMemcpyAsync(&ns, d_ns, 4, hipMemcpyDeviceToHost, st));
        BG_HIP(hipStreamSynchronize(st));
        if (ns > kMaxExcLds) return BG_ERR_HIP;  // cannot happen: the classes were cut so that they fit
        std::vector<FmExc<Pos>> sp(ns);
        if (ns) BG_HIP(hipMemcpy(sp.data(), d_sp, (size_t)ns * sizeof(FmExc<Pos>), hipMemcpyDeviceToHost));
        std::sort(sp.begin(), sp.end(), [](const FmExc<Pos>& a, const FmExc<Pos>& b) { return a.pos < b.pos; });
        std::vector<Pos> exc_pos(ns), exc_sym_pos;
        std::vector<uint32_t> sparse_off(K.sparse_syms.size() + 1, 0);
        std::vector<uint8_t> exc_byte(ns);
        for (uint32_t e = 0; e < ns; e++) {
            exc_pos[e] = sp[e].pos;
            exc_byte[e] = (uint8_t)sp[e].byte;
        }
        for (size_t e = 0; e < K.sparse_syms.size(); e++) {
            for (uint32_t q = 0; q < ns; q++)
                if ((int)sp[q].byte == K.sparse_syms[e]) exc_sym_pos.push_back(sp[q].pos);
            sparse_off[e + 1] = (uint32_t)exc_sym_pos.size();
        }
        Pos less_dev[256] = {};
        for (uint32_t i = 0; i < less.size() && i < 256; i++) less_dev[i] = (Pos)less[i];
        if ((rc = upload(&fm->d_exc_pos, exc_pos.data(), exc_pos.size() * sizeof(Pos)))) return rc;
        if ((rc = upload(&fm->d_exc_sym_pos, exc_sym_pos.data(), exc_sym_pos.size() * sizeof(Pos)))) return rc;
        if ((rc = upload(&fm->d_sparse_off, sparse_off.data(), sparse_off.size() * 4))) return rc;
        if ((rc = upload(&fm->d_exc_byte, exc_byte.data(), exc_byte.size()))) return rc;
        if ((rc = upload(&fm->d_class, K.cls, sizeof(K.cls)))) return rc;
        if ((rc = upload(&fm->d_less, less_dev, sizeof(less_dev)))) return rc;
        return BG_OK;
    }

    int narrow() {
        int rc;
        const uint64_t nblk = (n + kSymPerBlock - 1) / kSymPerBlock, nbv = (n + kBvBits - 1) / kBvBits;
        const size_t n_dense = K.dense_syms.size();
        // ---- 2-bit blocks
        uint32_t *d_cnt = nullptr, *d_scan = nullptr;
        void* d_cub = nullptr;
        const uint64_t n_cnt = std::max<uint64_t>(4 * nblk, (uint64_t)n_dense * nbv);
        if ((rc = keep(&fm->d_blocks, nblk * 64))) return rc;
        if ((rc = temp((void**)&d_cnt, n_cnt * 4))) return rc;
        if ((rc = temp((void**)&d_scan, n_cnt * 4))) return rc;
        size_t cub_bytes = 0;
        BG_HIP(rocprim::exclusive_scan(nullptr, cub_bytes, d_cnt, d_scan, 0u, std::max<uint64_t>(nblk, nbv), rocprim::plus<uint32_t>(), st));
        if ((rc = temp(&d_cub, cub_bytes))) return rc;
        fmb_blocks_kernel<<<dim3(grid_for(nblk)), dim3(256), 0, st>>>(d_bwt, n, nblk, d_tab, (uint32_t*)fm->d_blocks, d_cnt);
        BG_HIP(hipGetLastError());
        for (int k = 0; k < 4; k++)
            BG_HIP(rocprim::exclusive_scan(d_cub, cub_bytes, d_cnt + (uint64_t)k * nblk, d_scan + (uint64_t)k * nblk, 0u, nblk, rocprim::plus<uint32_t>(), st));
        fmb_block_heads_kernel<<<dim3(grid_for(nblk)), dim3(256), 0, st>>>(nblk, d_scan, (uint32_t*)fm->d_blocks);
        // ---- one-hot bit vectors of the dense symbols
        if ((rc = keep(&fm->d_bitvecs, n_dense * nbv * 64))) return rc;
        std::vector<uint8_t> dense_byte(K.dense_syms.begin(), K.dense_syms.end());
        if (n_dense) {
            uint8_t* d_db = nullptr;
            if ((rc = temp((void**)&d_db, n_dense))) return rc;
            BG_HIP(hipMemcpyAsync(d_db, dense_byte.data(), n_dense, hipMemcpyHostToDevice, st));
            const uint64_t tot = (uint64_t)n_dense * nbv;
            fmb_bitvec_kernel<<<dim3(grid_for(tot)), dim3(256), 0, st>>>(d_bwt, n, nbv, (uint32_t)n_dense, d_db, (uint32_t*)fm->d_bitvecs, d_cnt);
            BG_HIP(hipGetLastError());
            for (size_t d = 0; d < n_dense; d++)
                BG_HIP(rocprim::exclusive_scan(d_cub, cub_bytes, d_cnt + d * nbv, d_scan + d * nbv, 0u, nbv, rocprim::plus<uint32_t>(), st));
            fmb_bitvec_heads_kernel<<<dim3(grid_for(tot)), dim3(256), 0, st>>>(tot, d_scan, (uint32_t*)fm->d_bitvecs);
        }
        uint32_t ns = 0;
        if ((rc = lists<uint32_t>(ns))) return rc;
        if (K.gen) {  // K6 reads bwt[pos] here
            if ((rc = keep(&fm->d_bwt_raw, n))) return rc;
            BG_HIP(hipMemcpyAsync(fm->d_bwt_raw, d_bwt, n, hipMemcpyDeviceToDevice, st));
        }
        BG_HIP(hipStreamSynchronize(st));
        fm->dev.blocks = (const uint4*)fm->d_blocks;
        fm->dev.bitvecs = (const uint4*)fm->d_bitvecs;
        fm->dev.exc_pos = (const uint32_t*)fm->d_exc_pos;
        fm->dev.exc_sym_pos = (const uint32_t*)fm->d_exc_sym_pos;
        fm->dev.sparse_off = (const uint32_t*)fm->d_sparse_off;
        fm->dev.sym_class = (const uint16_t*)fm->d_class;
        fm->dev.less = (const uint32_t*)fm->d_less;
        fm->dev.bwt_raw = (const uint8_t*)fm->d_bwt_raw;
        fm->dev.n = (uint32_t)n;
        fm->dev.n_exc = K.gen ? 0u : ns;
        fm->dev.nbv_blocks = (uint32_t)nbv;
        fm->dev.n_dense = (uint32_t)n_dense;
        return BG_OK;
    }

    int wide() {
        int rc;
        const uint64_t nblk = (n + kSymPerBlock - 1) / kSymPerBlock;
        const uint32_t sb_shift = ctx->fm_wide_sb_shift;
        const uint64_t n_sb = ((nblk - 1) >> sb_shift) + 1;
        uint32_t* d_cnt = nullptr;
        uint64_t* d_scan = nullptr;
        void* d_cub = nullptr;
        if ((rc = keep(&fm->d_blocks, nblk * 64))) return rc;
        if ((rc = keep(&fm->d_sb, n_sb * 32))) return rc;
        if ((rc = temp((void**)&d_cnt, 4 * nblk * 4))) return rc;
        if ((rc = temp((void**)&d_scan, 4 * nblk * 8))) return rc;
        size_t cub_bytes = 0;
        BG_HIP(rocprim::exclusive_scan(nullptr, cub_bytes, rocprim::make_transform_iterator(d_cnt, U32ToU64()), d_scan, (uint64_t)0, nblk,
                                       rocprim::plus<uint64_t>(), st));
        if ((rc = temp(&d_cub, cub_bytes))) return rc;
        fmb_blocks_kernel<<<dim3(grid_for(nblk)), dim3(256), 0, st>>>(d_bwt, n, nblk, d_tab, (uint32_t*)fm->d_blocks, d_cnt);
        BG_HIP(hipGetLastError());
        for (int k = 0; k < 4; k++)
            BG_HIP(rocprim::exclusive_scan(d_cub, cub_bytes, rocprim::make_transform_iterator(d_cnt + (uint64_t)k * nblk, U32ToU64()),
                                           d_scan + (uint64_t)k * nblk, (uint64_t)0, nblk, rocprim::plus<uint64_t>(), st));
        fmw_heads_kernel<<<dim3(grid_for(nblk)), dim3(256), 0, st>>>(nblk, sb_shift, d_scan, (uint32_t*)fm->d_blocks, (uint64_t*)fm->d_sb);
        BG_HIP(hipGetLastError());
        uint32_t ns = 0;
        if ((rc = lists<uint64_t>(ns))) return rc;
        BG_HIP(hipStreamSynchronize(st));
        fm->wdev.blocks = (const uint4*)fm->d_blocks;
        fm->wdev.sb = (const uint64_t*)fm->d_sb;
        fm->wdev.exc_pos = (const uint64_t*)fm->d_exc_pos;
        fm->wdev.exc_sym_pos = (const uint64_t*)fm->d_exc_sym_pos;
        fm->wdev.sparse_off = (const uint32_t*)fm->d_sparse_off;
        fm->wdev.sym_class = (const uint16_t*)fm->d_class;
        fm->wdev.less = (const uint64_t*)fm->d_less;
        fm->wdev.n = n;
        fm->wdev.n_exc = ns;
        fm->wdev.sb_shift = sb_shift;
        return BG_OK;
    }
};

// The index of a BWT in HBM, on the layout its length calls for.  less_in null: the BWT's own cumulative counts; less_out
// (if given) receives the less[] of the index, al.less_len entries.
int fm_build_on_device(bg_ctx* ctx, const uint8_t* d_bwt, uint64_t n, const FmAlphabet& al, const uint64_t* less_in, uint64_t* less_out,
                       bg_fm** out, hipStream_t st) {
    BG_HIP(hipSetDevice(ctx->device));
    const bool wide = n >= fm_wide_threshold(ctx);
    FmBuilder b(ctx, d_bwt, n, st);
    int rc = b.front(al, less_in, wide);
    if (!rc) rc = wide ? b.wide() : b.narrow();
    b.free_temps();
    if (rc) {
        bg_fm_free(b.fm);
        return rc;
    }
    if (less_out) memcpy(less_out, b.less.data(), b.less.size() * 8);
    if (b.consistent) wide ? fm_build_step2_wide(b.fm, st) : fm_build_step2(b.fm, st);
    *out = b.fm;
    return BG_OK;
}

}  // namespace

// the exported builders: the builder above + what bg_fm_save needs to write the index out again (fm_persist.hip)
extern "C" int bg_fm_build(bg_ctx* ctx, const uint8_t* bwt, uint64_t n, const uint64_t* less, uint32_t less_len, uint32_t occ_k,
                           const uint8_t* alphabet, uint32_t n_sym, bg_fm** out) {
    if (!ctx || !bwt || !less || !alphabet || !out || n == 0 || n_sym == 0 || occ_k == 0) return BG_ERR_INVALID_ARG;
    if (n > (1ull << 40)) return BG_ERR_TOO_LARGE;
    const FmAlphabet al = fm_parse_alphabet(alphabet, n_sym);
    if (less_len != al.less_len) return BG_ERR_INVALID_ARG;
    // the BWT goes up and the device builder lays the index out (the caller's less[] kept)
    BG_HIP(hipSetDevice(ctx->device));
    uint8_t* d_b = nullptr;
    BG_HIP(hipMalloc((void**)&d_b, n));
    int rc = bg_copy_pieces(d_b, bwt, n, hipMemcpyHostToDevice, ctx->stream) == hipSuccess ? BG_OK : BG_ERR_HIP;
    if (!rc) rc = fm_build_on_device(ctx, d_b, n, al, less, nullptr, out, ctx->stream);
    hipStreamSynchronize(ctx->stream);
    hipFree(d_b);
    if (rc == BG_OK) fm_remember_inputs(*out, alphabet, n_sym, occ_k, less, less_len);
    return rc;
}
extern "C" int bg_fm_build_dev(bg_ctx* ctx, const uint8_t* d_bwt, uint64_t n, uint32_t occ_k, const uint8_t* alphabet, uint32_t n_sym,
                               uint64_t* less_out, bg_fm** out, void* stream) {
    if (!ctx || !d_bwt || !alphabet || !out || n == 0 || n_sym == 0 || occ_k == 0) return BG_ERR_INVALID_ARG;
    if (n > (1ull << 40)) return BG_ERR_TOO_LARGE;
    const FmAlphabet al = fm_parse_alphabet(alphabet, n_sym);
    std::vector<uint64_t> less(al.less_len, 0);
    const int rc = fm_build_on_device(ctx, d_bwt, n, al, nullptr, less.data(), out, (hipStream_t)stream);
    if (rc == BG_OK) {
        fm_remember_inputs(*out, alphabet, n_sym, occ_k, less.data(), al.less_len);
        if (less_out) memcpy(less_out, less.data(), less.size() * 8);
    }
    return rc;
}
