// bg_myers_long_best_batch[_dev], bg_myers_long_find_all_batch[_dev]: bio::pattern_matching::myers::long::Myers<u64> (the
// block-based variant: patterns of more than 64 symbols) for batches of texts against a handful of patterns.
// include/biogpu.h has the contract, the tests hold the reference restated line by line; myers_common.h holds
// what this file shares with myers.hip (texts, records, byte classes, the tables' upload, the host flavour).
//
// One lane per job (text t, pattern p), as in myers.hip.  The pattern's ceil(m / 64) blocks are pv[NB], mv[NB] in
// registers; a text column is advance_block (long.rs:136-179) block after block, the carry (-1, 0, +1) handed down in a
// register, and only the bottom block's distance is kept.  The kernels are instantiated for NB = 1, 2, 3, 4, 8, 16 blocks;
// a launch holds consecutive patterns of one instantiation (the smallest that holds them), so the block loop unrolls and
// nothing is indexed at run time; blocks a pattern does not have are predicated off (b < nb: uniform in a wavefront but for
// the one where two patterns meet).
//
// No Ukkonen band.  The reference keeps, per column, only the blocks that can still reach max_dist (long.rs:239-268) and
// reports a column only when all blocks were computed.  Every cell whose value is at most max_dist lies in a computed block
// and has its exact value there, and a traceback from a hit reads nothing else that matters: the uncomputed neighbours
// ("barrier" blocks, long.rs:339-343) only say "larger than here", which the exact values say too.  So all blocks in every
// column give the same ends, distances and paths; tests/test_myers_long_rule.py compares the two on the restatement.  The
// price is NB block steps per column where the band would often need fewer; the gain is a lane that never branches on its
// own band height.
//
// Traceback columns.  As in myers.hip the best call runs the text twice and stores, in the second pass, the last
// R = m + min(k, m) + 2 columns up to the best end (traceback.rs:153-186); the find-all call keeps the reference's ring of
// R columns.  A column is NB words of pv, NB of mv and the bottom distance: planes [slot][block][lane] and [slot][lane],
//     per job  (16 * NB + 4) * (m + min(k, m) + 2)  bytes,
// independent of the text's length; a block's own distance (State::dist of long.rs) is the bottom distance taken up through
// the blocks below it by popcounts.  m = 1024 and k >= 1024: 260 * 2050 = 533 000 bytes per job, 503 jobs (512 after
// rounding to the block size) per launch under the 256 MB budget; m = 66, k = 3: 36 * 71 = 2556 bytes, 105 000 jobs.
#include "myers_common.h"

namespace {

constexpr uint32_t ML_MAX_DIST = 0xFFFFFFFFu;  // the reference's usize::MAX: the max-state column, "no distance"

struct MlArgs {
    const uint8_t* text;
    const uint64_t* off;
    uint64_t n_texts;
    const uint64_t* peqc;  // [block][n_cls], pattern p's blocks from pb[p]
    const uint32_t* pm;    // [n_pat]
    const uint32_t* pb;    // [n_pat + 1]
    const uint8_t* cls;    // [256]
    uint32_t n_pat, n_cls, g0, gn;
    uint64_t i0, i1;  // this launch's range of the group's index space: idx = pl * n_texts + t
    uint32_t k, max_hits;
    uint64_t* s_pv;  // [slot][NB][pitch]
    uint64_t* s_mv;
    uint32_t* s_dist;  // [slot][pitch]
    uint64_t pitch;
    bg_alignment_t* aln;
    uint32_t* count;
    uint8_t* ops;
    uint64_t ops_stride;
    int* flag;
};

struct MlJob {
    uint64_t job, lane;
    uint32_t m, ylen;
    const uint8_t* tb;
    const uint8_t* te;
};

struct MlShape {  // of one pattern
    uint32_t m, nb, last_m;  // blocks; symbols in the last block (1 .. 64)
    uint64_t high_last;      // Peq::high_mask of the last block (long.rs:113); the others' is bit 63
    __host__ __device__ __forceinline__ explicit MlShape(uint32_t m_) : m(m_), nb((m_ + 63) / 64), last_m(((m_ - 1) & 63) + 1) {
        high_last = 1ull << (last_m - 1);
    }
    __host__ __device__ __forceinline__ uint64_t chunk_mask(uint32_t b) const {  // the bits of block b that are pattern rows
        return b + 1 == nb && last_m < 64 ? (1ull << last_m) - 1 : ~0ull;
    }
};

template <int NB>
struct MlState {
    uint64_t pv[NB], mv[NB];
    uint32_t dist;  // of the bottom row
    __host__ __device__ __forceinline__ void init(uint32_t d) {  // States::new with every block (long.rs:196-236)
#pragma unroll
        for (int b = 0; b < NB; b++) {
            pv[b] = ~0ull;
            mv[b] = 0;
        }
        dist = d;
    }
};

// States::step without the band: advance_block (long.rs:136-179) over the pattern's blocks; peq: block b's word of the
// column's byte class at peq[b * stride]
template <int NB>
__host__ __device__ __forceinline__ void ml_step(const uint64_t* peq, uint32_t stride, const MlShape& sh, MlState<NB>& s) {
    int hin = 0;
#pragma unroll
    for (int b = 0; b < NB; b++) {
        if ((uint32_t)b < sh.nb) {
            uint64_t eq = peq[(size_t)b * stride];
            const uint64_t high = (uint32_t)b + 1 == sh.nb ? sh.high_last : 1ull << 63;
            const uint64_t pv = s.pv[b], mv = s.mv[b];
            const uint64_t xv = eq | mv;
            if (hin < 0) eq |= 1;
            const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
            uint64_t ph = mv | ~(xh | pv);
            uint64_t mh = pv & xh;
            const int hout = (int)((ph & high) != 0) - (int)((mh & high) != 0);
            ph <<= 1;
            mh <<= 1;
            if (hin < 0) mh |= 1;
            if (hin > 0) ph |= 1;
            s.pv[b] = mh | ~(xv | ph);
            s.mv[b] = ph & xv;
            hin = hout;
        }
    }
    s.dist += (uint32_t)hin;  // the bottom block's hout
}

struct MlBlock {  // State<u64, usize> of one block
    uint64_t pv, mv;
    uint32_t dist;
};
// State::adjust_one_up / adjust_up_by, myers_impl.rs:70-77, 97-103
__host__ __device__ __forceinline__ void ml_one_up(MlBlock& s, uint64_t pos_mask) {
    if (s.pv & pos_mask)
        s.dist--;
    else if (s.mv & pos_mask)
        s.dist++;
}
__host__ __device__ __forceinline__ void ml_up_by(MlBlock& s, uint64_t range_mask) {
    s.dist += (uint32_t)__builtin_popcountll(s.mv & range_mask) - (uint32_t)__builtin_popcountll(s.pv & range_mask);
}

template <int NB>
struct MlScratch {
    uint64_t* pv;
    uint64_t* mv;
    uint32_t* dist;
    uint64_t pitch, lane;
    __host__ __device__ __forceinline__ void put(uint32_t slot, const MlShape& sh, const MlState<NB>& s) const {
#pragma unroll
        for (int b = 0; b < NB; b++)
            if ((uint32_t)b < sh.nb) {
                const uint64_t i = ((uint64_t)slot * NB + b) * pitch + lane;
                pv[i] = s.pv[b];
                mv[i] = s.mv[b];
            }
        dist[(uint64_t)slot * pitch + lane] = s.dist;
    }
    // block b of the column in `slot` with its own distance: the bottom distance taken up through the rows of the blocks
    // below (in the max-state column every block has the maximum, long.rs:315-320)
    __host__ __device__ inline MlBlock get(uint32_t slot, uint32_t b, const MlShape& sh) const {
        uint32_t d = dist[(uint64_t)slot * pitch + lane];
        if (d != ML_MAX_DIST)
            for (uint32_t bb = sh.nb - 1; bb > b; bb--) {
                const uint64_t i = ((uint64_t)slot * NB + bb) * pitch + lane, cm = sh.chunk_mask(bb);
                d += (uint32_t)__builtin_popcountll(mv[i] & cm) - (uint32_t)__builtin_popcountll(pv[i] & cm);
            }
        const uint64_t i = ((uint64_t)slot * NB + b) * pitch + lane;
        return MlBlock{pv[i], mv[i], d};
    }
};

// _traceback_at (traceback.rs:235-318) with LongTracebackHandler (long.rs:402-563) from the column in slot `pos`; the next
// column to the left of slot s is slot s - 1, and `wrap` (the ring's size; 0: no ring) after slot 0, the reference's
// chain + cycle.  Operations go out in reverse, from ops_end - 1 down, while they fit `cap`.  Returns the aligned columns.
template <int NB>
__host__ __device__ inline uint32_t ml_traceback(const MlScratch<NB>& S, uint32_t pos, uint32_t wrap, const MlShape& sh, uint8_t* ops_end,
                                                 uint64_t cap, uint32_t& n_ops, bool& broken) {
    const uint64_t top = 1ull << 63;
    const uint64_t mask0 = sh.high_last;
    uint32_t cur = pos;  // slot of the left column once next_col has run
    auto next_col = [&]() {
        if (cur == 0) {
            if (wrap == 0) {
                broken = true;  // a path left of the max-state column: cannot happen (the initial column only moves up)
                return 0u;
            }
            cur = wrap;
        }
        return --cur;
    };
    uint32_t col = pos, left_col = next_col();
    // LongTracebackHandler::new, long.rs:430-453
    uint32_t left_idx = sh.nb - 1, block_idx = sh.nb - 1;
    uint64_t left_adj = mask0, max_mask = mask0, pos_mask = mask0;
    if (sh.last_m == 1 && sh.nb > 1) {
        left_idx = sh.nb - 2;
        left_adj = 0;
        max_mask = top;
    }
    MlBlock left = S.get(left_col, left_idx, sh);
    ml_up_by(left, left_adj);
    MlBlock block = S.get(col, block_idx, sh);
    // adjust_left_up, long.rs:461-473
    auto adjust_left_up = [&]() {
        const bool at_boundary = (left_adj & 2) != 0 && left_idx > 0;
        if (!at_boundary) {
            left_adj = (left_adj >> 1) | max_mask;
        } else {
            max_mask = top;
            left_adj = 0;
            left_idx--;
        }
        return at_boundary;
    };
    uint32_t h = 0, n = 0;
    // every turn moves one row up or one column left: at most m + (m + dist) <= 3 m turns
    for (uint32_t turn = 0; !(pos_mask == 0 && block_idx == 0) && turn < 3 * sh.m + 4; turn++) {
        uint8_t op;
        bool move_left = true, diagonal = false;
        if (left.dist + 1 == block.dist) {  // Subst
            diagonal = true;
            op = BG_OP_SUBST;
        } else if (block.pv & pos_mask) {  // try_move_up, move_up (long.rs:488-517): Ins
            if (pos_mask != 1 || block_idx == 0) {
                ml_one_up(block, pos_mask);
                pos_mask >>= 1;
            } else {
                pos_mask = top;
                block_idx--;
                block = S.get(col, block_idx, sh);
            }
            if (!adjust_left_up())
                ml_one_up(left, pos_mask);
            else
                left = S.get(left_col, left_idx, sh);
            op = BG_OP_INS;
            move_left = false;
        } else {  // try_prepare_left, long.rs:532-550: Del
            bool del = false;
            if (left_adj != 0) {
                if (left.mv & pos_mask) {
                    left.dist--;
                    del = true;
                }
            } else if (left_idx + 1 < sh.nb) {  // at a block's lower boundary: the row below is bit 0 of the next block
                const MlBlock b = S.get(left_col, left_idx + 1, sh);
                if (b.mv & 1) {
                    left = MlBlock{b.pv, b.mv, left.dist - 1};
                    del = true;
                }
            }
            if (del) {
                op = BG_OP_DEL;
            } else {  // Match
                diagonal = true;
                op = BG_OP_MATCH;
            }
        }
        if (diagonal) {  // prepare_diagonal, long.rs:520-530
            adjust_left_up();
            if (pos_mask != 1 || block_idx == 0) {
                pos_mask >>= 1;
            } else {
                pos_mask = top;
                block_idx--;
            }
        }
        if (move_left) {  // finish_move_left, long.rs:553-558
            h++;
            col = left_col;
            left_col = next_col();
            block = left;
            left = S.get(left_col, left_idx, sh);
            ml_up_by(left, left_adj);
        }
        if (ops_end && n < cap) ops_end[-(int64_t)n - 1] = op;
        n++;
    }
    if (!(pos_mask == 0 && block_idx == 0)) broken = true;
    n_ops = n;
    return h;
}

// one job of the best call; peq: the pattern's block words by class, l_cls: the byte classes (both in LDS on the device)
template <int NB>
__host__ __device__ inline void ml_best_job(const MlArgs& a, const MlJob& j, const uint64_t* peq, const uint8_t* l_cls) {
    const MlShape sh(j.m);
    const uint32_t m = j.m, n = j.ylen, k = a.k < m ? a.k : m;  // "distances cannot exceed m", long.rs:205-206
    // pass 1: the smallest distance at most k and its first end (find_all ... min_by_key)
    uint32_t best = ML_MAX_DIST, best_end = 0;
    {
        MlState<NB> s;
        s.init(m);
        MyText tx(j.tb, j.te);
        for (uint32_t i = 0; i < n; i++) {
            ml_step<NB>(peq + l_cls[tx.next()], a.n_cls, sh, s);
            if (s.dist <= k && s.dist < best) {
                best = s.dist;
                best_end = i;
            }
        }
    }
    if (best == ML_MAX_DIST) {
        a.aln[j.job] = my_no_hit(m, n);
        return;
    }
    // pass 2: the columns a traceback from best_end can reach.  Virtual column v: 0 the max state, 1 the initial state,
    // i + 2 the text's column i; kept are the last R = m + min(k, m) + 2 up to v_e, in slot v - v_lo.
    const MlScratch<NB> S{a.s_pv, a.s_mv, a.s_dist, a.pitch, j.lane};
    const uint32_t R = m + k + 2;
    const uint64_t v_e = (uint64_t)best_end + 2;
    const uint64_t v_lo = v_e >= R - 1 ? v_e - (R - 1) : 0;
    {
        MlState<NB> s;
        s.init(ML_MAX_DIST);
        if (v_lo == 0) S.put(0, sh, s);
        s.dist = m;
        if (v_lo <= 1) S.put((uint32_t)(1 - v_lo), sh, s);
        MyText tx(j.tb, j.te);
        for (uint32_t i = 0; i <= best_end; i++) {
            ml_step<NB>(peq + l_cls[tx.next()], a.n_cls, sh, s);
            const uint64_t v = (uint64_t)i + 2;
            if (v >= v_lo) S.put((uint32_t)(v - v_lo), sh, s);
        }
    }
    uint32_t n_ops = 0;
    bool broken = false;
    uint8_t* slot_end = a.ops ? a.ops + (j.job + 1) * a.ops_stride : nullptr;
    const uint32_t h = ml_traceback<NB>(S, (uint32_t)(v_e - v_lo), 0, sh, slot_end, a.ops_stride, n_ops, broken);
    bg_alignment_t r = my_hit(m, n, best_end + 1 - h, best_end + 1, best);
    my_set_ops(r, n_ops, broken, a.ops, a.ops_stride, j.job, a.flag);
    a.aln[j.job] = r;
}

// one job of the find-all call
template <int NB, bool ENDS_ONLY>
__host__ __device__ inline void ml_find_all_job(const MlArgs& a, const MlJob& j, const uint64_t* peq, const uint8_t* l_cls) {
    const MlShape sh(j.m);
    const uint32_t m = j.m, n = j.ylen, k = a.k < m ? a.k : m;
    const MlScratch<NB> S{a.s_pv, a.s_mv, a.s_dist, a.pitch, j.lane};
    const uint32_t R = m + k + 2;  // the reference's ring (myers_impl.rs:327, traceback.rs:162)
    bg_alignment_t* out = a.aln + j.job * a.max_hits;
    MlState<NB> s;
    s.init(ML_MAX_DIST);
    uint32_t pos = 1;  // ring slot of the newest column
    if (!ENDS_ONLY) {
        S.put(0, sh, s);
        s.dist = m;
        S.put(1, sh, s);
    }
    s.dist = m;
    uint32_t found = 0;
    MyText tx(j.tb, j.te);
    for (uint32_t i = 0; i < n; i++) {
        ml_step<NB>(peq + l_cls[tx.next()], a.n_cls, sh, s);
        if (!ENDS_ONLY) {
            pos = pos + 1 == R ? 0 : pos + 1;
            S.put(pos, sh, s);
        }
        if (s.dist <= k) {
            if (found < a.max_hits) {
                bg_alignment_t r;
                if (!ENDS_ONLY) {
                    uint32_t n_ops = 0;
                    bool broken = false;
                    const uint32_t h = ml_traceback<NB>(S, pos, R, sh, nullptr, 0, n_ops, broken);
                    r = my_hit(m, n, i + 1 - h, i + 1, s.dist);
                    if (broken) r.status = (int8_t)BG_ERR_TRACEBACK;
                } else {
                    r = my_hit(m, n, i + 1, i + 1, s.dist);
                }
                out[found] = r;
            }
            found++;
        }
    }
    for (uint32_t f = found; f < a.max_hits; f++) out[f] = my_no_hit(m, n);
    a.count[j.job] = found;
}

// cls[256] and the group's block words by class into LDS; false for the lanes past the launch's range.  peq: the job's
// pattern's first block in LDS.
__device__ __forceinline__ bool ml_setup(const MlArgs& a, uint64_t* l_peq, uint8_t* l_cls, MlJob& j, const uint64_t*& peq) {
    const uint32_t b0 = a.pb[a.g0], nblk = a.pb[a.g0 + a.gn] - b0;
    for (uint32_t i = threadIdx.x; i < nblk * a.n_cls; i += MY_BLOCK) l_peq[i] = a.peqc[(uint64_t)b0 * a.n_cls + i];
    for (uint32_t i = threadIdx.x; i < 256; i += MY_BLOCK) l_cls[i] = a.cls[i];
    __syncthreads();
    const uint64_t idx = a.i0 + (uint64_t)blockIdx.x * MY_BLOCK + threadIdx.x;
    if (idx >= a.i1) return false;
    const uint64_t t = idx % a.n_texts;
    const uint32_t p = a.g0 + (uint32_t)(idx / a.n_texts);
    j.job = t * a.n_pat + p;
    j.lane = idx - a.i0;
    j.m = a.pm[p];
    const uint64_t b = a.off[t], e = a.off[t + 1];
    j.tb = a.text + b;
    j.te = a.text + e;
    j.ylen = (uint32_t)(e - b);
    peq = l_peq + (size_t)(a.pb[p] - b0) * a.n_cls;
    return true;
}

template <int NB>
__global__ __launch_bounds__(MY_BLOCK) void myers_long_best_kernel(MlArgs a) {
    extern __shared__ uint64_t l_peq[];
    uint8_t* l_cls = (uint8_t*)(l_peq + (size_t)(a.pb[a.g0 + a.gn] - a.pb[a.g0]) * a.n_cls);
    MlJob j;
    const uint64_t* peq;
    if (!ml_setup(a, l_peq, l_cls, j, peq)) return;
    ml_best_job<NB>(a, j, peq, l_cls);
}
template <int NB, bool ENDS_ONLY>
__global__ __launch_bounds__(MY_BLOCK) void myers_long_find_all_kernel(MlArgs a) {
    extern __shared__ uint64_t l_peq[];
    uint8_t* l_cls = (uint8_t*)(l_peq + (size_t)(a.pb[a.g0 + a.gn] - a.pb[a.g0]) * a.n_cls);
    MlJob j;
    const uint64_t* peq;
    if (!ml_setup(a, l_peq, l_cls, j, peq)) return;
    ml_find_all_job<NB, ENDS_ONLY>(a, j, peq, l_cls);
}

// the instantiation that holds a pattern of nb blocks
inline uint32_t ml_width(uint32_t nb) { return nb <= 4 ? nb : nb <= 8 ? 8 : 16; }

struct MlTables {
    std::vector<uint8_t> blob;  // peqc[blocks][n_cls] (uint64), pm[n_pat] (uint32), pb[n_pat + 1] (uint32), cls[256]
    uint32_t n_cls = 0, max_m = 0, max_ring = 0, max_width = 0;
    size_t off_pm = 0, off_pb = 0, off_cls = 0;
    std::vector<uint32_t> pm, pb;
};

int ml_check(const uint64_t* peq, const uint64_t* blk_off, const uint32_t* m, uint32_t n_pat) {
    if (!peq || !blk_off || !m || n_pat == 0) return BG_ERR_INVALID_ARG;
    if (n_pat > BG_MYERS_MAX_PATTERNS) return BG_ERR_TOO_LARGE;
    if (blk_off[0] != 0) return BG_ERR_INVALID_ARG;
    for (uint32_t p = 0; p < n_pat; p++) {
        if (m[p] == 0) return BG_ERR_INVALID_ARG;                 // "Pattern is empty", long.rs:83
        if (m[p] > BG_MYERS_LONG_MAX_M) return BG_ERR_TOO_LARGE;  // this library's limit; the reference has none
        if (blk_off[p + 1] < blk_off[p] || blk_off[p + 1] - blk_off[p] != (m[p] + 63) / 64) return BG_ERR_INVALID_ARG;
    }
    return BG_OK;
}

// the blocks' peq words by class of text byte (bits at or above a block's chunk length do not count)
void ml_tables(const uint64_t* peq, const uint32_t* m, uint32_t n_pat, uint32_t k, MlTables& T) {
    std::vector<MyRow> rows;
    T.pm.assign(m, m + n_pat);
    T.pb.assign(n_pat + 1, 0);
    for (uint32_t p = 0; p < n_pat; p++) {
        const MlShape sh(m[p]);
        for (uint32_t b = 0; b < sh.nb; b++) rows.push_back(MyRow{peq + (size_t)(T.pb[p] + b) * 256, sh.chunk_mask(b)});
        T.pb[p + 1] = T.pb[p] + sh.nb;
        T.max_m = std::max(T.max_m, m[p]);
        T.max_ring = std::max(T.max_ring, m[p] + std::min(k, m[p]) + 2);
        T.max_width = std::max(T.max_width, ml_width(sh.nb));
    }
    uint8_t cls[256];
    std::vector<std::vector<uint64_t>> cols;
    my_classes(rows, cls, cols);
    T.n_cls = (uint32_t)cols.size();
    T.off_pm = rows.size() * T.n_cls * 8;
    T.off_pb = T.off_pm + (size_t)n_pat * 4;
    T.off_cls = T.off_pb + (size_t)(n_pat + 1) * 4;
    T.blob.assign(T.off_cls + 256, 0);
    uint64_t* peqc = (uint64_t*)T.blob.data();
    for (size_t r = 0; r < rows.size(); r++)
        for (uint32_t c = 0; c < T.n_cls; c++) peqc[r * T.n_cls + c] = cols[c][r];
    memcpy(T.blob.data() + T.off_pm, T.pm.data(), (size_t)n_pat * 4);
    memcpy(T.blob.data() + T.off_pb, T.pb.data(), (size_t)(n_pat + 1) * 4);
    memcpy(T.blob.data() + T.off_cls, cls, 256);
}

template <int NB>
void ml_launch(const MyCall& c, const MlArgs& a, dim3 grid, size_t lds_bytes, hipStream_t st) {
    if (!c.find_all)
        myers_long_best_kernel<NB><<<grid, dim3(MY_BLOCK), lds_bytes, st>>>(a);
    else if (c.ends_only)
        myers_long_find_all_kernel<NB, true><<<grid, dim3(MY_BLOCK), lds_bytes, st>>>(a);
    else
        myers_long_find_all_kernel<NB, false><<<grid, dim3(MY_BLOCK), lds_bytes, st>>>(a);
}

int ml_run(bg_ctx* ctx, const uint64_t* peq, const uint32_t* m, uint32_t n_pat, const MyCall& c, hipStream_t st) {
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);
    MlTables T;
    ml_tables(peq, m, n_pat, c.k, T);
    if (int rc = my_upload(ctx, T.blob, 1, st)) return rc;
    bg_myers_scratch* M = ctx->myers;
    const bool need_scratch = !(c.find_all && c.ends_only);
    const bool may_overflow = !c.find_all && c.d_ops && c.ops_stride < 2ull * T.max_m;
    if (may_overflow) BG_HIP(hipMemsetAsync(M->d_flag, 0, sizeof(int), st));
    // jobs per launch: the traceback columns of one launch stay within 256 MB; ENDS_ONLY stores none and is cut only on request
    // (at 40 KB a job — m = 300 — the budget leaves 6 900 jobs a launch: 27 workgroups for 256 compute units)
    const uint64_t per_job_max = (16ull * T.max_width + 4) * T.max_ring;
    uint64_t chunk = ctx->myers_chunk_jobs > 0 ? (uint64_t)ctx->myers_chunk_jobs
                     : need_scratch           ? (256ull << 20) / per_job_max
                                              : 1ull << 30;
    chunk = std::max<uint64_t>(MY_BLOCK, (chunk + MY_BLOCK - 1) / MY_BLOCK * MY_BLOCK);
    const uint64_t lds = ctx->myers_lds_bytes > 0 ? (uint64_t)ctx->myers_lds_bytes : 48u << 10;
    MlArgs a = {};
    a.text = c.d_text;
    a.off = c.d_off;
    a.n_texts = c.n_texts;
    a.peqc = (const uint64_t*)M->d;
    a.pm = (const uint32_t*)(M->d + T.off_pm);
    a.pb = (const uint32_t*)(M->d + T.off_pb);
    a.cls = M->d + T.off_cls;
    a.n_pat = n_pat;
    a.n_cls = T.n_cls;
    a.k = c.k;
    a.max_hits = c.max_hits;
    a.aln = c.d_aln;
    a.count = c.d_count;
    a.ops = c.d_ops;
    a.ops_stride = c.ops_stride;
    a.flag = M->d_flag;
    for (uint32_t g0 = 0; g0 < n_pat;) {
        // a group: consecutive patterns of one instantiation whose class tables fit the LDS budget (one always does)
        const uint32_t width = ml_width(T.pb[g0 + 1] - T.pb[g0]);
        uint32_t gn = 1;
        while (g0 + gn < n_pat && ml_width(T.pb[g0 + gn + 1] - T.pb[g0 + gn]) == width &&
               (uint64_t)(T.pb[g0 + gn + 1] - T.pb[g0]) * T.n_cls * 8 + 256 <= lds)
            gn++;
        a.g0 = g0;
        a.gn = gn;
        const uint64_t total = c.n_texts * gn;
        const size_t lds_bytes = (size_t)(T.pb[g0 + gn] - T.pb[g0]) * T.n_cls * 8 + 256;
        for (uint64_t i0 = 0; i0 < total; i0 += chunk) {
            a.i0 = i0;
            a.i1 = std::min(total, i0 + chunk);
            const uint64_t cnt = a.i1 - a.i0;
            if (need_scratch) {
                a.pitch = (cnt + 63) / 64 * 64;
                const size_t plane = (size_t)T.max_ring * width * a.pitch;
                if (int rc = bg_reserve(&ctx->tb, &ctx->tb_bytes, plane * 16 + (size_t)T.max_ring * a.pitch * 4)) return rc;
                a.s_pv = (uint64_t*)ctx->tb;
                a.s_mv = a.s_pv + plane;
                a.s_dist = (uint32_t*)(a.s_mv + plane);
            }
            const dim3 grid((uint32_t)((cnt + MY_BLOCK - 1) / MY_BLOCK));
            switch (width) {
                case 1: ml_launch<1>(c, a, grid, lds_bytes, st); break;
                case 2: ml_launch<2>(c, a, grid, lds_bytes, st); break;
                case 3: ml_launch<3>(c, a, grid, lds_bytes, st); break;
                case 4: ml_launch<4>(c, a, grid, lds_bytes, st); break;
                case 8: ml_launch<8>(c, a, grid, lds_bytes, st); break;
                default: ml_launch<16>(c, a, grid, lds_bytes, st); break;
            }
            BG_HIP(hipGetLastError());
        }
        g0 += gn;
    }
    if (may_overflow) {
        int flag = 0;
        BG_HIP(hipMemcpyAsync(&flag, M->d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
        BG_HIP(hipStreamSynchronize(st));
        if (flag) return BG_ERR_OPS_CAP;
    }
    return BG_OK;
}

}  // namespace

extern "C" int bg_myers_long_best_batch_dev(bg_ctx* ctx, const uint64_t* peq, const uint64_t* blk_off, const uint32_t* m, uint32_t n_pat,
                                            uint32_t max_dist, uint64_t n_texts, const uint8_t* d_text, const uint64_t* d_off,
                                            bg_alignment_t* d_aln, uint8_t* d_ops, uint64_t ops_stride, void* stream) {
    if (int rc = ml_check(peq, blk_off, m, n_pat)) return rc;
    if (!ctx) return BG_ERR_INVALID_ARG;
    if (n_texts == 0) return BG_OK;
    if (!d_text || !d_off || !d_aln) return BG_ERR_INVALID_ARG;
    MyCall c;
    c.k = max_dist;  // clamped to each pattern's m in its jobs (States::new, long.rs:205-206)
    c.n_texts = n_texts;
    c.d_text = d_text;
    c.d_off = d_off;
    c.d_aln = d_aln;
    c.d_ops = d_ops;
    c.ops_stride = ops_stride;
    return ml_run(ctx, peq, m, n_pat, c, (hipStream_t)stream);
}

extern "C" int bg_myers_long_best_batch(bg_ctx* ctx, const uint64_t* peq, const uint64_t* blk_off, const uint32_t* m, uint32_t n_pat,
                                        uint32_t max_dist, uint64_t n_texts, const uint8_t* text, const uint64_t* off, bg_alignment_t* aln,
                                        uint8_t* ops, uint64_t ops_stride) {
    if (int rc = ml_check(peq, blk_off, m, n_pat)) return rc;
    if (!ctx) return BG_ERR_INVALID_ARG;
    MyCall c;
    c.k = max_dist;
    c.n_texts = n_texts;
    c.ops_stride = ops_stride;
    return my_host(ctx, n_pat, c, text, off, aln, nullptr, ops,
                   [&](const MyCall& cc, hipStream_t st) { return ml_run(ctx, peq, m, n_pat, cc, st); });
}

extern "C" int bg_myers_long_find_all_batch_dev(bg_ctx* ctx, const uint64_t* peq, const uint64_t* blk_off, const uint32_t* m,
                                                uint32_t n_pat, uint32_t max_dist, uint32_t max_hits, uint32_t flags, uint64_t n_texts,
                                                const uint8_t* d_text, const uint64_t* d_off, bg_alignment_t* d_aln, uint32_t* d_count,
                                                void* stream) {
    if (int rc = ml_check(peq, blk_off, m, n_pat)) return rc;
    if (max_hits == 0 || max_hits > BG_MYERS_MAX_HITS || (flags & ~(uint32_t)BG_MYERS_ENDS_ONLY)) return BG_ERR_INVALID_ARG;
    if (!ctx) return BG_ERR_INVALID_ARG;
    if (n_texts == 0) return BG_OK;
    if (!d_text || !d_off || !d_aln || !d_count) return BG_ERR_INVALID_ARG;
    MyCall c;
    c.find_all = true;
    c.ends_only = (flags & BG_MYERS_ENDS_ONLY) != 0;
    c.k = max_dist;
    c.max_hits = max_hits;
    c.n_texts = n_texts;
    c.d_text = d_text;
    c.d_off = d_off;
    c.d_aln = d_aln;
    c.d_count = d_count;
    return ml_run(ctx, peq, m, n_pat, c, (hipStream_t)stream);
}

extern "C" int bg_myers_long_find_all_batch(bg_ctx* ctx, const uint64_t* peq, const uint64_t* blk_off, const uint32_t* m, uint32_t n_pat,
                                            uint32_t max_dist, uint32_t max_hits, uint32_t flags, uint64_t n_texts, const uint8_t* text,
                                            const uint64_t* off, bg_alignment_t* aln, uint32_t* count) {
    if (int rc = ml_check(peq, blk_off, m, n_pat)) return rc;
    if (max_hits == 0 || max_hits > BG_MYERS_MAX_HITS || (flags & ~(uint32_t)BG_MYERS_ENDS_ONLY)) return BG_ERR_INVALID_ARG;
    if (!ctx) return BG_ERR_INVALID_ARG;
    if (n_texts && !count) return BG_ERR_INVALID_ARG;
    MyCall c;
    c.find_all = true;
    c.ends_only = (flags & BG_MYERS_ENDS_ONLY) != 0;
    c.k = max_dist;
    c.max_hits = max_hits;
    c.n_texts = n_texts;
    return my_host(ctx, n_pat, c, text, off, aln, count, nullptr,
                   [&](const MyCall& cc, hipStream_t st) { return ml_run(ctx, peq, m, n_pat, cc, st); });
}
