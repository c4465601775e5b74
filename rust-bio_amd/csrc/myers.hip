// bg_myers_best_batch[_dev], bg_myers_find_all_batch[_dev]: bio::pattern_matching::myers::Myers<u64> for batches of texts
// against a handful of patterns (include/biogpu.h has the contract; the tests hold the reference restated line by line).
// myers_common.h holds what this file shares with myers_long.hip (patterns of more than 64 symbols): the text walk, the
// records, the byte classes, the tables' upload and the host flavour.
//
// One lane per job (text t, pattern p): pv, mv and dist live in registers and one step is the reference's _step
// (simple.rs:95-117) in 64-bit integer operations — the add in xh is a real 64-bit add, its carry out of bit 31 is the
// compiler's v_add_co / v_addc pair.  A launch covers one pattern group and a range of its (pattern, text) index space
// with the text running fastest: the lanes of a wavefront hold consecutive texts of the packed buffer and one pattern, so
// their loads fall into one contiguous region and their table reads into a few LDS words.
//
// Tables.  A pattern's peq is 2 KB; the host compacts the 256 text bytes into classes (bytes whose peq words agree in
// every pattern of the call: five for plain DNA patterns) and LDS holds cls[256] and peq[pattern][class] of one group of
// patterns; a call whose patterns do not fit runs one launch sequence per group.
//
// Texts.  A lane streams its own text: single bytes up to the first 8-byte boundary, aligned 8-byte words while eight
// bytes remain, single bytes to the end — never a byte outside [off[t], off[t + 1]).
//
// Traceback columns.  The best call runs the text twice: a pass in registers that finds (end, dist), then
// a pass that stores only the columns the traceback from that end can reach — the last m + min(k, m) + 2 of the
// virtual column sequence (max state, initial state, text columns; traceback.rs:153-186), the size of the reference's own
// ring (myers_impl.rs:323-334) — as scratch[slot][lane] (pv and mv planes of 8 bytes, a dist plane of 1), so a wavefront's
// stores coalesce: 17 * (m + min(k, m) + 2) <= 2210 bytes per job, independent of the text's length.  The find-all call
// keeps the reference's ring in the same layout and traces back (coordinates only) at each hit column; ENDS_ONLY stores
// nothing.  Launches are cut so that the scratch of one stays within a budget (option myers_chunk_jobs).
#include "myers_common.h"

namespace {

struct MyArgs {
    const uint8_t* text;
    const uint64_t* off;
    uint64_t n_texts;
    const uint64_t* peqc;  // [n_pat][n_cls]
    const uint32_t* pm;    // [n_pat]
    const uint8_t* cls;    // [256]
    uint32_t n_pat, n_cls, g0, gn;
    uint64_t i0, i1;  // this launch's range of the group's index space: idx = pl * n_texts + t
    uint32_t k, max_hits;
    uint64_t* s_pv;
    uint64_t* s_mv;
    uint8_t* s_dist;
    uint64_t pitch;  // lanes per scratch slot
    bg_alignment_t* aln;
    uint32_t* count;
    uint8_t* ops;
    uint64_t ops_stride;
    int* flag;  // set to 1 when some path did not fit its slot
};

struct MyState {
    uint64_t pv, mv;
    uint32_t dist;  // the reference's u8
};

// _step, simple.rs:95-117
__host__ __device__ __forceinline__ void my_step(uint64_t eq, uint64_t bound, MyState& s) {
    const uint64_t xv = eq | s.mv;
    const uint64_t xh = (((eq & s.pv) + s.pv) ^ s.pv) | eq;
    uint64_t ph = s.mv | ~(xh | s.pv);
    uint64_t mh = s.pv & xh;
    s.dist = (s.dist + ((ph & bound) != 0) - ((mh & bound) != 0)) & 0xFFu;
    ph <<= 1;
    mh <<= 1;
    s.pv = mh | ~(xv | ph);
    s.mv = ph & xv;
}
// State::adjust_one_up / adjust_up_by, myers_impl.rs:70-77, 97-103
__host__ __device__ __forceinline__ void my_one_up(MyState& s, uint64_t pos_mask) {
    if (s.pv & pos_mask)
        s.dist = (s.dist - 1) & 0xFFu;
    else if (s.mv & pos_mask)
        s.dist = (s.dist + 1) & 0xFFu;
}
__host__ __device__ __forceinline__ void my_up_by(MyState& s, uint64_t range_mask) {
    s.dist = (s.dist + __builtin_popcountll(s.mv & range_mask) - __builtin_popcountll(s.pv & range_mask)) & 0xFFu;
}

struct MyScratch {
    uint64_t* pv;
    uint64_t* mv;
    uint8_t* dist;
    uint64_t pitch, lane;
    __host__ __device__ __forceinline__ void put(uint32_t slot, const MyState& s) const {
        const uint64_t i = (uint64_t)slot * pitch + lane;
        pv[i] = s.pv;
        mv[i] = s.mv;
        dist[i] = (uint8_t)s.dist;
    }
    __host__ __device__ __forceinline__ MyState get(uint32_t slot) const {
        const uint64_t i = (uint64_t)slot * pitch + lane;
        return MyState{pv[i], mv[i], dist[i]};
    }
};

// _traceback_at (traceback.rs:235-318) with ShortTracebackHandler (simple.rs:202-297) from the column in slot `pos`; the
// next column to the left of slot s is slot s - 1, and `wrap` (the ring's size; 0: no ring) after slot 0, the reference's
// chain + cycle.  Operations go out in reverse, from ops_end - 1 down, while they fit `cap`.  Returns the aligned columns.
__host__ __device__ inline uint32_t my_traceback(const MyScratch& S, uint32_t pos, uint32_t wrap, uint32_t m, uint8_t* ops_end, uint64_t cap,
                                 uint32_t& n_ops, bool& broken) {
    uint64_t pos_mask = 1ull << (m - 1);
    const uint64_t max_mask = pos_mask;
    uint64_t left_adj = pos_mask;
    uint32_t cur = pos;
    auto next_state = [&]() {
        if (cur == 0) {
            if (wrap == 0) {
                broken = true;  // a path left of the max-state column: cannot happen (the initial column only moves up)
                return S.get(0);
            }
            cur = wrap;
        }
        cur--;
        return S.get(cur);
    };
    MyState block = S.get(pos);
    MyState left = next_state();
    my_one_up(left, pos_mask);
    uint32_t h = 0, n = 0;
    // every turn clears a bit of pos_mask or moves one column left: at most m + (m + dist) <= 3 m turns
    for (uint32_t turn = 0; pos_mask && turn < 3 * 64 + 4; turn++) {
        uint8_t op;
        bool move_left = true;
        if (((left.dist + 1) & 0xFFu) == block.dist) {  // Subst
            left_adj = (left_adj >> 1) | max_mask;
            pos_mask >>= 1;
            op = BG_OP_SUBST;
        } else if (block.pv & pos_mask) {  // try_move_up: Ins
            my_one_up(block, pos_mask);
            pos_mask >>= 1;
            left_adj = (left_adj >> 1) | max_mask;
            my_one_up(left, pos_mask);
            op = BG_OP_INS;
            move_left = false;
        } else if (left.mv & pos_mask) {  // try_prepare_left: Del
            left.dist = (left.dist - 1) & 0xFFu;
            op = BG_OP_DEL;
        } else {  // Match
            left_adj = (left_adj >> 1) | max_mask;
            pos_mask >>= 1;
            op = BG_OP_MATCH;
        }
        if (move_left) {  // finish_move_left
            h++;
            block = left;
            left = next_state();
            my_up_by(left, left_adj);
        }
        if (ops_end && n < cap) ops_end[-(int64_t)n - 1] = op;
        n++;
    }
    if (pos_mask) broken = true;
    n_ops = n;
    return h;
}

// cls[256] and the group's peq[pl][class] into LDS; returns false for the lanes past the launch's range
struct MyJob {
    uint64_t job, lane;
    uint32_t m, pl, ylen;
    const uint8_t* tb;
    const uint8_t* te;
};
__device__ __forceinline__ bool my_setup(const MyArgs& a, uint64_t* l_peq, uint8_t* l_cls, MyJob& j) {
    for (uint32_t i = threadIdx.x; i < a.gn * a.n_cls; i += MY_BLOCK) l_peq[i] = a.peqc[(uint64_t)a.g0 * a.n_cls + i];
    for (uint32_t i = threadIdx.x; i < 256; i += MY_BLOCK) l_cls[i] = a.cls[i];
    __syncthreads();
    const uint64_t idx = a.i0 + (uint64_t)blockIdx.x * MY_BLOCK + threadIdx.x;
    if (idx >= a.i1) return false;
    const uint64_t t = idx % a.n_texts;
    j.pl = (uint32_t)(idx / a.n_texts);
    j.job = t * a.n_pat + a.g0 + j.pl;
    j.lane = idx - a.i0;
    j.m = a.pm[a.g0 + j.pl];
    const uint64_t b = a.off[t], e = a.off[t + 1];
    j.tb = a.text + b;
    j.te = a.text + e;
    j.ylen = (uint32_t)(e - b);
    return true;
}

// one job of the best call; peq: the job's pattern's words by class, l_cls: the byte classes (both in LDS)
__host__ __device__ inline void my_best_job(const MyArgs& a, const MyJob& j, const uint64_t* peq, const uint8_t* l_cls) {
    const uint32_t m = j.m, n = j.ylen;
    const uint64_t bound = 1ull << (m - 1);
    // pass 1: the smallest distance at most k and its first end (find_all ... min_by_key)
    uint32_t best = 256, best_end = 0;
    {
        MyState s{~0ull, 0, m};
        MyText tx(j.tb, j.te);
        for (uint32_t i = 0; i < n; i++) {
            my_step(peq[l_cls[tx.next()]], bound, s);
            if (s.dist <= a.k && s.dist < best) {
                best = s.dist;
                best_end = i;
            }
        }
    }
    if (best == 256) {
        a.aln[j.job] = my_no_hit(m, n);
        return;
    }
    // pass 2: the columns a traceback from best_end can reach.  Virtual column v: 0 the max state, 1 the initial state,
    // i + 2 the text's column i; kept are the last R = m + min(k, m) + 2 up to v_e, in slot v - v_lo.
    const MyScratch S{a.s_pv, a.s_mv, a.s_dist, a.pitch, j.lane};
    const uint32_t R = m + (a.k < m ? a.k : m) + 2;
    const uint64_t v_e = (uint64_t)best_end + 2;
    const uint64_t v_lo = v_e >= R - 1 ? v_e - (R - 1) : 0;
    {
        MyState s{~0ull, 0, 255};
        if (v_lo == 0) S.put(0, s);
        s.dist = m;
        if (v_lo <= 1) S.put((uint32_t)(1 - v_lo), s);
        MyText tx(j.tb, j.te);
        for (uint32_t i = 0; i <= best_end; i++) {
            my_step(peq[l_cls[tx.next()]], bound, s);
            const uint64_t v = (uint64_t)i + 2;
            if (v >= v_lo) S.put((uint32_t)(v - v_lo), s);
        }
    }
    uint32_t n_ops = 0;
    bool broken = false;
    uint8_t* slot_end = a.ops ? a.ops + (j.job + 1) * a.ops_stride : nullptr;
    const uint32_t h = my_traceback(S, (uint32_t)(v_e - v_lo), 0, m, slot_end, a.ops_stride, n_ops, broken);
    bg_alignment_t r = my_hit(m, n, best_end + 1 - h, best_end + 1, best);
    my_set_ops(r, n_ops, broken, a.ops, a.ops_stride, j.job, a.flag);
    a.aln[j.job] = r;
}

// one job of the find-all call
template <bool ENDS_ONLY>
__host__ __device__ inline void my_find_all_job(const MyArgs& a, const MyJob& j, const uint64_t* peq, const uint8_t* l_cls) {
    const uint32_t m = j.m, n = j.ylen;
    const uint64_t bound = 1ull << (m - 1);
    const MyScratch S{a.s_pv, a.s_mv, a.s_dist, a.pitch, j.lane};
    const uint32_t R = m + (a.k < m ? a.k : m) + 2;  // the reference's ring (myers_impl.rs:327, traceback.rs:162)
    bg_alignment_t* out = a.aln + j.job * a.max_hits;
    MyState s{~0ull, 0, 255};
    uint32_t pos = 1;  // ring slot of the newest column
    if (!ENDS_ONLY) {
        S.put(0, s);
        s.dist = m;
        S.put(1, s);
    }
    s.dist = m;
    uint32_t found = 0;
    MyText tx(j.tb, j.te);
    for (uint32_t i = 0; i < n; i++) {
        my_step(peq[l_cls[tx.next()]], bound, s);
        if (!ENDS_ONLY) {
            pos = pos + 1 == R ? 0 : pos + 1;
            S.put(pos, s);
        }
        if (s.dist <= a.k) {
            if (found < a.max_hits) {
                uint32_t h = 0;
                bg_alignment_t r;
                if (!ENDS_ONLY) {
                    uint32_t n_ops = 0;
                    bool broken = false;
                    h = my_traceback(S, pos, R, m, nullptr, 0, n_ops, broken);
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

__global__ __launch_bounds__(MY_BLOCK) void myers_best_kernel(MyArgs a) {
    extern __shared__ uint64_t l_peq[];
    uint8_t* l_cls = (uint8_t*)(l_peq + (size_t)a.gn * a.n_cls);
    MyJob j;
    if (!my_setup(a, l_peq, l_cls, j)) return;
    my_best_job(a, j, l_peq + (size_t)j.pl * a.n_cls, l_cls);
}
template <bool ENDS_ONLY>
__global__ __launch_bounds__(MY_BLOCK) void myers_find_all_kernel(MyArgs a) {
    extern __shared__ uint64_t l_peq[];
    uint8_t* l_cls = (uint8_t*)(l_peq + (size_t)a.gn * a.n_cls);
    MyJob j;
    if (!my_setup(a, l_peq, l_cls, j)) return;
    my_find_all_job<ENDS_ONLY>(a, j, l_peq + (size_t)j.pl * a.n_cls, l_cls);
}

}  // namespace

void bg_myers_scratch_free(bg_myers_scratch* s) {
    if (!s) return;
    if (s->h) hipHostFree(s->h);
    hipFree(s->d);
    hipFree(s->d_flag);
    delete s;
}

namespace {

struct MyTables {
    std::vector<uint8_t> blob;  // peqc[n_pat][n_cls] (uint64), pm[n_pat] (uint32), cls[256]
    uint32_t n_cls = 0, max_m = 0, max_ring = 0;
    size_t off_pm = 0, off_cls = 0;
};

int my_check(const bg_myers_pattern_t* pats, uint32_t n_pat) {
    if (!pats || n_pat == 0) return BG_ERR_INVALID_ARG;
    if (n_pat > BG_MYERS_MAX_PATTERNS) return BG_ERR_TOO_LARGE;
    for (uint32_t p = 0; p < n_pat; p++) {
        if (pats[p].m == 0) return BG_ERR_INVALID_ARG;  // "Pattern is empty"
        if (pats[p].m > 64) return BG_ERR_TOO_LARGE;    // "Pattern too long"
    }
    return BG_OK;
}

// the patterns' peq words by class of text byte (bits at or above m do not count)
void my_tables(const bg_myers_pattern_t* pats, uint32_t n_pat, uint32_t k, MyTables& T) {
    uint8_t cls[256];
    std::vector<MyRow> rows(n_pat);
    for (uint32_t p = 0; p < n_pat; p++) rows[p] = MyRow{pats[p].peq, pats[p].m == 64 ? ~0ull : (1ull << pats[p].m) - 1};
    std::vector<std::vector<uint64_t>> cols;
    my_classes(rows, cls, cols);
    T.n_cls = (uint32_t)cols.size();
    T.off_pm = (size_t)n_pat * T.n_cls * 8;
    T.off_cls = T.off_pm + (size_t)n_pat * 4;
    T.blob.assign(T.off_cls + 256, 0);
    uint64_t* peqc = (uint64_t*)T.blob.data();
    uint32_t* pm = (uint32_t*)(T.blob.data() + T.off_pm);
    for (uint32_t p = 0; p < n_pat; p++) {
        for (uint32_t c = 0; c < T.n_cls; c++) peqc[(size_t)p * T.n_cls + c] = cols[c][p];
        const uint32_t m = pats[p].m;
        pm[p] = m;
        T.max_m = std::max(T.max_m, m);
        T.max_ring = std::max(T.max_ring, m + std::min(k, m) + 2);
    }
    memcpy(T.blob.data() + T.off_cls, cls, 256);
}

int my_run(bg_ctx* ctx, const bg_myers_pattern_t* pats, uint32_t n_pat, const MyCall& c, hipStream_t st) {
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);
    MyTables T;
    my_tables(pats, n_pat, c.k, T);
    if (int rc = my_upload(ctx, T.blob, 0, st)) return rc;
    bg_myers_scratch* M = ctx->myers;
    const bool need_scratch = !(c.find_all && c.ends_only);
    const bool may_overflow = !c.find_all && c.d_ops && c.ops_stride < 2ull * T.max_m;
    if (may_overflow) BG_HIP(hipMemsetAsync(M->d_flag, 0, sizeof(int), st));
    // jobs per launch: the traceback columns of one launch stay within 256 MB
    const uint64_t per_job = 17ull * T.max_ring;
    uint64_t chunk = ctx->myers_chunk_jobs > 0 ? (uint64_t)ctx->myers_chunk_jobs : (256ull << 20) / per_job;
    chunk = std::max<uint64_t>(MY_BLOCK, (chunk + MY_BLOCK - 1) / MY_BLOCK * MY_BLOCK);
    // patterns per group: their class tables within the LDS budget
    const uint64_t lds = ctx->myers_lds_bytes > 0 ? (uint64_t)ctx->myers_lds_bytes : 48u << 10;
    const uint32_t gmax = (uint32_t)std::max<uint64_t>(1, (lds - 256) / (8ull * T.n_cls));
    MyArgs a = {};
    a.text = c.d_text;
    a.off = c.d_off;
    a.n_texts = c.n_texts;
    a.peqc = (const uint64_t*)M->d;
    a.pm = (const uint32_t*)(M->d + T.off_pm);
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
    for (uint32_t g0 = 0; g0 < n_pat; g0 += gmax) {
        a.g0 = g0;
        a.gn = std::min(gmax, n_pat - g0);
        const uint64_t total = c.n_texts * a.gn;
        const size_t lds_bytes = (size_t)a.gn * T.n_cls * 8 + 256;
        for (uint64_t i0 = 0; i0 < total; i0 += chunk) {
            a.i0 = i0;
            a.i1 = std::min(total, i0 + chunk);
            const uint64_t cnt = a.i1 - a.i0;
            if (need_scratch) {
                a.pitch = (cnt + 63) / 64 * 64;
                if (int rc = bg_reserve(&ctx->tb, &ctx->tb_bytes, (size_t)(per_job * a.pitch))) return rc;
                a.s_pv = (uint64_t*)ctx->tb;
                a.s_mv = a.s_pv + (size_t)T.max_ring * a.pitch;
                a.s_dist = (uint8_t*)(a.s_mv + (size_t)T.max_ring * a.pitch);
            }
            const dim3 grid((uint32_t)((cnt + MY_BLOCK - 1) / MY_BLOCK)), block(MY_BLOCK);
            if (!c.find_all)
                myers_best_kernel<<<grid, block, lds_bytes, st>>>(a);
            else if (c.ends_only)
                myers_find_all_kernel<true><<<grid, block, lds_bytes, st>>>(a);
            else
                myers_find_all_kernel<false><<<grid, block, lds_bytes, st>>>(a);
            BG_HIP(hipGetLastError());
        }
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

extern "C" int bg_myers_best_batch_dev(bg_ctx* ctx, const bg_myers_pattern_t* pats, uint32_t n_pat, uint32_t max_dist,
                                       uint64_t n_texts, const uint8_t* d_text, const uint64_t* d_off, bg_alignment_t* d_aln,
                                       uint8_t* d_ops, uint64_t ops_stride, void* stream) {
    if (int rc = my_check(pats, n_pat)) return rc;
    if (!ctx) return BG_ERR_INVALID_ARG;
    if (n_texts == 0) return BG_OK;
    if (!d_text || !d_off || !d_aln) return BG_ERR_INVALID_ARG;
    MyCall c;
    c.k = std::min(max_dist, 255u);
    c.n_texts = n_texts;
    c.d_text = d_text;
    c.d_off = d_off;
    c.d_aln = d_aln;
    c.d_ops = d_ops;
    c.ops_stride = ops_stride;
    return my_run(ctx, pats, n_pat, c, (hipStream_t)stream);
}

extern "C" int bg_myers_best_batch(bg_ctx* ctx, const bg_myers_pattern_t* pats, uint32_t n_pat, uint32_t max_dist,
                                   uint64_t n_texts, const uint8_t* text, const uint64_t* off, bg_alignment_t* aln, uint8_t* ops,
                                   uint64_t ops_stride) {
    if (int rc = my_check(pats, n_pat)) return rc;
    if (!ctx) return BG_ERR_INVALID_ARG;
    MyCall c;
    c.k = std::min(max_dist, 255u);
    c.n_texts = n_texts;
    c.ops_stride = ops_stride;
    return my_host(ctx, n_pat, c, text, off, aln, nullptr, ops,
                   [&](const MyCall& cc, hipStream_t st) { return my_run(ctx, pats, n_pat, cc, st); });
}

extern "C" int bg_myers_find_all_batch_dev(bg_ctx* ctx, const bg_myers_pattern_t* pats, uint32_t n_pat, uint32_t max_dist,
                                           uint32_t max_hits, uint32_t flags, uint64_t n_texts, const uint8_t* d_text,
                                           const uint64_t* d_off, bg_alignment_t* d_aln, uint32_t* d_count, void* stream) {
    if (int rc = my_check(pats, n_pat)) return rc;
    if (max_hits == 0 || max_hits > BG_MYERS_MAX_HITS || (flags & ~(uint32_t)BG_MYERS_ENDS_ONLY)) return BG_ERR_INVALID_ARG;
    if (!ctx) return BG_ERR_INVALID_ARG;
    if (n_texts == 0) return BG_OK;
    if (!d_text || !d_off || !d_aln || !d_count) return BG_ERR_INVALID_ARG;
    MyCall c;
    c.find_all = true;
    c.ends_only = (flags & BG_MYERS_ENDS_ONLY) != 0;
    c.k = std::min(max_dist, 255u);
    c.max_hits = max_hits;
    c.n_texts = n_texts;
    c.d_text = d_text;
    c.d_off = d_off;
    c.d_aln = d_aln;
    c.d_count = d_count;
    return my_run(ctx, pats, n_pat, c, (hipStream_t)stream);
}

extern "C" int bg_myers_find_all_batch(bg_ctx* ctx, const bg_myers_pattern_t* pats, uint32_t n_pat, uint32_t max_dist,
                                       uint32_t max_hits, uint32_t flags, uint64_t n_texts, const uint8_t* text,
                                       const uint64_t* off, bg_alignment_t* aln, uint32_t* count) {
    if (int rc = my_check(pats, n_pat)) return rc;
    if (max_hits == 0 || max_hits > BG_MYERS_MAX_HITS || (flags & ~(uint32_t)BG_MYERS_ENDS_ONLY)) return BG_ERR_INVALID_ARG;
    if (!ctx) return BG_ERR_INVALID_ARG;
    if (n_texts && !count) return BG_ERR_INVALID_ARG;
    MyCall c;
    c.find_all = true;
    c.ends_only = (flags & BG_MYERS_ENDS_ONLY) != 0;
    c.k = std::min(max_dist, 255u);
    c.max_hits = max_hits;
    c.n_texts = n_texts;
    return my_host(ctx, n_pat, c, text, off, aln, count, nullptr,
                   [&](const MyCall& cc, hipStream_t st) { return my_run(ctx, pats, n_pat, cc, st); });
}
