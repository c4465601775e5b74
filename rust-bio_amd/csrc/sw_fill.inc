// K1 — sw_fill_kernel<R, LP, SM>.  Included by its instantiation unit, sw_fill_k1.hip.
// Design notes: sw_kernels.h.  Reference: pairwise/mod.rs:597-843.
#include <type_traits>

#include "sw_kernels.h"

namespace bgsw {

template <int SM>
__device__ __forceinline__ int32_t sub_score(const SwScoring& sc, const int32_t* s_table,
                                             const int32_t* g_table, int alpha, uint32_t p,
                                             uint32_t q) {
    if (SM == SCORE_PARAMS) return p == q ? sc.match : sc.mismatch;  // MatchParams, mod.rs:208-217
    if (SM == SCORE_LDS) return s_table[p * alpha + q];
    return g_table[p * alpha + q];
}

// inclusive scan over the LP lanes of a group with combine(earlier, later) =
// later.v > earlier.v ? later : earlier  ("first maximum wins", the reference's strict '>')
template <int LP>
__device__ __forceinline__ void scan_first_max(int ll, int64_t& v, uint32_t& idx) {
#pragma unroll
    for (int off = 1; off < LP; off <<= 1) {
        const int64_t ov = __shfl_up(v, off, LP);
        const uint32_t oi = (uint32_t)__shfl_up((int)idx, off, LP);
        if (ll >= off && !(v > ov)) {
            v = ov;
            idx = oi;
        }
    }
}

// LOCAL: all four clip penalties are 0 (Aligner::local, mod.rs:995-999).  Then xclip_j == 0, the
// y-prefix-clip candidate yp+go+ge(i-1) <= 0 can never beat it (ties go to the earlier XCLIP_PREFIX),
// and the two running maxima need no penalty add.
// NARROW: every reachable score fits in 28 bits (checked by the host from the scoring and the
// lengths): the first-maximum selection of mod.rs:757-786 becomes one max over score<<3|priority keys.
// LF ("local, fast": the int32 sibling of K1p's flavour of that name, sw_fill_pk16.inc): Aligner::local (LOCAL) under
// MatchParams with gap_open < 0, mismatch < 0 <= match and reads of one strip (the caller checks all of it).  There no
// alignment a caller can see needs the x-suffix-clip fold of a column before n (DESIGN.md section 4; checked against the
// restatement of the reference on the CPU, a property test under tests/): the fill keeps no fold and publishes no
// Lx[j < n] (K2 fails loudly should a path ever ask for one), column n's fold is one more scan of the epilogue
// (EPI_FOLD_PRE).  I and D values carry their candidate priority with them (score << 4 | priority << 1 | opened: K3i's
// keys, banded_fill2i.hip) — no clearing and or-ing per cell — and Sn / Ly are kept per block of 16 steps (one or and
// one max per cell).  Traceback cells: TBF_K1_LF — six 5-bit cells per word like TBF_K1, each I opened | move << 1 |
// D opened << 4.
#ifndef K1_WAVES  // wavefronts per SIMD K1 is compiled for (0: the compiler's choice — 233 VGPRs, two wavefronts, for R = 10; variant
#define K1_WAVES 0  // builds: tools/exp/ko_build.sh sw_fill_k1.hip k1w3 -DK1_WAVES=3)
#endif
#if K1_WAVES
#define K1_OCC __attribute__((amdgpu_waves_per_eu(K1_WAVES, K1_WAVES)))
#else
#define K1_OCC
#endif
template <int R, int LP, int SM, bool LOCAL, bool NARROW, bool LF = false>
__global__ __launch_bounds__(256) K1_OCC void sw_fill_kernel(const SwArgs a) {
    static_assert(!LF || (LOCAL && NARROW && SM == SCORE_PARAMS), "LF is a flavour of the local MatchParams kernel with scaled keys");
    constexpr int PW = 64 / LP;
    constexpr int NW = tb_words(R);
    static_assert((LP & (LP - 1)) == 0 && LP >= 16 && LP <= 64, "LP must be 16/32/64");
    static_assert(R >= 1 && R <= 12, "R rows per lane");

    __shared__ int32_t s_table[SM == SCORE_LDS ? kMaxLdsAlphabet * kMaxLdsAlphabet : 1];
    __shared__ uint8_t s_map[SM != SCORE_PARAMS ? 256 : 1];
    if (SM != SCORE_PARAMS) {
        for (uint32_t t = threadIdx.x; t < 256; t += blockDim.x) s_map[t] = a.code_map[t];
        if (SM == SCORE_LDS)
            for (int t = threadIdx.x; t < a.alpha * a.alpha; t += blockDim.x) s_table[t] = a.table[t];
        __syncthreads();
    }

    const int lane = threadIdx.x & 63;
    const uint32_t job = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if ((uint64_t)job * PW >= a.n_pairs) return;  // wave-uniform
    const int g = lane / LP, ll = lane % LP;
    const uint32_t pair = job * PW + g;
    const bool pair_ok = pair < a.n_pairs;
    const SwScoring sc = a.sc;
    const SwGeom geo = a.g;
    // NARROW kernels keep every DP value scaled by 16: the low 4 bits of a score are then free to
    // carry a priority (candidate order / row order), so that "first maximum wins" becomes a plain
    // integer max, and the open/extend decision of I and D rides in bit 3 of the winning value.
    constexpr int SH = NARROW ? 4 : 0;
    constexpr int32_t NEGS = NARROW ? (kNarrowFloor * 16) : NEG;  // scaled 'minus infinity'
    auto scl = [](int32_t v) -> int32_t { return NARROW ? (int32_t)((uint32_t)max(v, kNarrowFloor) << 4) : v; };
    const int32_t go_s = sc.go << SH, ge_s = sc.ge << SH;
    const int32_t xs_s = scl(sc.xs), ys_s = scl(sc.ys);
    const int32_t match_k = (sc.match << SH) | (int32_t)C_MATCH, mismatch_k = (sc.mismatch << SH) | (int32_t)C_SUBST;

    uint32_t m = 0, n = 0;
    const uint8_t* x = a.x;
    const uint8_t* y = a.y;
    if (pair_ok) {
        const uint64_t xo = a.x_off[a.pair0 + pair], yo = a.y_off[a.pair0 + pair];
        m = (uint32_t)(a.x_off[a.pair0 + pair + 1] - xo);
        n = (uint32_t)(a.y_off[a.pair0 + pair + 1] - yo);
        x += xo;
        y += yo;
        if (len_over(geo, m, n)) m = n = 0;  // beyond the caller's bounds: K2 reports it, nothing is computed
    }
    uint32_t m_w = m, n_w = n;  // wave-uniform loop bounds
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        m_w = max(m_w, (uint32_t)__shfl_xor((int)m_w, o));
        n_w = max(n_w, (uint32_t)__shfl_xor((int)n_w, o));
    }
    // all reads of this wavefront end on the last row of a lane (m % R == 0): see `cells` below
    constexpr bool FASTM = LOCAL && NARROW && SM == SCORE_PARAMS;
    const bool m_last = FASTM && __all(!pair_ok || m % R == 0);
    const uint32_t nstrips_w = max(1u, (m_w + LP * R - 1) / (LP * R));
    const uint32_t nsteps_w = n_w ? n_w + LP - 1 : 0;

    // tiled traceback layout, see tb_word_off()
    uint32_t* tb = (uint32_t*)a.tb + (size_t)job * tb_job_words(geo.nstrips, geo.nsteps, NW) + lane * 16u;
    int32_t* aux = a.aux + (size_t)(pair_ok ? pair : 0) * geo.aux_stride;
    int4* bnd = a.bnd + (size_t)(pair_ok ? pair : 0) * (geo.n_cap + 1);
    int32_t* gLy = aux + geo.off_Ly();
    int32_t* gLx = aux + geo.off_Lx();
    uint8_t* gBits = (uint8_t*)(aux + geo.off_bits());

    int32_t fold0;
    uint32_t lx0;
    col0_fold(sc, m, fold0, lx0);
    int32_t Sn0 = sc.ys;  // Sn[0], Ly[0] (mod.rs:618-619), carried by group lane 0 in strip 0
    uint32_t Ly0 = n;
    int32_t S0n = 0;            // S(0, n)
    uint32_t sb0n = TB_START;   // S nibble of (0, n) as the fill leaves it
    if (pair_ok && ll == 0) {
        aux[0] = m ? (int32_t)col0_cell(sc, m, m, fold0).sbits : (int32_t)TB_START;
        gLx[0] = (int32_t)lx0;
    }

    // ---- carries of the last-column epilogue across strips (group-uniform) ----
    int64_t e_carry = INT64_MIN;   // max over rows k handled so far of S1(k,n) - go*k
    uint32_t sbf_carry = TB_START; // fill-time S nibble of the last handled row of column n
    uint32_t sb2_carry = TB_START; // final S nibble of that row
    int64_t c1v = INT64_MIN, c2v = INT64_MIN;  // best x-suffix-clip candidates of the two epilogue loops
    uint32_t c1i = 0, c2i = 0;

    for (uint32_t strip = 0; strip < nstrips_w; strip++) {
        const uint32_t rb = (strip * LP + ll) * R;  // this lane owns rows rb+1 .. rb+R
        const int32_t mrow = (int32_t)m - (int32_t)rb - 1;  // r of row m inside this lane (if 0 <= mrow < R)
        int32_t Sl[R], Dl[R], Il[R], Sn[R], ycl[LOCAL ? 1 : R], SnB[LF ? R : 1];
        uint32_t Ly[R], px[R];
        constexpr int32_t kI = LF ? (int32_t)(C_INS << 1) : 0, kD = LF ? (int32_t)(C_DEL << 1) : 0;  // LF: I / D values carry these
        uint64_t nib0S = 0, nib0I = 0;  // column-0 S / I nibbles, 4 bits per row (only read when n == 0)
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t i = rb + r + 1;
            px[r] = 0;
            Sl[r] = Dl[r] = Il[r] = Sn[r] = NEGS;
            if (LF) {
                Dl[r] = NEGS | kD;
                SnB[r] = NEGS;
            }
            if (!LOCAL) ycl[LOCAL ? 0 : r] = NARROW ? kNarrowKeyFloor : NEG;
            Ly[r] = 0;
            if (pair_ok && i <= m) {
                const uint32_t ch = x[i - 1];
                px[r] = (SM == SCORE_PARAMS) ? ch : ((uint32_t)s_map[ch] | (ch << 8));  // class code | raw byte << 8
                const Col0 c = col0_cell(sc, i, m, fold0);
                Sl[r] = scl(c.S);
                Il[r] = scl(c.I);
                nib0S |= (uint64_t)c.sbits << (4 * r);
                nib0I |= (uint64_t)c.ibits << (4 * r);
                if (c.S + sc.ys > NEG) {  // mod.rs:667-670
                    Sn[r] = NARROW ? scl(c.S) + ys_s : c.S + sc.ys;
                    Ly[r] = n;
                }
                if (!LOCAL) {  // mod.rs:780-782
                    const int32_t yc = sc.yp + sc.go + sc.ge * ((int32_t)i - 1);
                    ycl[LOCAL ? 0 : r] = NARROW ? (int32_t)((uint32_t)scl(yc) | C_YP) : yc;
                }
            }
        }
        int32_t diag0 = (pair_ok && rb < m) ? scl(col0_S(sc, rb, m, fold0)) : NEGS;  // S(rb, 0)

        int32_t S_out = NEGS, I_out = NEGS | kI, cm_out = NEGS;
        int32_t ca_out = 0, q_out = 0;
        // LF: the block of 16 steps that ends at step s_end into (Sn, Ly): the winner sat at step s_end - its priority
        auto merge_rows = [&](const uint32_t s_end) {
            if (LF) {
                const int32_t nmj_end = (int32_t)n - ((int32_t)s_end + 1 - ll);  // n - j at step s_end
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int32_t nb = SnB[LF ? r : 0] & ~15;
                    const bool up = nb > Sn[r];
                    Ly[r] = up ? (uint32_t)(nmj_end + (SnB[LF ? r : 0] & 15)) : Ly[r];
                    Sn[r] = max(Sn[r], nb);
                    SnB[LF ? r : 0] = NEGS;
                }
            }
        };
        int32_t ychunk = 0, ychunk_nx = 0;
        int4 bch = make_int4(NEGS, NEGS, NEGS, 0), bch_nx = bch;
        uint32_t wlast[NW];  // traceback word of this lane's last column
#pragma unroll
        for (int w = 0; w < NW; w++) wlast[w] = 0;
        uint32_t lx_n = lx0;  // Lx[n] as the fill leaves it (row-m lane)
        if (pair_ok && (uint32_t)ll < n) {
            const uint32_t ch = y[ll];
            ychunk_nx = (SM == SCORE_PARAMS) ? ch : ((uint32_t)s_map[ch] | (ch << 8));
            if (strip) bch_nx = bnd[ll + 1];
        }

        for (uint32_t s = 0; s < nsteps_w; s++) {
            if (LF && s && (s & 15u) == 0) merge_rows(s - 1);
            if ((s & (LP - 1)) == 0) {  // wave-uniform: next LP columns of y (and of the row buffer)
                ychunk = ychunk_nx;
                bch = bch_nx;
                const uint32_t nb = s + LP + ll;
                if (pair_ok && nb < n) {
                    const uint32_t ch = y[nb];
                    ychunk_nx = (SM == SCORE_PARAMS) ? ch : ((uint32_t)s_map[ch] | (ch << 8));
                    if (strip) bch_nx = bnd[nb + 1];
                }
            }
            // values produced by the lane above one step ago (same column)
            int32_t S_up = wave_shr1(S_out), I_up = wave_shr1(I_out), cm = wave_shr1(cm_out);
            int32_t ca = wave_shr1(ca_out), q = wave_shr1(q_out);
            const uint32_t j = s + 1 - (uint32_t)ll;
            const bool col_ok = pair_ok && (j - 1) < n;  // 1 <= j <= n
            if (ll == 0) {
                q = ychunk;
                if (strip) {
                    S_up = bch.x;
                    I_up = bch.y;
                    cm = bch.z;
                    ca = bch.w;
                } else if (col_ok) {  // row 0 of the matrix, mod.rs:678-717
                    const Row0 c = row0_cell(sc, j);
                    int32_t S0 = c.S;
                    uint32_t sb = c.sbits;
                    if (j == n && Sn0 > S0) {
                        S0 = Sn0;
                        sb = TB_YCLIP_SUFFIX;
                    } else if (S0 + sc.ys > Sn0) {
                        Sn0 = S0 + sc.ys;
                        Ly0 = n - j;
                    }
                    S0n = S0;   // the last write is column n
                    sb0n = sb;
                    S_up = scl(S0);
                    I_up = NEGS | kI;  // mod.rs:681
                    cm = NEGS;    // S[curr][1..=m] reset, mod.rs:719-721
                    ca = 0;      // Lx[j] starts at 0
                }
            }
            ychunk = wave_shl1(ychunk);
            if (strip) {
                bch.x = wave_shl1(bch.x);
                bch.y = wave_shl1(bch.y);
                bch.z = wave_shl1(bch.z);
                bch.w = wave_shl1(bch.w);
            }

            if (col_ok) {
                // mod.rs:724-728
                const int32_t xclip_j = LOCAL ? 0 : sc.xp + max(sc.yp, sc.go + sc.ge * ((int32_t)j - 1));
                const int32_t xkey_j = (int32_t)((uint32_t)scl(xclip_j) | C_XP);
                const int32_t nmj = (int32_t)(n - j);
                int32_t diag = diag0;
                diag0 = S_up;
                uint32_t word[NW];
#pragma unroll
                for (int w = 0; w < NW; w++) word[w] = 0;
                const int32_t ca_in = ca;
                if (LF) {
                    const int32_t tpri = 15 - (int32_t)(s & 15u);
                    const int32_t go_ti = go_s + (kI | 1), go_td = go_s + (kD | 1);
                    const int32_t mk = (sc.match << SH) | (int32_t)(C_MATCH << 1), mmk = (sc.mismatch << SH) | (int32_t)(C_SUBST << 1);
                    constexpr int32_t xkey0 = (int32_t)(C_XP << 1);  // the floor of a local alignment: score 0, XCLIP_PREFIX
#pragma unroll
                    for (int r = 0; r < R; r++) {  // rows past m compute garbage nobody reads
                        const int32_t m_key = diag + (px[r] == (uint32_t)q ? mk : mmk);
                        const int32_t Iv_t = max(I_up + ge_s, S_up + go_ti);   // mod.rs:733-743
                        const int32_t Dv_t = max(Dl[r] + ge_s, Sl[r] + go_td);  // mod.rs:745-755
                        int32_t kb = max(max(m_key, Iv_t), max(Dv_t, xkey0));   // mod.rs:757-786
                        const int32_t best = kb & ~15;
                        diag = Sl[r];
                        Sl[r] = best;
                        Dl[r] = Dv_t & ~1;
                        Il[r] = Iv_t;  // (the epilogue clears the low bits of what it reads)
                        S_up = best;
                        I_up = Iv_t & ~1;
                        SnB[LF ? r : 0] = max(SnB[LF ? r : 0], best | tpri);  // mod.rs:799-802, per block of 16 steps
                        // I opened (bit 0 of its key) | move << 1 (bits 1-3 of the winner) | D opened << 4: two v_bfi_b32
                        uint32_t c1, c2;
                        asm("v_bfi_b32 %0, 1, %1, %2" : "=v"(c1) : "v"(Iv_t), "v"(kb));
                        asm("v_bfi_b32 %0, 16, %1, %2" : "=v"(c2) : "v"((uint32_t)Dv_t << 4), "v"(c1));
                        word[r / 6] |= (c2 & 31u) << (5 * (r % 6));
                    }
                } else if (NARROW) {
                    // fold key: clean running maximum | row priority (15 = an earlier lane)
                    int32_t cmk = cm | 15;
                    int32_t snap = cmk;  // the fold as row m sees it
                    const int32_t go_t = go_s + 8;  // "open" candidates carry bit 3: they win ties (strict '>')
                    // MRk >= 0: every pair of this wavefront has its row m at r == MRk (equal read lengths, the
                    // usual short-read case): the x-suffix-clip candidate drops out of the other rows' cells
                    auto cells = [&](auto mr_tag) {
                    constexpr int MRk = decltype(mr_tag)::value;
#pragma unroll
                    for (int r = 0; r < R; r++) {  // rows past m compute garbage nobody reads
                        const bool is_m = MRk < 0 ? (r == mrow) : (r == MRk && mrow == MRk);
                        // mod.rs:733-755
                        // substitution score with the MATCH/SUBST move code already in its low bits
                        const bool eq = (SM == SCORE_PARAMS) ? px[r] == (uint32_t)q : ((px[r] ^ (uint32_t)q) >> 8) == 0;
                        const int32_t f_k = (SM == SCORE_PARAMS)
                                                ? (eq ? match_k : mismatch_k)
                                                : ((sub_score<SM>(sc, s_table, a.table, a.alpha, px[r] & 255u, (uint32_t)q & 255u) << SH) |
                                                   (int32_t)(eq ? C_MATCH : C_SUBST));
                        const int32_t m_key = diag + f_k;
                        const int32_t Iv_t = max(I_up + ge_s, S_up + go_t);
                        const int32_t Dv_t = max(Dl[r] + ge_s, Sl[r] + go_t);
                        const int32_t Iv = Iv_t & ~15, Dv = Dv_t & ~15;
                        // mod.rs:757-786: first maximum wins == max over (score | priority)
                        const int32_t k_init = is_m ? (int32_t)(((uint32_t)cmk & ~15u) | C_XS) : kNarrowKeyFloor;
                        int32_t kb = max(max(k_init, m_key), (int32_t)((uint32_t)Iv | C_INS));
                        kb = max(max(kb, (int32_t)((uint32_t)Dv | C_DEL)), xkey_j);
                        if (!LOCAL) kb = max(kb, ycl[LOCAL ? 0 : r]);
                        const int32_t best = kb & ~15;
                        diag = Sl[r];
                        Sl[r] = best;
                        Dl[r] = Dv;
                        Il[r] = Iv;
                        S_up = best;
                        I_up = Iv;
                        snap = is_m ? cmk : snap;
                        // mod.rs:793-796
                        cmk = max(cmk, (int32_t)((uint32_t)(LOCAL ? best : best + xs_s) | (uint32_t)(14 - r)));
                        // mod.rs:799-802
                        const int32_t t1 = LOCAL ? best : best + ys_s;
                        Ly[r] = (t1 > Sn[r]) ? (uint32_t)nmj : Ly[r];
                        Sn[r] = max(Sn[r], t1);
                        // packed cell: 3-bit move | I extends << 3 | D extends << 4
                        const uint32_t cell = (((uint32_t)kb & 7u) | (((uint32_t)Dv_t & 8u) << 1) | ((uint32_t)Iv_t & 8u)) ^ 24u;
                        word[r / 6] |= cell << (5 * (r % 6));
                    }
                    };
                    if (FASTM && m_last)
                        cells(std::integral_constant<int, R - 1>{});
                    else
                        cells(std::integral_constant<int, -1>{});
                    const int32_t lo = cmk & 15, slo = snap & 15;
                    if (mrow >= 0 && mrow < R) {  // the lane that owns row m publishes Lx[j]
                        lx_n = slo == 15 ? (uint32_t)ca_in : (uint32_t)(mrow - 14 + slo);
                        gLx[j] = (int32_t)lx_n;
                    }
                    ca = lo == 15 ? ca_in : (mrow - 14 + lo);
                    cm = cmk & ~15;
                } else {
                    int32_t ca_loc = 0;   // r+1 of the last row of this lane that improved the fold
                    int32_t ca_snap = 0;  // ca_loc as row m saw it
#pragma unroll
                    for (int r = 0; r < R; r++) {  // rows past m compute garbage nobody reads
                        const bool is_m = (r == mrow);
                        // mod.rs:733-755
                        const bool eq = (SM == SCORE_PARAMS) ? px[r] == (uint32_t)q : ((px[r] ^ (uint32_t)q) >> 8) == 0;
                        const int32_t m_sc = diag + sub_score<SM>(sc, s_table, a.table, a.alpha, px[r] & 255u, (uint32_t)q & 255u);
                        const int32_t ie = I_up + sc.ge, io = S_up + sc.go;
                        const bool iext = ie > io;
                        const int32_t Iv = max(ie, io);
                        const int32_t de = Dl[r] + sc.ge, dop = Sl[r] + sc.go;
                        const bool dext = de > dop;
                        const int32_t Dv = max(de, dop);
                        // mod.rs:757-786 — strict '>' in this exact order = first maximum wins
                        const int32_t init = is_m ? cm : NEG;
                        int32_t best = max(max(max(init, m_sc), max(Iv, Dv)), xclip_j);
                        uint32_t code = C_XP;
                        if (!LOCAL) {
                            best = max(best, ycl[LOCAL ? 0 : r]);
                            code = C_YP;
                            code = (xclip_j == best) ? (uint32_t)C_XP : code;
                        }
                        code = (Dv == best) ? (uint32_t)C_DEL : code;
                        code = (Iv == best) ? (uint32_t)C_INS : code;
                        code = (m_sc == best) ? (uint32_t)(eq ? C_MATCH : C_SUBST) : code;
                        code = (init == best) ? (uint32_t)C_XS : code;
                        diag = Sl[r];
                        Sl[r] = best;
                        Dl[r] = Dv;
                        Il[r] = Iv;
                        S_up = best;
                        I_up = Iv;
                        ca_snap = is_m ? ca_loc : ca_snap;
                        // mod.rs:793-796 (the reference's check at i == m is a no-op: the snapshot
                        // above is taken before it, and nothing reads the fold after row m)
                        const int32_t t2 = LOCAL ? best : best + sc.xs;
                        ca_loc = (t2 > cm) ? (r + 1) : ca_loc;
                        cm = max(cm, t2);
                        // mod.rs:799-802
                        const int32_t t1 = LOCAL ? best : best + sc.ys;
                        Ly[r] = (t1 > Sn[r]) ? (uint32_t)nmj : Ly[r];
                        Sn[r] = max(Sn[r], t1);
                        word[r / 6] |= (code | (iext ? 8u : 0u) | (dext ? 16u : 0u)) << (5 * (r % 6));
                    }
                    if (mrow >= 0 && mrow < R) {  // the lane that owns row m publishes Lx[j]
                        lx_n = ca_snap ? (uint32_t)(mrow + 1 - ca_snap) : (uint32_t)ca_in;
                        gLx[j] = (int32_t)lx_n;
                    }
                    ca = ca_loc ? (mrow + 1 - ca_loc) : ca_in;
                }
                if (NW == 1)
                    tb[tb_word_off((uint64_t)strip * geo.nsteps + s, 0, NW)] = word[0];
                else
                    *(uint2*)&tb[tb_word_off((uint64_t)strip * geo.nsteps + s, 0, NW)] = make_uint2(word[0], word[NW - 1]);
#pragma unroll
                for (int w = 0; w < NW; w++) wlast[w] = word[w];
                S_out = S_up;
                I_out = I_up;
                cm_out = cm;
                ca_out = ca;
                q_out = q;
                if (ll == LP - 1 && strip + 1 < nstrips_w) bnd[j] = make_int4(S_up, I_up, cm, ca);
            }
        }

        // =========== epilogue of the last column for this strip's rows (mod.rs:808-843) ===========
        // Per row i (ascending over lanes): S1 = max'(S(i,n), Sn[i]) [YCLIP_SUFFIX];
        // first-loop fold candidate S1 + xs (rows < m, row 0 included);
        // second loop: s_score(i) = max_{k<i}(S1(k) - go*k) + go*i (a prefix maximum),
        // replaces S and marks INS where strictly greater, repairs the I nibble, and feeds the
        // second fold.  Row m is resolved by its owner lane once all candidates are known.
        // Nibbles are kept packed (4 bits per row) to stay out of the main loop's register budget.
        if (LF) {
            merge_rows((nsteps_w ? nsteps_w - 1 : 0u) | 15u);  // the last (partial) block: its missing steps added nothing
#pragma unroll
            for (int r = 0; r < R; r++) Il[r] &= ~15;
        }
        {
            // the packed cell of row r in column n, in TBF_K1's layout (move | I extended << 3 | D extended << 4)
            auto cell_of = [&](int r) -> uint32_t {
                const uint32_t v = (wlast[r / 6] >> (5 * (r % 6))) & 31u;
                return LF ? (((v >> 1) & 7u) | ((~v & 1u) << 3) | (~v & 16u)) : v;
            };
            constexpr bool EPI_FOLD_PRE = LF;  // K1 keeps the fold during the fill; its LF flavour leaves column n's to the epilogue
#include "sw_epilogue.inc"
        }
        if (nstrips_w > 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}

}  // namespace bgsw
