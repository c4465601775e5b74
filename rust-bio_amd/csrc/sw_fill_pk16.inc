// K1p — sw_fill_pk16_kernel<R, LP, clips>: the short-read variant of K1 (sw_fill.inc) for MatchParams scoring
// (pairwise/mod.rs:597-843) when every reachable score fits 12 bits.  Instantiated per clip pattern: local
// (mod.rs:995-999), semiglobal (963-967), global (934-938) and the general Aligner::custom.
//
// Same anti-diagonal wavefront, same keys (score << 4 | priority, "first maximum wins" == one integer
// max), but every VGPR holds TWO pairs: the DP values of pair A in bits 0-15 and of pair B in bits 16-31,
// combined with the packed-math VALU ops of CDNA (v_pk_add_i16 clamp, v_pk_max_i16, v_pk_mad_u16): one
// instruction advances a cell of both pairs.  K1 is bound by VALU issue (about 46 lane-instructions per
// cell), so halving the instructions per cell is the lever; HBM traffic per cell is unchanged.
// The two pairs of a lane group ("couple") are slots g of the wavefront jobs 2w and 2w+1; they share the
// lane-level control (column validity, the row that owns row m), so they must have equal lengths — a
// couple with different lengths is simply processed in two passes, each pair against itself.  On ragged
// batches the slots hold the pairs in (m, n) order (SwArgs::perm, built in sw_api.hip), so that couples of
// equal lengths are the rule.
// Traceback words: 3 cells x 5 bits (I extends | move << 1 | D extends << 4) per 16-bit half
// (SwGeom::tb_fmt == TBF_K1P), same tiles as K1.
#include <type_traits>

#include "sw_kernels.h"

#ifndef PK16_CELL_KO
#define PK16_CELL_KO 0
#endif

namespace bgsw {
namespace pk16 {

typedef uint32_t pk;  // two int16: [15:0] = first pair of the couple, [31:16] = second

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 as_s(pk v) { return __builtin_bit_cast(s16x2, v); }
__device__ __forceinline__ u16x2 as_u(pk v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ pk bits(s16x2 v) { return __builtin_bit_cast(pk, v); }
__device__ __forceinline__ pk bits(u16x2 v) { return __builtin_bit_cast(pk, v); }
// v_pk_add_i16 clamp / v_pk_max_i16 / v_pk_add_u16 / v_pk_sub_u16 [clamp] / v_pk_mad_u16
__device__ __forceinline__ pk pk_adds(pk a, pk b) { return bits(__builtin_elementwise_add_sat(as_s(a), as_s(b))); }
__device__ __forceinline__ pk pk_max(pk a, pk b) { return bits(__builtin_elementwise_max(as_s(a), as_s(b))); }
// v_pk_maximum3_f16: the integer maximum of three, bits untouched, while every half lies in [0, 0x7bff] — there the bit
// patterns are the non-negative finite halves (denormals included), which IEEE maximum orders as the integers do
__device__ __forceinline__ pk pk_max3h(pk a, pk b, pk c) {
    const h16x2 x = __builtin_bit_cast(h16x2, a), y = __builtin_bit_cast(h16x2, b), z = __builtin_bit_cast(h16x2, c);
    return __builtin_bit_cast(pk, __builtin_elementwise_maximum(__builtin_elementwise_maximum(x, y), z));
}
__device__ __forceinline__ pk pk_min(pk a, pk b) { return bits(__builtin_elementwise_min(as_s(a), as_s(b))); }
__device__ __forceinline__ pk pk_add_u16(pk a, pk b) { return bits((u16x2)(as_u(a) + as_u(b))); }
__device__ __forceinline__ pk pk_sub_u16(pk a, pk b) { return bits((u16x2)(as_u(a) - as_u(b))); }
__device__ __forceinline__ pk pk_subs_u16(pk a, pk b) { return bits(__builtin_elementwise_sub_sat(as_u(a), as_u(b))); }  // max(a - b, 0)
__device__ __forceinline__ pk pk_mad_u16(pk a, pk b, pk c) { return bits((u16x2)(as_u(a) * as_u(b) + as_u(c))); }
__device__ __forceinline__ pk dup16(int32_t v) { return ((uint32_t)v & 0xffffu) | ((uint32_t)v << 16); }
__device__ __forceinline__ pk bfi(pk mask, pk a, pk b) { return (a & mask) | (b & ~mask); }
// 0xffff in every half that is non-zero
__device__ __forceinline__ pk nz_mask(pk v, pk one) { return pk_sub_u16(pk_subs_u16(one, v), one); }

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

// v with the lanes of its row of 16 permuted by a DPP control (every lane of the wavefront active)
template <int CTRL>
__device__ __forceinline__ pk dpp_row(pk v) {
    return (pk)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false);
}
// Packed first maximum over the LP lanes of a pair, in every lane: each half of v is score | 15 - (lane % 16) with the score a
// multiple of 16, so the signed packed maximum over a row of 16 lanes keeps the earliest lane of the largest score.  Four
// DPP steps (lane ^ 1, lane ^ 2, mirror within 8, mirror within 16), no LDS round trip.  LP == 32 has no room for a fifth
// priority bit in a half: the two rows of 16 are reduced on their own and combined by one more packed maximum in which the
// lower row's score carries a 1 below the score bits, so it keeps ties; hi gets 16 in the halves the upper row won.
template <int LP>
__device__ __forceinline__ pk group_first_max(pk v, int ll, pk& hi) {
    constexpr pk CLEAN = 0xfff0fff0u, ONE = 0x00010001u;
    v = pk_max(v, dpp_row<0xb1>(v));   // quad_perm [1, 0, 3, 2]
    v = pk_max(v, dpp_row<0x4e>(v));   // quad_perm [2, 3, 0, 1]
    v = pk_max(v, dpp_row<0x141>(v));  // row_half_mirror
    v = pk_max(v, dpp_row<0x140>(v));  // row_mirror
    hi = 0;
    if (LP == 32) {
        const pk o = (pk)__shfl_xor((int)v, 16);
        const pk lo_v = ll < 16 ? v : o, up_v = ll < 16 ? o : v;
        const pk lowwin = nz_mask(pk_max((lo_v & CLEAN) | ONE, up_v & CLEAN) & ONE, ONE);
        v = bfi(lowwin, lo_v, up_v);
        hi = ~lowwin & 0x00100010u;
    }
    return v;
}

constexpr int32_t kFloor16 = -2048;  // 'minus infinity' of the 12-bit score range (scaled: 0x8000)

// FAST: the wavefronts whose pairs all end on the last row of a lane (m % R == 0, the usual equal-length
// short reads), first pass only.  !FAST: launched right after it on the same grid, picks up what FAST left —
// the other wavefronts, and the second pair of every couple whose lengths differ.  Both derive the split
// from the lengths alone, so no flags travel between the two launches.
// How a clip penalty enters the kernel: CZ it is 0 (no add), CI it is MIN_SCORE (its candidate does not
// exist: nothing is computed for it), CF anything (adds, with MIN_SCORE mapped below every real value).
enum { CZ = 0, CF = 1, CI = 2 };
// MODE (three launches on the same grid, each without a loop over passes — a loop costs ~100 VGPRs here):
//   0 "fast"  first pass of the wavefronts whose pairs all end on the last row of a lane (m % R == 0);
//   1 "rest"  first pass of the other wavefronts (any m: the row that owns row m is found at run time);
//   2 "second" the second pair of every couple whose lengths differ, in any wavefront.
// LF ("local, fast"): Aligner::local with gap_open < 0 and mismatch < 0 (the caller checks both).  There the fill keeps
// no x-suffix-clip fold at all (DESIGN.md §4 "what local alignments do not need"): every value of row m that descends
// from a fold of a column before n is <= the best cell of the rows above, which the last column's folds offer to (m, n)
// anyway, with priority, and a gap on top makes it strictly smaller — so no cell of row m needs the candidate, and no
// Lx[j < n] is ever asked for; the fold of column n itself (over the fill's S(1..m-1, n), before the y-suffix clip:
// mod.rs:793-796 at j == n) is one more first maximum of the LF flavours' own last-column epilogue (below), which has
// those values in hand.  That takes two instructions out of every cell, the fold's carry, Lx and the clip candidate
// of row m out of every step, and makes every wavefront a "fast" one (row m is nothing special during the fill: one
// launch).  The local floor 0 (the x-prefix-clip candidate, mod.rs:765-768) comes out of the unsigned saturation of the
// substitution score instead of one more maximum — the move code of such a cell is 0, which K2 and the epilogue read as
// C_XP (SwGeom::tb_fmt == TBF_K1P_LF).
// FR (LF only, where pk16_frame_fits): the keys live in an offset frame, K^ = K + B + g (r + s) with r the row within the
// lane, s the step, g = 16 |ge| and B = pk16_frame_bias (sw_kernels.h).  A gap extension is then no instruction at all
// (I^(r, s) = I^(r - 1, s), D^(r, s) = D^(r, s - 1)), the opens and the diagonal differ from their sources by constants,
// and since every key of the frame lies in [0, 0x7fff] those constants go on with full-rate 32-bit adds, one per cell
// for both pairs (no half ever carries into the other): four v_pk_add_i16 clamp per cell become two v_add_u32.  The
// local floor 0 becomes the per-(row, step) constant F(r, s) = B + g (r + s), one more maximum; the row maxima SnB leave
// the frame as they are taken (best^ - F + priority, one subtract instead of the or), and so do Sl / Il when they are
// parked: the epilogue, the traceback cells and K2 see what the plain LF cell gives them.  The values crossing to the lane
// below (row R - 1 there, row -1 here) are re-based by g (R - 1), and 0 is 'minus infinity' of I and D.
// FR == 2 (where pk16_max3_fits: every key of the frame below 0x7c00, half precision's +inf, and pk16_delta <= 256): the
// same keys with maxima of three (v_pk_maximum3_f16, pk_max3h) and three things the result does not need left out.
//  - The floor enters through D: D' = max3(D, S + open, F(r, s)) replaces D's v_pk_max_i16, and the best key is one
//    max3(m_key, D', I).  A gap extension is free in the frame and F rises by g per step, so a floored D is F(r, s) <=
//    F(r, s + 1) one step on and never passes the floor it meets there: by induction D'(r, s) = max(D(r, s), F(r, s)), the
//    candidates of the best key are what they were, and since F's low nibble is 0 so is the key, move code included (on
//    equal scores D's nibble wins, as before).  What differs from FR == 1 is Dl and the "D opens" bit of the traceback cell
//    where D < F strictly.  K2 reads that bit only while it walks in state D (the epilogue never does); a path enters D in
//    a cell where D won the best key, so D >= F there, and every cell further back along the gap holds the same D^
//    against a smaller F: cells whose bit differs are cells no walk visits in state D.  Records and operations are
//    those of FR == 1 bit for bit; the traceback words are not.
//  - The symbols px[] / q sit in the high byte of their halves (shifted once at set-up and once per y_pair load), so
//    px ^ q is 0 or >= 256 >= DELTA in each half and the match term is pk_subs_u16(DELTA, px ^ q): the v_pk_mad_u16 by
//    DELTA becomes a full-rate add.
//  - The row maxima SnB of the two steps of a trip of the unpredicated loop are taken in the second step by one
//    max3(SnB, best(s - 1) - c(s - 1), best(s) - c(s)); best(s - 1) is still in Sl[r] there.  Trips start on even steps,
//    so both steps share a 16-step priority block, merge_rows (s % 16 == 15) follows a second step, and the first step's
//    key carries an odd priority: it is never 0, so the result does not depend on how maximum orders SnB's initial
//    0x8000 (-0.0 as a half) against key 0 (+0.0).  In unpredicated steps every lane and row, those past m included, holds
//    keys of the frame: no NaN pattern reaches a maximum.
template <int R, int LP, int MODE, int XP, int XS, int YP, int YS, bool LF = false, int FR = 0>
__device__ __forceinline__ void sw_fill_pk16_body(const SwArgs& a) {
    constexpr bool FAST = MODE == 0;
    constexpr int PW = 64 / LP;
    constexpr int NW = tb_words(R);
    constexpr int NH = (R + 2) / 3;  // 16-bit halves of traceback cells per pair and step
    constexpr bool NARROW = true, LOCAL = XP == CZ && XS == CZ && YP == CZ && YS == CZ;
    constexpr bool ROW0_ZERO = YP == CZ && YS == CZ;  // S(0,j) = 0 by YCLIP_PREFIX, Sn[0] stays 0 (mod.rs:678-717)
    constexpr int SH = 4;
    constexpr int32_t NEGS = kFloor16 * 16;
    constexpr pk CLEAN = 0xfff0fff0u, FLOORK = 0x80008000u, ONE = 0x00010001u;
    static_assert(LP == 16 || LP == 32, "lanes per pair");
    static_assert(R >= 1 && R <= 12, "rows per lane");
    static_assert(!LF || LOCAL, "LF is a flavour of the local kernel");
    static_assert(FR >= 0 && FR <= 2 && (!FR || LF), "the frame is a cell of the LF flavour");
    (void)NARROW;
    (void)LOCAL;
    // LDS, two uses that never overlap in time: during the fill, the traceback words of the current tile (a
    // lane's 64 bytes per pair, kTileStride dwords apart: 8-byte writes, 16-byte aligned reads); after it, the
    // packed rows parked for the epilogue
    constexpr int kTileStride = 20;
    // (LF parks S, Sn, Ly and the last column's cells; the others I and Lx[n] as well)
    constexpr int kParkDw = LF ? 64 * (3 * R + NH) : 64 * (4 * R + NH + 1), kTileDw = 2 * 64 * kTileStride;  // per wavefront
    constexpr int kWaveDw = kParkDw > kTileDw ? kParkDw : kTileDw;
    __shared__ __align__(16) pk s_lds[4 * kWaveDw];
    pk* const wave_lds = s_lds + (threadIdx.x >> 6) * kWaveDw;  // wavefronts of a block run unsynchronised

    const int lane = threadIdx.x & 63;
    const uint32_t wv = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if ((uint64_t)wv * 2 * PW >= a.n_pairs) return;  // wave-uniform
    // a sub-batch of one length has no unequal couple: the "second" launch leaves before it loads a pair's offsets
    if (MODE == 2 && a.len_stats && a.len_stats[0] == a.len_stats[2] && a.len_stats[1] == a.len_stats[3]) return;
    const int g = lane / LP, ll = lane % LP;
    const SwScoring sc = a.sc;
    const SwGeom geo = a.g;
    auto scl = [](int32_t v) -> int32_t { return max(v, kFloor16) * 16; };
    // the epilogue works on sign-extended 32/64-bit values: there 'minus infinity' has room to stay below
    // every real value after an add
    const int32_t go_s = sc.go * 16, xs_s = sc.xs <= kFloor16 ? -(1 << 30) : sc.xs * 16;
    (void)xs_s;
    // Keys: score << 4 | move code << 1 | "opens".  The I and D values keep their move code in the low bits
    // (bit 0, the open/extend decision, is cleared when they are stored), so they enter the cell's maximum
    // as they are; bit 0 sits below the code and only ever decides between the two candidates of one value
    // (open wins ties, like the reference's strict '>' for extend, mod.rs:738,749).
    constexpr int32_t K_XS = C_XS << 1, K_MATCH = C_MATCH << 1, K_SUBST = C_SUBST << 1, K_INS = C_INS << 1,
                      K_DEL = C_DEL << 1, K_XP = C_XP << 1;
    constexpr pk NOFLAG = 0xfffefffeu;
    const pk GE = dup16(sc.ge * 16);
    const pk GOT_I = dup16(sc.go * 16 + K_INS + 1), GOT_D = dup16(sc.go * 16 + K_DEL + 1);
    const pk MISK = dup16((sc.mismatch * 16) | K_SUBST);
    const pk DELTA = dup16(((sc.match * 16) | K_MATCH) - ((sc.mismatch * 16) | K_SUBST));
    // x-suffix-clip fold and row maxima add a clip penalty to a cell value: MIN_SCORE would land inside the
    // 16-bit range, so the sum is capped at the floor instead (CF only)
    const pk XS16 = dup16(scl(sc.xs)), YS16 = dup16(scl(sc.ys));
    const pk XSCAP = sc.xs <= kFloor16 ? FLOORK : 0x7fff7fffu, YSCAP = sc.ys <= kFloor16 ? FLOORK : 0x7fff7fffu;
    (void)XS16; (void)YS16; (void)XSCAP; (void)YSCAP;
    // -(mismatch | K_SUBST) as an unsigned amount (LF: mismatch <= -1)
    const pk MISC = dup16(-((sc.mismatch * 16) | K_SUBST));
    (void)MISC;
    // FR: fr(c) adds c to both halves with one 32-bit add (exact while each half stays inside [0, 0xffff]; any c)
    auto fr = [](int32_t c) -> pk { return (uint32_t)c * 0x10001u; };
    const int32_t gF = -16 * sc.ge, BF = pk16_frame_bias(sc);
    const pk GF = fr(gF);
    const pk KGOI = fr(sc.go * 16 + K_INS + 1 + gF), KGOD = fr(sc.go * 16 + K_DEL + 1 + gF);  // opens: one row / step on
    const pk KSUB = fr(((sc.mismatch * 16) | K_SUBST) + 2 * gF);                                // diagonal: both
    const pk KREB = fr(gF * (R - 1));  // row R - 1 of the lane above at step s -> row -1 here at step s + 1
    (void)GF; (void)KGOI; (void)KGOD; (void)KSUB; (void)KREB;
    // the three savings of the FR == 2 cell (see above); PK16_CELL_KO knocks them out one by one for timing builds
    // (tools/exp/ko_build.sh sw_fill_pk16_localfast.hip <name> -DPK16_CELL_KO=<bits>; results stay the same)
    constexpr bool DFLOOR = FR == 2 && !(PK16_CELL_KO & 1);   // the floor enters through D
    constexpr bool SYMHI = FR == 2 && !(PK16_CELL_KO & 2);    // symbols in the high byte, match term by one saturating subtract
    constexpr bool ROWMAX2 = FR == 2 && !(PK16_CELL_KO & 4);  // row maxima of a two-step trip by one maximum of three
    constexpr int SYM_SH = SYMHI ? 8 : 0;
    // ceilings of the once-per-wavefront code of the LF flavours (timing only, WRONG results): bit 4 leaves right after the last
    // tile store (no last-column epilogue), bit 5 starts every row from constants (no col0_cell set-up)
    constexpr bool KO_EPILOGUE = LF && (PK16_CELL_KO & 16), KO_SETUP = LF && (PK16_CELL_KO & 32);
    // the traceback cells are put together with v_pk_mad_u16; the factors are hidden from the compiler, which
    // otherwise rewrites every multiply-add by a power of two into a shift and an add (two instructions for one)
    pk C16 = dup16(16), C32 = dup16(32), C1024 = dup16(1024);
    asm volatile("" : "+s"(C16), "+s"(C32), "+s"(C1024));

    // ---- the couple of this lane group
    const uint32_t pA = (2 * wv) * PW + g, pB = (2 * wv + 1) * PW + g;
    const bool okA = pA < a.n_pairs, okB = pB < a.n_pairs;
    uint32_t mA = 0, nA = 0, mB = 0, nB = 0;
    uint64_t xoA = 0, yoA = 0, xoB = 0, yoB = 0;
    // pA / pB are SLOTS of the sub-batch (traceback words, aux records); the pairs in them come through a.perm
    const uint32_t* perm = a.slot_perm();
    if (okA) {
        const uint64_t r = a.pair0 + (perm ? perm[pA] : pA);
        xoA = a.x_off[r];
        yoA = a.y_off[r];
        mA = (uint32_t)(a.x_off[r + 1] - xoA);
        nA = (uint32_t)(a.y_off[r + 1] - yoA);
        if (len_over(geo, mA, nA)) mA = nA = 0;  // beyond the caller's bounds: K2 reports it, nothing is computed
    }
    if (okB) {
        const uint64_t r = a.pair0 + (perm ? perm[pB] : pB);
        xoB = a.x_off[r];
        yoB = a.y_off[r];
        mB = (uint32_t)(a.x_off[r + 1] - xoB);
        nB = (uint32_t)(a.y_off[r + 1] - yoB);
        if (len_over(geo, mB, nB)) mB = nB = 0;
    }
    const bool same = okA && okB && mA == mB && nA == nB;
    const bool two = okA && okB && !same;
    const bool m_last0 = LF || __all(!okA || mA % R == 0);  // LF: one launch takes every wavefront
    if (MODE == 0 && !m_last0) return;   // wave-uniform
    if (MODE == 1 && m_last0) return;    // the fast launch did it
    if (MODE == 2 && !__any(two)) return;
    const uint64_t job_words = tb_job_words(geo.nstrips, geo.nsteps, NW);

    auto do_pass = [&](const int pass) {
        // pass 0: (A, B) if they agree, else (A, A); pass 1: (B, B) for the couples that did not
        const bool pair_ok = pass == 0 ? okA : two;
        const uint32_t P0 = pass == 0 ? pA : pB, P1 = (pass == 0 && !same) ? pA : pB;
        const uint32_t m = !pair_ok ? 0 : (pass == 0 ? mA : mB), n = !pair_ok ? 0 : (pass == 0 ? nA : nB);
        // symbol offsets of the two pairs' sequences (bytes, or 2-bit codes when a.packed: sym2)
        const uint64_t xs0 = pass == 0 ? xoA : xoB, ys0 = pass == 0 ? yoA : yoB;
        const uint64_t xs1 = (pass == 0 && !same) ? xoA : xoB, ys1 = (pass == 0 && !same) ? yoA : yoB;
        const uint8_t* x0 = a.x + xs0;
        const uint8_t* x1 = a.x + xs1;
        const bool packed = a.packed != 0;  // wave-uniform (kernel argument)
        // one y symbol of both pairs of the couple (only the two offsets stay live across the steps, as the two byte
        // pointers did)
        // (SYMHI: in the high byte of each half, as px[])
        auto y_pair = [&](uint32_t col) -> pk {
            if (packed) return (sym2(a.y, ys0 + col) | (sym2(a.y, ys1 + col) << 16)) << SYM_SH;
            return ((uint32_t)a.y[ys0 + col] | ((uint32_t)a.y[ys1 + col] << 16)) << SYM_SH;
        };
        const uint32_t Q0 = pair_ok ? P0 : 0, Q1 = pair_ok ? P1 : 0;
        uint32_t* tb0 = (uint32_t*)a.tb + (size_t)(Q0 / PW) * job_words + ((Q0 % PW) * LP + ll) * 16u;
        uint32_t* tb1 = (uint32_t*)a.tb + (size_t)(Q1 / PW) * job_words + ((Q1 % PW) * LP + ll) * 16u;
        int32_t* aux0 = a.aux + (size_t)Q0 * geo.aux_stride;
        int32_t* aux1 = a.aux + (size_t)Q1 * geo.aux_stride;
        int32_t* gLx0 = aux0 + geo.off_Lx();
        int32_t* gLx1 = aux1 + geo.off_Lx();

        uint32_t m_w = m, n_w = n;  // wave-uniform loop bounds
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            m_w = max(m_w, (uint32_t)__shfl_xor((int)m_w, o));
            n_w = max(n_w, (uint32_t)__shfl_xor((int)n_w, o));
        }
        (void)m_w;
        n_w = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_w);  // tell the compiler it is wave-uniform
        const uint32_t nsteps_w = n_w ? n_w + LP - 1 : 0;

        int32_t fold0;
        uint32_t lx0;
        if (KO_SETUP) {
            fold0 = NEG;
            lx0 = 0;
        } else {
            col0_fold(sc, m, fold0, lx0);
        }
        // row 0 (mod.rs:678-717), kept by group lane 0.  ROW0_ZERO (yclip_prefix == yclip_suffix == 0): S(0,j) = 0
        // by YCLIP_PREFIX, Sn[0] stays 0 and Ly[0] = n
        int32_t Sn0 = sc.ys;
        uint32_t Ly0 = n;
        int32_t S0n = 0;
        uint32_t sb0n = (ROW0_ZERO && n) ? row0_cell(sc, n).sbits : (uint32_t)TB_START;
        if (pair_ok && ll == 0) {
            const int32_t v = m ? (int32_t)col0_cell(sc, m, m, fold0).sbits : (int32_t)TB_START;
            aux0[0] = v;
            aux1[0] = v;
            if (m == 0) {  // otherwise Lx[0] travels with the row-m lane's first packed store
                if (LP == 16) {
                    *(uint8_t*)gLx0 = (uint8_t)lx0;
                    *(uint8_t*)gLx1 = (uint8_t)lx0;
                } else {
                    *(uint16_t*)gLx0 = (uint16_t)lx0;
                    *(uint16_t*)gLx1 = (uint16_t)lx0;
                }
            }
        }

        const uint32_t rb = (uint32_t)ll * R;  // this lane owns rows rb+1 .. rb+R (single strip)
        const int32_t mrow = (int32_t)m - (int32_t)rb - 1;
        pk Sl[R], Dl[R], Il[R], SnR[R], SnB[R], Ly[R], px[R];
        uint64_t nib0S = 0, nib0I = 0;
        // packed x: this lane's R symbols (rows rb + 1 .. rb + R) of each pair come out of two dwords of the stream —
        // two loads per pair instead of R byte loads (the stream is padded by one dword: the second may lie past the end)
        uint64_t xw0 = 0, xw1 = 0;
        if (packed && pair_ok && rb < m) {
            const uint32_t* p0 = (const uint32_t*)a.x + ((xs0 + rb) >> 4);
            const uint32_t* p1 = (const uint32_t*)a.x + ((xs1 + rb) >> 4);
            xw0 = (((uint64_t)p0[1] << 32) | p0[0]) >> (2 * ((uint32_t)(xs0 + rb) & 15u));
            xw1 = (((uint64_t)p1[1] << 32) | p1[0]) >> (2 * ((uint32_t)(xs1 + rb) & 15u));
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t i = rb + r + 1;
            px[r] = 0;
            Sl[r] = Dl[r] = Il[r] = SnR[r] = SnB[r] = FLOORK;
            Ly[r] = 0;
            if (pair_ok && i <= m) {
                px[r] = packed ? (((uint32_t)(xw0 >> (2 * r)) & 3u) | (((uint32_t)(xw1 >> (2 * r)) & 3u) << 16))
                               : ((uint32_t)x0[i - 1] | ((uint32_t)x1[i - 1] << 16));
                px[r] <<= SYM_SH;
                const Col0 c = KO_SETUP ? Col0{0, kFloor16, (uint32_t)TB_XCLIP_PREFIX, (uint32_t)TB_START} : col0_cell(sc, i, m, fold0);
                Sl[r] = dup16(scl(c.S));
                Il[r] = dup16(scl(c.I) | K_INS);
                nib0S |= (uint64_t)c.sbits << (4 * r);
                nib0I |= (uint64_t)c.ibits << (4 * r);
                if (YS != CI && c.S + sc.ys > NEG) {  // mod.rs:667-670
                    SnR[r] = dup16(scl(c.S + sc.ys));
                    Ly[r] = dup16((int32_t)n);
                }
            }
        }
        pk diag0 = dup16((pair_ok && rb < m) ? (KO_SETUP ? 0 : scl(col0_S(sc, rb, m, fold0))) : NEGS);  // S(rb, 0)
        if (FR) {
            // into the frame: column 0 is step ll - 1 of this lane, its diagonal step ll - 2 of row -1.  Exact modular adds, undone
            // when the rows are parked (a lane that computes nothing gets back what it started with); rows past m start at
            // score 0 and stay garbage nobody reads, as without the frame
            const int32_t off0 = BF + gF * ((int32_t)ll - 1);
#pragma unroll
            for (int r = 0; r < R; r++) {
                const pk o = fr(off0 + gF * r);
                Sl[r] = (pair_ok && rb + r + 1 <= m) ? Sl[r] + o : o;
                Il[r] += o;
                Dl[r] = 0;
            }
            diag0 = fr(off0 - gF) + ((pair_ok && rb < m) ? dup16((KO_SETUP ? 0 : scl(col0_S(sc, rb, m, fold0)))) : 0u);
        }

        pk S_out = FLOORK, I_out = FLOORK, cm_out = FLOORK, ca_out = 0, q_out = 0;
        pk ychunk = 0, ychunk_nx = 0;
        pk hwlast[NH];  // traceback halves of this lane's last column
#pragma unroll
        for (int k = 0; k < NH; k++) hwlast[k] = 0;
        pk lx_n = dup16((int32_t)lx0);
        // VMEM store instructions are the scarce resource of this kernel (four per step cost 5 ms of 17 on
        // 1M x 150 bp), and 64-byte slots filled 8 or 16 bytes at a time get evicted half-written (1.5x HBM
        // write traffic): a lane's traceback words collect in LDS and leave as its complete 64-byte slot of the
        // tile, four back-to-back 16-byte stores per pair every 16 / NW steps; Lx[j] (<= m < 256) leaves as bytes,
        // four columns per dword store
        pk* tileA = wave_lds + (0 * 64 + lane) * kTileStride;
        pk* tileB = wave_lds + (1 * 64 + lane) * kTileStride;
        // Lx[0] ends up in the first element of the first dword (bytes up to 16 x 12 rows, else 16 bits)
        uint32_t lxaccA = lx0 << (LP == 16 ? 24 : 16), lxaccB = lxaccA;
        if (pair_ok && (uint32_t)ll < n) ychunk_nx = y_pair((uint32_t)ll);

        // Sn[i]/Ly[i] (mod.rs:799-802, "first maximum of the row") per block of 16 steps: inside a block the
        // key best | (15 - step % 16) lets one packed max keep the earliest column; the block's winner is
        // folded into the running maximum (strictly greater only) when the block ends.
        auto merge_rows = [&](uint32_t blockbase) {
            const pk lybase = dup16((int32_t)(n - blockbase - 16u + (uint32_t)ll));
#pragma unroll
            for (int r = 0; r < R; r++) {
                const pk nr = pk_max(SnR[r], SnB[r] & CLEAN);
                const pk msk = nz_mask(nr ^ SnR[r], ONE);
                Ly[r] = bfi(msk, pk_add_u16(lybase, SnB[r] & 0x000f000fu), Ly[r]);
                SnR[r] = nr;
                SnB[r] = FLOORK;
            }
        };

        constexpr uint32_t tsteps = tb_tile_steps(NW);
        auto store_tile = [&](uint32_t s_any) {  // the tile that holds step s_any, see tb_word_off()
            if (!pair_ok) return;
            const uint32_t off = (s_any / tsteps) * 1024u;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                *(uint4*)&tb0[off + 4 * k] = *(const uint4*)&tileA[4 * k];
                *(uint4*)&tb1[off + 4 * k] = *(const uint4*)&tileB[4 * k];
            }
        };
        // MRk >= 0: every pair of this wavefront has its row m at r == MRk of its owner lane (equal read
        // lengths, the usual short-read case): the x-suffix-clip candidate drops out of the other rows
        // ALLON: every lane of the wavefront is inside its matrix at this step (LP - 1 <= s < min over the lanes of
        // n + ll): the body runs without the column predicate — the compiler kept the 4 R loop-carried row values in
        // a second set of registers around the predicated region and copied them back every step (≈ 40 v_mov of 350
        // instructions).  The ramp-up and ramp-down steps keep the predicate.
        uint32_t s_all = pair_ok ? n + (uint32_t)ll : 0u;
#pragma unroll
        for (int o = 32; o; o >>= 1) s_all = min(s_all, (uint32_t)__shfl_xor((int)s_all, o));
        s_all = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_all);
        auto run_steps = [&](auto mr_tag) {
        constexpr int MRk = decltype(mr_tag)::value;
        auto step = [&](auto allon_tag, auto fast_tag, auto trip_tag, const uint32_t s) {
            constexpr bool ALLON = decltype(allon_tag)::value;
            // ROWMAX2: 1 / 2 = the first / second step of a two-step trip (s even / odd, both ALLON), 0 = a step on its own
            constexpr int TRIP = decltype(trip_tag)::value;
            static_assert(!TRIP || (ALLON && ROWMAX2), "trips are pairs of unpredicated steps of the FR == 2 cell");
            constexpr bool FB = decltype(fast_tag)::value;  // LF: no fold (see above)
            constexpr bool FOLD = XS != CI && !FB;
            if ((s & (LP - 1)) == 0) {  // wave-uniform: next LP columns of y
                ychunk = ychunk_nx;
                const uint32_t nb = s + LP + ll;
                if (pair_ok && nb < n) ychunk_nx = y_pair(nb);
            }
            // lane 0 of the wavefront keeps its own value ("old" == source): it is a row-0 lane and overrides it
            pk S_up = (pk)wave_shr1((int)S_out, (int)S_out), I_up = (pk)wave_shr1((int)I_out, (int)I_out);
            if (FR) {  // into this lane's frame (re-based here rather than before the shift: S_out / I_out stay the last row's registers)
                S_up -= KREB;
                I_up -= KREB;
            }
            pk cm = FLOORK, ca = 0;
            if (FOLD) {
                cm = (pk)wave_shr1((int)cm_out, (int)cm_out);
                ca = (pk)wave_shr1((int)ca_out, (int)ca_out);
            }
            pk q = (pk)wave_shr1((int)q_out, (int)q_out);
            const uint32_t j = s + 1 - (uint32_t)ll;
            const bool col_ok = ALLON || (pair_ok && (j - 1) < n);  // 1 <= j <= n
            const pk F0 = fr(BF + gF * (int32_t)s);  // FR: the frame of row 0 at this step (wave-uniform)
            (void)F0;
            if (ll == 0) {  // row 0 of the matrix (mod.rs:678-721)
                q = ychunk;
                S_up = FR ? F0 - GF : 0u;  // row -1
                I_up = FR ? 0u : FLOORK;   // mod.rs:681
                cm = FLOORK;    // S[curr][1..=m] reset, mod.rs:719-721 (both dead without FOLD)
                ca = 0;         // Lx[j] starts at 0
                if (!ROW0_ZERO && col_ok) {
                    const Row0 c = row0_cell(sc, j);
                    int32_t S0 = c.S;
                    uint32_t sb = c.sbits;
                    if (j == n && Sn0 > S0) {  // mod.rs:706-714
                        S0 = Sn0;
                        sb = TB_YCLIP_SUFFIX;
                    } else if (S0 + sc.ys > Sn0) {
                        Sn0 = S0 + sc.ys;
                        Ly0 = n - j;
                    }
                    S0n = S0;  // the last write is column n
                    sb0n = sb;
                    S_up = dup16(scl(S0));
                }
            }
            ychunk = (pk)wave_shl1((int)ychunk, (int)ychunk);

            if (col_ok) {
                const pk sprio = dup16((int32_t)(15u - (s & 15u)));
                pk diag = diag0;
                diag0 = S_up;
                pk hw[NH];
                const pk ca_in = ca;
                pk cmk = cm | 0x000f000fu;  // fold key: clean running maximum | row priority (15 = an earlier lane)
                pk snap = cmk;               // the fold as row m sees it
                // mod.rs:724-728: the x-prefix-clip candidate of this column (0 for local; absent when xclip_prefix
                // is MIN_SCORE).  The y-prefix-clip candidate yp + go + ge (i - 1) of mod.rs:780-782 is never
                // strictly above I(i,j) >= S(0,j) + go + ge (i - 1) >= the same, and INS comes first: it is not computed.
                pk XKEY = dup16(K_XP);
                if (XP == CF || (XP == CZ && YP != CZ))
                    XKEY = dup16(scl(sc.xp + max(sc.yp, sc.go + sc.ge * ((int32_t)j - 1))) | K_XP);
#pragma unroll
                    for (int r = 0; r < R; r++) {  // rows past m compute garbage nobody reads
                        const bool maybe_m = MRk < 0 || r == MRk;
                        const bool is_m = MRk < 0 ? (r == mrow) : (r == MRk && mrow == MRk);
                        // mod.rs:733-755: substitution score with the MATCH/SUBST move code in its low bits
                        // (SYMHI: DELTA where they agree — px[r] ^ q is 0 or >= 256 >= DELTA in each half)
                        const pk e = pk_subs_u16(SYMHI ? DELTA : ONE, px[r] ^ q);  // 1 where the characters agree
                        // LF: diag >= 0, the sum saturates at key 0 = (score 0, code 0) where the reference's S falls back on
                        // the x-prefix clip; FR: the floor is that key in the frame, F(r, s)
                        const pk Fr = F0 + (uint32_t)r * GF;
                        (void)Fr;
                        // (FR == 2: the floor enters D's maximum of three instead, or kb's first)
                        // (SYMHI: two full-rate adds, kept apart: the compiler would make them one half-rate v_add3_u32)
                        pk dk = diag + KSUB;
                        if (SYMHI && !(PK16_CELL_KO & 8)) asm("" : "+v"(dk));
                        const pk m_key = SYMHI   ? e + dk
                                         : FR == 2 ? pk_mad_u16(e, DELTA, diag) + KSUB
                                         : FR    ? pk_max(pk_mad_u16(e, DELTA, diag) + KSUB, Fr)
                                         : LF    ? pk_subs_u16(pk_mad_u16(e, DELTA, diag), MISC)
                                                 : pk_adds(diag, pk_mad_u16(e, DELTA, MISK));
                        const pk Iv_t = FR ? pk_max(I_up, S_up + KGOI) : pk_max(pk_adds(I_up, GE), pk_adds(S_up, GOT_I));
                        // DFLOOR: D carries the floor, max(D, F(r, s)) — off the row-to-row chain — and kb takes one maximum of
                        // three; why no record or operation changes: see FR == 2 above
                        const pk Dv_t = DFLOOR ? pk_max3h(Dl[r], Sl[r] + KGOD, Fr)
                                        : FR   ? pk_max(Dl[r], Sl[r] + KGOD)
                                               : pk_max(pk_adds(Dl[r], GE), pk_adds(Sl[r], GOT_D));
                        const pk Iv = Iv_t & NOFLAG, Dv = Dv_t & NOFLAG;
                        // mod.rs:757-786: first maximum wins == max over (score | priority)
                        pk kb = DFLOOR ? m_key : FR == 2 ? pk_max3h(m_key, Fr, Dv_t) : pk_max(m_key, Dv_t);
                        if (XP != CI && !LF) kb = pk_max(kb, XKEY);
                        // the value that waits for the row above comes last
                        kb = DFLOOR ? pk_max3h(kb, Dv_t, Iv_t) : FR == 2 ? pk_max3h(kb, Iv_t, Iv_t) : pk_max(kb, Iv_t);
                        if (FOLD && maybe_m)
                            kb = pk_max(kb, is_m ? ((cmk & CLEAN) | (0x00010001u * K_XS)) : FLOORK);
                        const pk best = kb & CLEAN;
                        const pk best_prev = Sl[r];  // this row's best of the step before
                        diag = Sl[r];
                        Sl[r] = best;
                        Dl[r] = Dv;
                        Il[r] = Iv;
                        S_up = best;
                        I_up = Iv;
                        if (FOLD) {  // mod.rs:793-796
                            if (maybe_m) snap = is_m ? cmk : snap;
                            const pk fv = XS == CZ ? best : pk_min(pk_adds(best, XS16), XSCAP);
                            cmk = pk_max(cmk, fv | (0x00010001u * (uint32_t)(14 - r)));
                        }
                        if (YS != CI) {  // mod.rs:799-802
                            const pk t1 = YS == CZ ? best : pk_min(pk_adds(best, YS16), YSCAP);
                            // ROWMAX2: nothing in the first step of a trip; the second takes both steps' keys with one maximum
                            // of three (both lie in one 16-step priority block: s - 1 is even, its priority sprio + 1 >= 1, so
                            // that key is never 0 and the result does not depend on how maximum orders SnB's initial 0x8000,
                            // -0.0, against key 0, +0.0)
                            if (TRIP == 2)
                                SnB[r] = pk_max3h(SnB[r], best_prev - (Fr - GF - sprio - ONE), best - (Fr - sprio));
                            else if (TRIP == 0)
                                SnB[r] = pk_max(SnB[r], FR ? best - (Fr - sprio) : t1 | sprio);  // FR: out of the frame
                        }
                        // packed cell: I opens | 3-bit move << 1 | D opens << 4 (flipped to "extends" below)
                        const pk c5 = pk_mad_u16(Dv_t & ONE, C16, (kb & 0x000e000eu) | (Iv_t & ONE));
                        if (r % 3 == 0)
                            hw[r / 3] = c5;
                        else
                            hw[r / 3] = pk_mad_u16(c5, r % 3 == 1 ? C32 : C1024, hw[r / 3]);
                    }
                if (FOLD) {
                    // Lx[j] = rows between the fold's winner and row m (mod.rs:793-796): priority 15 = a lane above
                    const pk mbase = dup16(mrow - 14);
                    const pk lo = cmk & 0x000f000fu, slo = snap & 0x000f000fu;
                    if (mrow >= 0 && mrow < R) {  // the lane that owns row m publishes Lx[j]
                        const pk is15 = nz_mask(slo ^ 0x000f000fu, ONE);  // 0xffff where slo != 15
                        lx_n = bfi(is15, pk_add_u16(slo, mbase), ca_in);
                        if (LP == 16) {  // Lx <= m <= 192: bytes, four columns per dword
                            lxaccA = __builtin_amdgcn_perm(lx_n, lxaccA, 0x04030201u);  // acc >> 8 | Lx_A << 24
                            lxaccB = __builtin_amdgcn_perm(lx_n, lxaccB, 0x06030201u);  // acc >> 8 | Lx_B << 24
                            if ((j & 3u) == 3u || j == n) {
                                const uint32_t sh = 8u * (3u - (j & 3u));  // the last dword of the row may be partial
                                ((uint32_t*)gLx0)[j >> 2] = lxaccA >> sh;
                                ((uint32_t*)gLx1)[j >> 2] = lxaccB >> sh;
                            }
                        } else {  // 16 bits, two columns per dword
                            lxaccA = __builtin_amdgcn_perm(lx_n, lxaccA, 0x05040302u);  // acc >> 16 | Lx_A << 16
                            lxaccB = __builtin_amdgcn_perm(lx_n, lxaccB, 0x07060302u);  // acc >> 16 | Lx_B << 16
                            if ((j & 1u) == 1u || j == n) {
                                const uint32_t sh = 16u * (1u - (j & 1u));
                                ((uint32_t*)gLx0)[j >> 1] = lxaccA >> sh;
                                ((uint32_t*)gLx1)[j >> 1] = lxaccB >> sh;
                            }
                        }
                    }
                    {
                        const pk is15 = nz_mask(lo ^ 0x000f000fu, ONE);
                        ca = bfi(is15, pk_add_u16(lo, mbase), ca_in);
                    }
                    cm = cmk & CLEAN;
                }
                // 17 = both "opens" bits: stored as "extends" like K1's cells
                constexpr pk INV = 0x00010001u * (17u | (17u << 5) | (17u << 10));
                constexpr pk INV_LAST = 0x00010001u * ((R % 3 == 0) ? (17u | (17u << 5) | (17u << 10))
                                                      : (R % 3 == 1) ? 17u : (17u | (17u << 5)));
#pragma unroll
                for (int k = 0; k < NH; k++) {
                    hw[k] ^= (k == NH - 1) ? INV_LAST : INV;
                    hwlast[k] = hw[k];
                }
                const pk h0 = hw[0], h1 = NH > 1 ? hw[NH > 1 ? 1 : 0] : 0u;
                const uint32_t slot = (s % tsteps) * NW;
                if (NW == 1) {
                    tileA[slot] = __builtin_amdgcn_perm(h1, h0, 0x05040100u);
                    tileB[slot] = __builtin_amdgcn_perm(h1, h0, 0x07060302u);
                } else {
                    const pk h2 = hw[NH > 2 ? 2 : 0], h3 = NH > 3 ? hw[NH > 3 ? 3 : 0] : 0u;
                    *(uint2*)&tileA[slot] = make_uint2(__builtin_amdgcn_perm(h1, h0, 0x05040100u),
                                                       __builtin_amdgcn_perm(h3, h2, 0x05040100u));
                    *(uint2*)&tileB[slot] = make_uint2(__builtin_amdgcn_perm(h1, h0, 0x07060302u),
                                                       __builtin_amdgcn_perm(h3, h2, 0x07060302u));
                }
                S_out = S_up;
                I_out = I_up;
                if (FOLD) {
                    cm_out = cm;
                    ca_out = ca;
                }
                q_out = q;
            }
            if (s % tsteps == tsteps - 1) store_tile(s);  // wave-uniform
            if (YS != CI && (s & 15u) == 15u) merge_rows(s & ~15u);  // wave-uniform
        };
        uint32_t s = 0;
        const uint32_t s_on = min((uint32_t)(LP - 1), nsteps_w), s_off = max(s_on, min(s_all, nsteps_w));
        constexpr std::false_type no{};
        constexpr std::true_type yes{};
        constexpr std::bool_constant<LF> fast{};
        constexpr std::integral_constant<int, 0> single{};
        constexpr std::integral_constant<int, ROWMAX2 ? 1 : 0> first{};
        constexpr std::integral_constant<int, ROWMAX2 ? 2 : 0> second{};
        for (; s < s_on; s++) step(no, fast, single, s);
        // ROWMAX2: trips start on an even step (s_on = LP - 1 is odd: one step on its own first), so that both steps of a
        // trip share a priority block and merge_rows (s % 16 == 15) comes after a trip's second step
        if (ROWMAX2 && (s & 1u) && s < s_off) step(yes, fast, single, s++);
        for (; s + 1 < s_off; s += 2) {  // two steps per trip: the row values alternate between two sets of registers
            step(yes, fast, first, s);
            step(yes, fast, second, s + 1);
        }
        for (; s < s_off; s++) step(yes, fast, single, s);
        for (; s < nsteps_w; s++) step(no, fast, single, s);
        };
        run_steps(std::integral_constant<int, (FAST && !LF) ? R - 1 : -1>{});
        if (nsteps_w % tsteps) store_tile(nsteps_w - 1);  // the last, partial tile
        if (YS != CI && nsteps_w) merge_rows((nsteps_w - 1) & ~15u);
        if (KO_EPILOGUE) {  // what the epilogue reads stays computed
#pragma unroll
            for (int r = 0; r < R; r++) asm volatile("" ::"v"(Sl[r]), "v"(Il[r]), "v"(SnR[r]), "v"(Ly[r]));
#pragma unroll
            for (int k = 0; k < NH; k++) asm volatile("" ::"v"(hwlast[k]));
            asm volatile("" ::"v"(lx_n));
            return;
        }

        if constexpr (LF) {
            // =========== last column of a local alignment (mod.rs:808-821), both pairs of the couple at once ===========
            // Only what K2 reads of column n is computed and published (DESIGN.md §4.1): the score, Lx[n] and the S nibble
            // of (m, n), the row i* the x-suffix clip of (m, n) jumps to (aux[3]; m if it does not) with its S nibble and
            // Ly, and row 0.  The second pass (mod.rs:825-843) offers max S1(i' < i) + go + ge k with go < 0: strictly below a
            // value the first pass already offered, so it changes neither (m, n) nor the cell the clip lands on.
            // Everything stays in the packed 16-bit halves: scores are multiples of 16, the low nibble of a key holds the
            // priority ("equal keeps the earlier row" == a larger nibble), and one signed packed maximum compares both pairs.
            const bool nz = n != 0;
            const int32_t S0fin = nz ? scl(S0n) : 0;
            const uint32_t sb0fin = nz ? sb0n : (uint32_t)TB_START;
            const bool has_row0 = pair_ok && ll == 0;
            pk* park = wave_lds + lane;  // thread-private slots, stride 64: the rows are indexed at run time below
            // FR: out of the frame of the lane's last column, step n - 1 + ll (n == 0: the frame of column 0 it started in)
            const pk offl = FR ? fr(BF + gF * ((int32_t)ll + (int32_t)n - 1)) : 0u;
            // per lane: first maximum over its rows below m (r < mrow) of S(i, n) (the fold the fill did not keep) and of
            // S1(i) = max(S(i, n), Sn[i]); row r carries priority 14 - r, row 0 of the matrix 15
            pk KF = FLOORK, KC = FLOORK;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const pk sl = FR ? Sl[r] - (offl + (uint32_t)r * GF) : Sl[r];
                park[(0 * R + r) * 64] = sl;
                park[(1 * R + r) * 64] = SnR[r];
                park[(2 * R + r) * 64] = Ly[r];
                if (r < mrow) {
                    const pk pr = dup16(14 - r);
                    KF = pk_max(KF, sl | pr);
                    KC = pk_max(KC, pk_max(sl, SnR[r]) | pr);
                }
            }
#pragma unroll
            for (int k = 0; k < NH; k++) park[(3 * R + k) * 64] = hwlast[k];
            if (has_row0 && m != 0) KC = pk_max(KC, dup16(S0fin) | 0x000f000fu);
            // across the lanes of the pair: score | 15 - lane, one packed maximum over each row of 16 lanes (LP == 32: the two
            // rows are combined, the lower one keeps ties, see group_first_max)
            const pk lprio = dup16(15 - (ll & 15));
            pk HF, HC;
            const pk RF = group_first_max<LP>((KF & CLEAN) | lprio, ll, HF), RC = group_first_max<LP>((KC & CLEAN) | lprio, ll, HC);
            // row m: its owner's S(m, n) and Sn[m] go to every lane of the pair, which all resolve (m, n) the same way
            const bool own_m = pair_ok && m != 0 && mrow >= 0 && mrow < R;
            const bool own_m0 = pair_ok && m == 0 && ll == 0;
            const int mr = own_m ? mrow : 0;
            pk Sm = park[(0 * R + mr) * 64], Snm = park[(1 * R + mr) * 64];
            if (!own_m) {  // m == 0: (0, n) is row 0 itself, Sn[0] > S(0, n) never holds (mod.rs:706-714)
                Sm = dup16(S0fin);
                Snm = FLOORK;
            }
            const int ol = m ? (int)((m - 1) / (uint32_t)R) : 0;
            Sm = (pk)__shfl((int)Sm, ol, LP);
            Snm = (pk)__shfl((int)Snm, ol, LP);
            // in the reference's order: the cell's own candidates against the fold (the fold was there first: it keeps ties),
            // then rows 0 .. m - 1 of the first loop (strictly greater only), then Sn[m]
            const pk Fs = RF & CLEAN, Cs = RC & CLEAN;
            const pk v1 = nz ? pk_max(Sm, Fs) : Sm;
            const pk foldwin = nz ? ~nz_mask(v1 ^ Fs, ONE) : 0u;
            const pk v2 = pk_max(v1, Cs);
            const pk c1win = nz_mask(v2 ^ v1, ONE);
            const pk v3 = pk_max(v2, Snm);
            const pk ywin = nz_mask(v3 ^ v2, ONE);
            const pk xswon = foldwin | c1win;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (!pair_ok || (h == 1 && P1 == P0)) continue;  // (A, A) / (B, B): one record
                const uint32_t hs = 16u * (uint32_t)h;
                int32_t* aux = h ? aux1 : aux0;
                int32_t* gLy = aux + geo.off_Ly();
                uint8_t* gBits = (uint8_t*)(aux + geo.off_bits());
                const bool xs = (xswon >> hs) & 1u, c1 = (c1win >> hs) & 1u, yw = (ywin >> hs) & 1u;
                // the S nibble of (rb + r + 1, n) as the fill left it
                auto fillnib = [&](int r) -> uint32_t {
                    if (!nz) return (uint32_t)(nib0S >> (4 * r)) & 15u;
                    const uint32_t mv = (park[(3 * R + r / 3) * 64] >> (hs + 5u * (uint32_t)(r % 3) + 1u)) & 7u;
                    return s_nibble_of_code(mv == 0 ? (uint32_t)C_XP : mv);
                };
                // the lane that holds i*: its own key knows the row
                const uint32_t wl = 15u - (((c1 ? RC : RF) >> hs) & 15u) + (((c1 ? HC : HF) >> hs) & 16u);
                if (xs && (uint32_t)ll == wl) {
                    const uint32_t code = ((c1 ? KC : KF) >> hs) & 15u;
                    uint32_t istar = 0;  // code 15: row 0, whose entries lane 0 writes below
                    if (code != 15u) {
                        const int r = min(max(14 - (int)code, 0), R - 1);
                        istar = rb + (uint32_t)r + 1;
                        const int32_t sl = (int32_t)(int16_t)(park[(0 * R + r) * 64] >> hs);
                        const int32_t sn = (int32_t)(int16_t)(park[(1 * R + r) * 64] >> hs);
                        gBits[istar] = (uint8_t)(sn > sl ? (uint32_t)TB_YCLIP_SUFFIX : fillnib(r));  // mod.rs:812-815
                        gLy[istar] = (int32_t)((park[(2 * R + r) * 64] >> hs) & 0xffffu);
                    }
                    aux[2] = (int32_t)(m - istar);
                    aux[3] = (int32_t)istar;
                }
                if (own_m || own_m0) {
                    aux[1] = (int32_t)(int16_t)(v3 >> hs) >> SH;  // exact: every scaled value is a multiple of 16
                    const uint32_t sbm = yw ? (uint32_t)TB_YCLIP_SUFFIX : xs ? (uint32_t)TB_XCLIP_SUFFIX : own_m ? fillnib(mr) : sb0fin;
                    gBits[m] = (uint8_t)sbm;
                    if (own_m) gLy[m] = (int32_t)((park[(2 * R + mr) * 64] >> hs) & 0xffffu);
                    if (!xs) {
                        uint32_t istar = m;
                        if (sbm == (uint32_t)TB_XCLIP_SUFFIX) {  // n == 0, m >= 2: column 0's own fold (mod.rs:658-661) jumps to row m - lx0
                            istar = m - lx0;
                            gBits[istar] = (uint8_t)col0_cell(sc, istar, m, fold0).sbits;
                            gLy[istar] = (int32_t)n;  // mod.rs:667-670
                        }
                        aux[2] = (int32_t)lx0;
                        aux[3] = (int32_t)istar;
                    }
                }
                if (has_row0) {
                    gLy[0] = (int32_t)Ly0;
                    if (m != 0) gBits[0] = (uint8_t)(sb0fin | (TB_START << 4));
                }
            }
        } else {
            // =========== epilogue of the last column (mod.rs:808-843), one pair of the couple at a time ===========
            // The packed rows are parked in LDS (thread-private slots, stride 64: conflict-free) so that the
            // epilogue's 64-bit scans do not have to share the register file with them.
            pk* park = wave_lds + lane;
            // FR: out of the frame of the lane's last column, step n - 1 + ll (n == 0: the frame of column 0 it started in)
            const pk offl = FR ? fr(BF + gF * ((int32_t)ll + (int32_t)n - 1)) : 0u;
#pragma unroll
            for (int r = 0; r < R; r++) {
                park[(0 * R + r) * 64] = FR ? Sl[r] - (offl + (uint32_t)r * GF) : Sl[r];
                park[(1 * R + r) * 64] = FR ? Il[r] - (offl + (uint32_t)r * GF) : Il[r];
                park[(2 * R + r) * 64] = SnR[r];
                park[(3 * R + r) * 64] = Ly[r];
            }
#pragma unroll
            for (int k = 0; k < NH; k++) park[(4 * R + k) * 64] = hwlast[k];
            park[(4 * R + NH) * 64] = lx_n;
            const int nhalf = (pair_ok && P1 != P0) ? 2 : 1;
            const int nhalf_w = __any(nhalf == 2) ? 2 : 1;
#pragma unroll 1
            for (int h = 0; h < nhalf_w; h++) {
                if (h >= nhalf) continue;  // the shuffles below only pair lanes of one group, whose nhalf agree
                const uint32_t hs = 16u * (uint32_t)h;
                int32_t* aux = h ? aux1 : aux0;
                int32_t* gLy = aux + geo.off_Ly();
                uint8_t* gBits = (uint8_t*)(aux + geo.off_bits());
                const uint32_t strip = 0;
                // unpacked (sign-extended, still scaled by 16) views of this pair's half
                struct HalfS {
                    const pk* p;
                    uint32_t hs;
                    __device__ int32_t operator[](int r) const { return (int32_t)(int16_t)(p[r * 64] >> hs); }
                };
                struct HalfU {
                    const pk* p;
                    uint32_t hs;
                    __device__ uint32_t operator[](int r) const { return (p[r * 64] >> hs) & 0xffffu; }
                };
                int32_t Sl_u[R];  // the epilogue overwrites S(i, n)
#pragma unroll
                for (int r = 0; r < R; r++) Sl_u[r] = (int32_t)(int16_t)(park[r * 64] >> hs);
                const HalfS Il_u{park + 1 * R * 64, hs}, Sn_u{park + 2 * R * 64, hs};
                const HalfU Ly_u{park + 3 * R * 64, hs};
                const uint32_t lx_n_u = (park[(4 * R + NH) * 64] >> hs) & 0xffffu;
                int64_t e_carry = INT64_MIN;
                uint32_t sbf_carry = TB_START, sb2_carry = TB_START;
                int64_t c1v = INT64_MIN, c2v = INT64_MIN;
                uint32_t c1i = 0, c2i = 0;
                auto cell_of = [&](int r) -> uint32_t {  // K1's bit order: move | I extends << 3 | D extends << 4
                    const uint32_t c = (park[(4 * R + r / 3) * 64] >> (hs + 5 * (r % 3))) & 31u;
                    const uint32_t mv = (c >> 1) & 7u;
                    return ((LF && mv == 0) ? (uint32_t)C_XP : mv) | ((c & 1u) << 3) | (c & 16u);
                };
                {
                    constexpr bool EPI_FOLD_PRE = false;  // (K1's LF flavour; K1p's has the epilogue above)
                    // the names the shared body expects
                    int32_t(&Sl)[R] = Sl_u;
                    const HalfS& Il = Il_u;
                    const HalfS& Sn = Sn_u;
                    const HalfU& Ly = Ly_u;
                    const uint32_t lx_n = lx_n_u;
#include "sw_epilogue.inc"
                }
            }
        }
    };
    do_pass(MODE == 2 ? 1 : 0);
}

// the fast launch is tuned for three wavefronts per SIMD up to R = 10 (168 VGPRs, 46 KB of LDS per block); the two
// others take what the generic row-m handling needs, two per SIMD at least
template <int R, int LP, int XP, int XS, int YP, int YS, bool LF, int FR = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(R <= 10 ? 3 : 2, R <= 10 ? 3 : 2))) void sw_fill_pk16_kernel(const SwArgs a) {
    sw_fill_pk16_body<R, LP, 0, XP, XS, YP, YS, LF, FR>(a);
}
template <int R, int LP, int XP, int XS, int YP, int YS, bool LF, int FR = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(R <= 10 ? 3 : 2, R <= 10 ? 3 : 2))) void sw_fill_pk16_rest_kernel(const SwArgs a) {
    sw_fill_pk16_body<R, LP, 1, XP, XS, YP, YS, LF, FR>(a);
}
template <int R, int LP, int XP, int XS, int YP, int YS, bool LF, int FR = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(R <= 10 ? 3 : 2, R <= 10 ? 3 : 2))) void sw_fill_pk16_second_kernel(const SwArgs a) {
    sw_fill_pk16_body<R, LP, 2, XP, XS, YP, YS, LF, FR>(a);
}

}  // namespace pk16
}  // namespace bgsw

// shape (LP_, R_) of a unit's getter (sw_fill_get_K1P_*, one unit per clip pattern), expanded over a shape list of
// sw_kernels.h with the unit's clips XP_ .. YS_ and flavour LF_, FR_ in scope
#define BG_PK16_CASE(LP_, R_)                                                                          \
    if (lp == LP_ && r == R_)                                                                         \
        return which == 0   ? pk16::sw_fill_pk16_kernel<R_, LP_, XP_, XS_, YP_, YS_, LF_, FR_>        \
               : which == 1 ? pk16::sw_fill_pk16_rest_kernel<R_, LP_, XP_, XS_, YP_, YS_, LF_, FR_>   \
                            : pk16::sw_fill_pk16_second_kernel<R_, LP_, XP_, XS_, YP_, YS_, LF_, FR_>;
