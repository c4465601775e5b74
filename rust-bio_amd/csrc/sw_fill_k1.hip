// K1 instantiations (sw_fill.inc): MatchParams scoring (Scoring::from_scores, mod.rs:259-278) and its LF flavour, and
// tabulated match functions (closures / BLOSUM / PAM, scores/mod.rs) — SCORE_LDS keeps the compacted A x A table in LDS,
// SCORE_GLOBAL (A > 64) reads it from HBM/L2.  LOCAL: the cell of Aligner::local (all four clip penalties 0,
// mod.rs:995-999), for a tabulated match function with the table in LDS only (what a BLOSUM62 / PAM local alignment of
// protein reads runs).
#include "sw_fill.inc"
namespace bgsw {
template <int SM, bool LOCAL, bool NARROW, bool LF = false>
static sw_fill_fn k1(int lp, int r) {
#define BG_X(LP, R) if (lp == LP && r == R) return sw_fill_kernel<R, LP, SM, LOCAL, NARROW, LF>;
    if constexpr (SM == SCORE_PARAMS) {
        BG_K1_SHAPES(BG_X)
    } else if constexpr (SM == SCORE_LDS && NARROW) {
        BG_K1_TABLE_LDS_NARROW_SHAPES(BG_X)
    } else {
        BG_K1_TABLE_SHAPES(BG_X)
    }
#undef BG_X
    return nullptr;
}
template <int SM, bool LOCAL>
static sw_fill_fn k1(bool narrow, int lp, int r) {
    return narrow ? k1<SM, LOCAL, true>(lp, r) : k1<SM, LOCAL, false>(lp, r);
}
sw_fill_fn sw_fill_get_K1(bool narrow, int lp, int r, int) { return k1<SCORE_PARAMS, false>(narrow, lp, r); }
sw_fill_fn sw_fill_get_K1_LOCAL(bool narrow, int lp, int r, int) { return k1<SCORE_PARAMS, true>(narrow, lp, r); }
sw_fill_fn sw_fill_get_K1_LF(bool narrow, int lp, int r, int) { return narrow ? k1<SCORE_PARAMS, true, true, true>(lp, r) : nullptr; }
sw_fill_fn sw_fill_get_K1_LDS(bool narrow, int lp, int r, int) { return k1<SCORE_LDS, false>(narrow, lp, r); }
sw_fill_fn sw_fill_get_K1_LDS_LOCAL(bool narrow, int lp, int r, int) { return narrow ? k1<SCORE_LDS, true, true>(lp, r) : nullptr; }
sw_fill_fn sw_fill_get_K1_GLOBAL(bool narrow, int lp, int r, int) { return k1<SCORE_GLOBAL, false>(narrow, lp, r); }
}  // namespace bgsw
