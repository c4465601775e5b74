// K1p instantiations for Aligner::global (mod.rs:934-938): all four clip penalties MIN_SCORE.
#include "sw_fill_pk16.inc"
namespace bgsw {
sw_fill_fn sw_fill_get_K1P_GLOBAL(bool, int lp, int r, int which) {
    constexpr int XP_ = pk16::CI, XS_ = pk16::CI, YP_ = pk16::CI, YS_ = pk16::CI;
    constexpr bool LF_ = false, FR_ = false;
    BG_K1P_SHAPES(BG_PK16_CASE)
    return nullptr;
}
}  // namespace bgsw
