// K1p instantiations for Aligner::semiglobal (mod.rs:963-967): x clips MIN_SCORE, y clips 0.
#include "sw_fill_pk16.inc"
namespace bgsw {
sw_fill_fn sw_fill_get_K1P_SEMIGLOBAL(bool, int lp, int r, int which) {
    constexpr int XP_ = pk16::CI, XS_ = pk16::CI, YP_ = pk16::CZ, YS_ = pk16::CZ;
    constexpr bool LF_ = false, FR_ = false;
    BG_K1P_SHAPES(BG_PK16_CASE)
    return nullptr;
}
}  // namespace bgsw
