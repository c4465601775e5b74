// K1p instantiations for Aligner::custom (mod.rs:591): any clip penalties.
#include "sw_fill_pk16.inc"
namespace bgsw {
sw_fill_fn sw_fill_get_K1P_CUSTOM(bool, int lp, int r, int which) {
    constexpr int XP_ = pk16::CF, XS_ = pk16::CF, YP_ = pk16::CF, YS_ = pk16::CF;
    constexpr bool LF_ = false, FR_ = false;
    BG_K1P_SHAPES(BG_PK16_CASE)
    return nullptr;
}
}  // namespace bgsw
