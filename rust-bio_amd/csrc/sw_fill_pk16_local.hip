// K1p instantiations for Aligner::local (mod.rs:995-999): all four clip penalties 0.
#include "sw_fill_pk16.inc"
namespace bgsw {
sw_fill_fn sw_fill_get_K1P_LOCAL(bool, int lp, int r, int which) {
    constexpr int XP_ = pk16::CZ, XS_ = pk16::CZ, YP_ = pk16::CZ, YS_ = pk16::CZ;
    constexpr bool LF_ = false, FR_ = false;
    BG_K1P_LOCAL_SHAPES(BG_PK16_CASE)
    return nullptr;
}
}  // namespace bgsw
