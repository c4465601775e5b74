// K1p instantiations for Aligner::local (mod.rs:995-999) with gap_open < 0 and mismatch < 0: the LF flavour
// (sw_fill_pk16.inc) — the fold of the x-suffix clip only where column n is computed, the floor 0 by saturation — and its
// framed cell (FR: keys in the offset frame of pk16_frame_bias, for the scorings and lengths pk16_frame_fits admits), with
// the best key by v_pk_max_i16 (FR = 1) or, where pk16_max3_fits keeps every key a finite half and a match within 256 key
// units of a mismatch, the cell of v_pk_maximum3_f16 (FR = 2: the floor through D, the match term by a saturating subtract,
// paired row maxima).
#include "sw_fill_pk16.inc"
namespace bgsw {
sw_fill_fn sw_fill_get_K1P_LF(bool, int lp, int r, int which) {
    constexpr int XP_ = pk16::CZ, XS_ = pk16::CZ, YP_ = pk16::CZ, YS_ = pk16::CZ;
    constexpr bool LF_ = true;
    constexpr int FR_ = 0;
    BG_K1P_LOCAL_SHAPES(BG_PK16_CASE)
    return nullptr;
}
sw_fill_fn sw_fill_get_K1P_LF_FRAMED(bool, int lp, int r, int which) {
    constexpr int XP_ = pk16::CZ, XS_ = pk16::CZ, YP_ = pk16::CZ, YS_ = pk16::CZ;
    constexpr bool LF_ = true;
    constexpr int FR_ = 1;
    BG_K1P_LOCAL_SHAPES(BG_PK16_CASE)
    return nullptr;
}
sw_fill_fn sw_fill_get_K1P_LF_FRAMED_MAX3(bool, int lp, int r, int which) {
    constexpr int XP_ = pk16::CZ, XS_ = pk16::CZ, YP_ = pk16::CZ, YS_ = pk16::CZ;
    constexpr bool LF_ = true;
    constexpr int FR_ = 2;
    BG_K1P_LOCAL_SHAPES(BG_PK16_CASE)
    return nullptr;
}
}  // namespace bgsw
