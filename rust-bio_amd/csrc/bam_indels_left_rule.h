// The bodies behind the left-aligned indel events (bam_indels.hip: bg_bam_indels_left[_dev]; THE RULE is in include/biogpu.h) as
// __host__ __device__ functions, so that the kernels and tests/bam_indels_host_bodies.cpp (its left flavour), which runs them on the CPU under
// AddressSanitizer, share ONE definition of how far a raw event moves and of what its bytes are behind the move.  Everything in
// front of the shift and behind it is bam_indels_rule.h's (ind_raw_t, ind_depth, ind_is_kept, ind_event, ind_store).
//   * the walk:   inl_walk: ind_walk without the window's upper end: every raw event of a kept record whose RAW anchor is at or
//                 behind t0 and in front of t1 + max_shift (an event moves left only, by at most max_shift), with the record's pos
//   * the shift:  inl_shift_del / inl_shift_ins: the steps k a raw event takes against the contig's text; at most two byte loads
//                 a step, none in front of the record's pos + 1, none at or behind the contig's end
//   * the bytes:  inl_code: 4-bit code i of a shifted insertion; ind_raw_t carries the SHIFTED anchor and k in `reserved`
//   * the order:  inl_cmp: tile, shifted anchor, kind, len, then the shifted codes left to right
//   * placing:    inl_seq_lane: a lane's share of the ASCII bytes of a shifted insertion
// The identity behind inl_code.  Step j of an insertion is taken only if c_j == F(a - j), and c_j is s[n - 1 - j] for j < n and
// F(a - j + n) = F(a - (j - n)) = c_(j - n) beyond, so c_j = s[n - 1 - (j mod n)].  Byte i < min(k, n) of the shifted sequence is
// F(a' + 1 + i) = F(a - (k - 1 - i)) = c_(k - 1 - i) = s[(i - k) mod n], and byte i >= k is s[i - k]: the shifted sequence is s
// rotated right by k mod n, every byte of it a byte of the record, so neither the sort nor the placement reads the text and no
// rotated copy exists anywhere.  (A text base that entered has the code of its letter because it EQUALS the record's base.)
#ifndef BG_BAM_INDELS_LEFT_RULE_H
#define BG_BAM_INDELS_LEFT_RULE_H
#include "bam_indels_rule.h"
#include "bam_sites_rule.h"

static_assert(sizeof(bg_bam_indels_left_t) == 32, "the boundary's struct: bg_bam_indels_t and max_shift");

SAM_HD bg_bam_indels_t inl_indels_params(const bg_bam_indels_left_t& p) {
    bg_bam_indels_t q = {p.flags, p.require, p.exclude, p.min_mapq, p.min_baseq, p.reserved, p.min_depth, p.min_alt, p.min_alt_permille, p.min_alt_strand};
    return q;
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------
// The kept record rec: emit(kind, raw anchor, len, q, pos) for every raw event of bg_bam_indels whose raw anchor a has
// t0 <= a < t1 + max_shift.  One in front of t0 cannot land in [t0, t1) and costs no text read; one at or behind t1 may.
template <class Emit>
SAM_HD void inl_walk(const uint8_t* rec, uint32_t ref, int64_t t0, int64_t t1, uint32_t max_shift, Emit emit) {
    ind_walk_pos(rec, ref, t0, t1 + (int64_t)max_shift, emit);  // raw anchors at or behind t1 + max_shift stay at or behind t1
}

// ---- the shift --------------------------------------------------------------------------------------------------------------
SAM_HD bool inl_is_base(uint32_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
// text: the contig's first byte; clen: its length.  Reads text[a - k] (> pos) and text[a - k + n] (< clen) only.
SAM_HD uint32_t inl_shift_del(const uint8_t* text, int64_t clen, int64_t pos, int64_t a, int64_t n, uint32_t max_shift) {
    uint32_t k = 0;
    while (k < max_shift && a > pos && a + n < clen) {
        const uint32_t c = sit_fold(text[a]);
        if (c != sit_fold(text[a + n]) || !inl_is_base(c)) break;
        a--;
        k++;
    }
    return k;
}
// seq: the record's packed bases; q: the index of the insertion's first.  Reads text[a - k] (> pos) and, from step n on,
// text[a - k + n] (<= a), both inside the record's span of the contig.
SAM_HD uint32_t inl_shift_ins(const uint8_t* text, int64_t pos, int64_t a, int64_t n, const uint8_t* seq, uint64_t q, uint32_t max_shift) {
    uint32_t k = 0;
    while (k < max_shift && a - (int64_t)k > pos) {
        const uint32_t f = sit_fold(text[a - (int64_t)k]);
        const uint32_t c = (int64_t)k < n ? (uint32_t)(uint8_t)"=ACMGRSVTWYHKDBN"[ind_code(seq, q + (uint64_t)(n - 1 - (int64_t)k))] : (uint32_t)sit_fold(text[a - (int64_t)k + n]);
        if (c != f || !inl_is_base(f)) break;
        k++;
    }
    return k;
}

// ---- the bytes --------------------------------------------------------------------------------------------------------------
SAM_HD uint32_t inl_k(const ind_raw_t& e) { return e.reserved; }
// the index into the record's bases, from e.q, of byte i of the shifted insertion e: (i - k) mod len
SAM_HD uint32_t inl_rot(const ind_raw_t& e) { return e.len - inl_k(e) % e.len; }  // 1 .. len; added to i and reduced once
SAM_HD uint32_t inl_code(const ind_raw_t& e, const uint8_t* seq, uint32_t rot, uint32_t i) {
    const uint64_t j = (uint64_t)i + rot;
    return ind_code(seq, (uint64_t)e.q + (j >= e.len ? j - e.len : j));
}

// ---- the order --------------------------------------------------------------------------------------------------------------
// < 0, 0, > 0 as a sorts before, with, behind b.  Two raw events of different records and different k may be equal.
SAM_HD int inl_cmp(const ind_raw_t& a, const ind_raw_t& b, const uint8_t* recs, const uint64_t* off) {
    if (a.tile != b.tile) return a.tile < b.tile ? -1 : 1;
    if (a.anchor != b.anchor) return a.anchor < b.anchor ? -1 : 1;
    const uint32_t ka = ind_kind(a), kb = ind_kind(b);
    if (ka != kb) return ka < kb ? -1 : 1;
    if (a.len != b.len) return a.len < b.len ? -1 : 1;
    if (ka != BG_SITE_INS || (a.slot == b.slot && a.q == b.q && inl_k(a) == inl_k(b))) return 0;
    const uint8_t *sa = ind_seq_of(recs + off[a.slot]), *sb = ind_seq_of(recs + off[b.slot]);
    const uint32_t ra = inl_rot(a), rb = inl_rot(b);
    for (uint32_t j = 0; j < a.len; j++) {
        const uint32_t ca = inl_code(a, sa, ra, j), cb = inl_code(b, sb, rb, j);
        if (ca != cb) return ca < cb ? -1 : 1;
    }
    return 0;
}

// ---- placing ----------------------------------------------------------------------------------------------------------------
// Lane `lane` of G: its bytes of the shifted insertion e, ASCII, at dst[0 .. e.len)
SAM_HD void inl_seq_lane(const ind_raw_t& e, const uint8_t* recs, const uint64_t* off, uint8_t* dst, uint32_t lane, uint32_t G) {
    const uint8_t* seq = ind_seq_of(recs + off[e.slot]);
    const uint32_t rot = inl_rot(e);
    for (uint32_t j = lane; j < e.len; j += G) dst[j] = (uint8_t)"=ACMGRSVTWYHKDBN"[inl_code(e, seq, rot, j)];
}

#endif
