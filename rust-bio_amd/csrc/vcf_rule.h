// The bodies behind the VCF writer (vcf_emit.hip: bg_vcf_emit[_dev]; THE RULE is in include/biogpu.h) as __host__ __device__
// functions, so that the kernels and tests/vcf_host_bodies.cpp, which runs them on the CPU under AddressSanitizer, share ONE
// definition of which element is refused, of what a line holds and of where it goes.
//   * numbers:   vcf_ndig, vcf_put_dec
//   * bytes:     vcf_upper, vcf_ref_byte (R of the rule), vcf_ins_byte (S of the rule)
//   * checks:    vcf_site_ok, vcf_event_ok: every refusal of the rule for one element, its predecessor included
//   * a line:    vcf_line_t: what a line is made of and where its fields start; vcf_site_line, vcf_event_line
//   * the order: vcf_key_less, vcf_events_before (lower bound), vcf_sites_upto (upper bound)
//   * the text:  vcf_put_lane: a lane's share of a line, into LDS or global memory
#ifndef BG_VCF_RULE_H
#define BG_VCF_RULE_H
#include "sam_rule.h"

static_assert(sizeof(bg_vcf_params_t) == 8 && sizeof(bg_bam_site_t) == 32 && sizeof(bg_bam_indel_t) == 40, "the boundary's structs");

#define VCF_NONE 0xFFFFFFFFFFFFFFFFull
#define VCF_ROLES 8u  // the fixed pieces of a line; lane (role % G) of a group writes a role

// ---- numbers ----------------------------------------------------------------------------------------------------------------
SAM_HD uint32_t vcf_ndig(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10) {
        v /= 10;
        n++;
    }
    return n;
}
// v in n = vcf_ndig(v) decimal digits
template <class Dst>
SAM_HD void vcf_put_dec(Dst d, uint64_t v, uint32_t n) {
    for (uint32_t i = n; i-- > 0;) {
        d[i] = (char)('0' + v % 10);
        v /= 10;
    }
}

// ---- bytes ------------------------------------------------------------------------------------------------------------------
SAM_HD uint8_t vcf_upper(uint8_t b) { return b >= 'a' && b <= 'z' ? (uint8_t)(b - 32) : b; }
// R: a reference byte as REF shows it (VCF v4.3: an IUPAC code becomes the first base, alphabetically, that it stands for)
SAM_HD uint8_t vcf_ref_byte(uint8_t b) {
    switch (vcf_upper(b)) {
        case 'A': case 'M': case 'R': case 'W': case 'D': case 'H': case 'V': return 'A';
        case 'C': case 'Y': case 'S': case 'B': return 'C';
        case 'G': case 'K': return 'G';
        case 'T': return 'T';
        default: return 'N';
    }
}
// S: an inserted byte as ALT shows it
SAM_HD uint8_t vcf_ins_byte(uint8_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T' ? b : (uint8_t)'N'; }

// ---- the inputs of a call ---------------------------------------------------------------------------------------------------
struct vcf_args_t {
    const bg_bam_site_t* sites;  // 4-byte aligned
    uint64_t n_sites;
    const bg_bam_indel_t* events;  // 8-byte aligned
    uint64_t n_events;
    const uint8_t* seq;
    uint64_t n_seq;
    const bg_sam_contig_t* contigs;
    uint64_t n_contigs;
    const char* names;
    const uint8_t* text;
    uint64_t n_text;
};

// ---- the order --------------------------------------------------------------------------------------------------------------
SAM_HD bool vcf_key_less(uint32_t region_a, int32_t pos_a, uint32_t region_b, int32_t pos_b) {
    return region_a != region_b ? region_a < region_b : pos_a < pos_b;
}
// the events in front of a site's line: those with a smaller (region, pos)
SAM_HD uint64_t vcf_events_before(const bg_bam_indel_t* events, uint64_t n, uint32_t region, int32_t pos) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (vcf_key_less(events[mid].region, events[mid].pos, region, pos)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// the sites whose lines come in front of an event's: those with a (region, pos) that is not greater
SAM_HD uint64_t vcf_sites_upto(const bg_bam_site_t* sites, uint64_t n, uint32_t region, int32_t pos) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (!vcf_key_less(region, pos, sites[mid].region, sites[mid].pos)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- checks -----------------------------------------------------------------------------------------------------------------
// what every element must satisfy: a contig of the table that lies inside the text, a position on it.  Reads no text byte.
SAM_HD bool vcf_place_ok(const vcf_args_t& a, int32_t ref, int32_t pos) {
    if (ref < 0 || (uint64_t)ref >= a.n_contigs) return false;
    const bg_sam_contig_t& c = a.contigs[ref];
    if (c.start > a.n_text || c.len > a.n_text - c.start) return false;
    return pos >= 0 && (uint64_t)pos < c.len;
}
SAM_HD bool vcf_site_ok(const vcf_args_t& a, uint64_t i) {
    const bg_bam_site_t& s = a.sites[i];
    if (!vcf_place_ok(a, s.ref, s.pos) || s.kind > BG_SITE_INS || s.reserved) return false;
    if (i && vcf_key_less(s.region, s.pos, a.sites[i - 1].region, a.sites[i - 1].pos)) return false;
    if (s.kind != BG_SITE_SNV) return true;
    if (s.ref_base != vcf_upper(a.text[a.contigs[s.ref].start + (uint64_t)s.pos])) return false;
    return (s.alt == 'A' || s.alt == 'C' || s.alt == 'G' || s.alt == 'T') && s.alt != s.ref_base;
}
SAM_HD bool vcf_event_ok(const vcf_args_t& a, uint64_t j) {
    const bg_bam_indel_t& e = a.events[j];
    if (!vcf_place_ok(a, e.ref, e.pos) || (e.kind != BG_SITE_DEL && e.kind != BG_SITE_INS)) return false;
    if (e.reserved[0] | e.reserved[1] | e.reserved[2]) return false;
    if (j && vcf_key_less(e.region, e.pos, a.events[j - 1].region, a.events[j - 1].pos)) return false;
    if (e.len == 0) return false;
    if (e.kind == BG_SITE_DEL) return (uint64_t)e.pos + e.len < a.contigs[e.ref].len;  // the last deleted base is on the contig
    return e.seq_off <= a.n_seq && e.len <= a.n_seq - e.seq_off;
}

// ---- a line -----------------------------------------------------------------------------------------------------------------
// CHROM \t POS \t . \t REF \t ALT \t . \t . \t DP=d [;RO=r] ;AO=a ;SAF=f ;SAR=r ;TYPE=xxx \n
struct vcf_line_t {
    uint32_t kind;               // BG_SITE_*
    uint32_t name_len;
    uint64_t name_off;
    uint64_t pos1;               // POS
    uint64_t anchor;             // the text index of R(pos)
    uint64_t seq_at;             // INS: its bytes in seq
    uint32_t n;                  // DEL: the bytes of REF behind the anchor; INS: those of ALT; SNV: 0
    uint32_t depth, ro, saf, sar;
    uint8_t alt;                 // SNV: ALT
    uint64_t ao;
    // where the fields start; len is the whole line with its newline, 64-bit: a deletion has no bound below the contig's length
    uint64_t at_pos, at_ref, at_alt, at_dp, at_ro, at_ao, at_saf, at_sar, at_type, len;
};
SAM_HD void vcf_layout(vcf_line_t& L) {
    const uint64_t ref_len = 1 + (L.kind == BG_SITE_DEL ? (uint64_t)L.n : 0), alt_len = 1 + (L.kind == BG_SITE_INS ? (uint64_t)L.n : 0);
    L.at_pos = (uint64_t)L.name_len + 1;
    L.at_ref = L.at_pos + vcf_ndig(L.pos1) + 3;  // "\t.\t"
    L.at_alt = L.at_ref + ref_len + 1;
    L.at_dp = L.at_alt + alt_len + 5;            // "\t.\t.\t"
    L.at_ro = L.at_dp + 3 + vcf_ndig(L.depth);   // "DP="
    L.at_ao = L.at_ro + (L.kind == BG_SITE_SNV ? 4 + vcf_ndig(L.ro) : 0);  // ";RO="
    L.at_saf = L.at_ao + 4 + vcf_ndig(L.ao);     // ";AO="
    L.at_sar = L.at_saf + 5 + vcf_ndig(L.saf);   // ";SAF="
    L.at_type = L.at_sar + 5 + vcf_ndig(L.sar);  // ";SAR="
    L.len = L.at_type + 10;                      // ";TYPE=snp\n"
}
// the line of an SNV site / of an event that passed its check
SAM_HD vcf_line_t vcf_site_line(const vcf_args_t& a, uint64_t i) {
    const bg_bam_site_t& s = a.sites[i];
    const bg_sam_contig_t& c = a.contigs[s.ref];
    vcf_line_t L = {};
    L.kind = BG_SITE_SNV;
    L.name_len = c.name_len;
    L.name_off = c.name_off;
    L.pos1 = (uint64_t)s.pos + 1;
    L.anchor = c.start + (uint64_t)s.pos;
    L.depth = s.depth;
    L.ro = s.ref_count;
    L.saf = s.alt_fwd;
    L.sar = s.alt_rev;
    L.ao = (uint64_t)s.alt_fwd + s.alt_rev;
    L.alt = s.alt;
    vcf_layout(L);
    return L;
}
SAM_HD vcf_line_t vcf_event_line(const vcf_args_t& a, uint64_t j) {
    const bg_bam_indel_t& e = a.events[j];
    const bg_sam_contig_t& c = a.contigs[e.ref];
    vcf_line_t L = {};
    L.kind = e.kind;
    L.name_len = c.name_len;
    L.name_off = c.name_off;
    L.pos1 = (uint64_t)e.pos + 1;
    L.anchor = c.start + (uint64_t)e.pos;
    L.seq_at = e.seq_off;
    L.n = e.len;
    L.depth = e.depth;
    L.saf = e.alt_fwd;
    L.sar = e.alt_rev;
    L.ao = (uint64_t)e.alt_fwd + e.alt_rev;
    vcf_layout(L);
    return L;
}
// element e of the combined list (sites, then events)
SAM_HD vcf_line_t vcf_line_of(const vcf_args_t& a, uint64_t e) { return e < a.n_sites ? vcf_site_line(a, e) : vcf_event_line(a, e - a.n_sites); }

// ---- the text ---------------------------------------------------------------------------------------------------------------
// Lane `lane` of G: its bytes of line L at dst[0 .. L.len).  fold: the 256 entries of vcf_ref_byte.  The names, the deleted
// reference bytes and the inserted bytes are strided over the lanes; each of the VCF_ROLES fixed pieces belongs to one lane.
// Every byte of the line is written exactly once, and no byte outside it.
template <class Dst>
SAM_HD void vcf_put_lane(const vcf_args_t& a, const vcf_line_t& L, const uint8_t* fold, Dst dst, uint32_t lane, uint32_t G) {
    for (uint64_t i = lane; i < L.name_len; i += G) dst[i] = a.names[L.name_off + i];
    if (L.kind == BG_SITE_DEL)
        for (uint64_t i = lane; i < L.n; i += G) dst[L.at_ref + 1 + i] = (char)fold[a.text[L.anchor + 1 + i]];
    if (L.kind == BG_SITE_INS)
        for (uint64_t i = lane; i < L.n; i += G) dst[L.at_alt + 1 + i] = (char)vcf_ins_byte(a.seq[L.seq_at + i]);
    auto lit = [&](uint64_t at, const char* s, uint32_t n) {
        for (uint32_t i = 0; i < n; i++) dst[at + i] = s[i];
    };
    auto mine = [&](uint32_t role) { return role % G == lane; };
    if (mine(0)) {
        dst[L.at_pos - 1] = '\t';
        vcf_put_dec(dst + L.at_pos, L.pos1, vcf_ndig(L.pos1));
        lit(L.at_ref - 3, "\t.\t", 3);
    }
    if (mine(1)) {
        const uint8_t r = fold[a.text[L.anchor]];
        dst[L.at_ref] = (char)r;
        dst[L.at_alt - 1] = '\t';
        dst[L.at_alt] = (char)(L.kind == BG_SITE_SNV ? L.alt : r);
        lit(L.at_dp - 5, "\t.\t.\t", 5);
    }
    if (mine(2)) {
        lit(L.at_dp, "DP=", 3);
        vcf_put_dec(dst + L.at_dp + 3, L.depth, vcf_ndig(L.depth));
    }
    if (mine(3) && L.kind == BG_SITE_SNV) {
        lit(L.at_ro, ";RO=", 4);
        vcf_put_dec(dst + L.at_ro + 4, L.ro, vcf_ndig(L.ro));
    }
    if (mine(4)) {
        lit(L.at_ao, ";AO=", 4);
        vcf_put_dec(dst + L.at_ao + 4, L.ao, vcf_ndig(L.ao));
    }
    if (mine(5)) {
        lit(L.at_saf, ";SAF=", 5);
        vcf_put_dec(dst + L.at_saf + 5, L.saf, vcf_ndig(L.saf));
    }
    if (mine(6)) {
        lit(L.at_sar, ";SAR=", 5);
        vcf_put_dec(dst + L.at_sar + 5, L.sar, vcf_ndig(L.sar));
    }
    if (mine(7)) lit(L.at_type, L.kind == BG_SITE_SNV ? ";TYPE=snp\n" : L.kind == BG_SITE_DEL ? ";TYPE=del\n" : ";TYPE=ins\n", 10);
}

#endif
