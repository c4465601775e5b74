// The per-slot decisions of the SAM writer (sam_emit.hip) and the bodies of the calls behind it (sam_sort.hip:
// bg_sam_markdup[_dev], bg_sam_sort_keys[_dev], bg_sam_sort[_dev]; the rules are in include/biogpu.h) as __host__ __device__
// functions, so that the writer, the duplicate marker and the key pass share ONE definition of "placed" and of "writes a
// line", and so that tests/sam_sort_host_bodies.cpp can run them on the CPU under AddressSanitizer.
//   * placement:     sam_rule_place, sam_rule_writes
//   * the sort key:  sam_rule_key
//   * duplicates:    md_score_share (a lane's share of a read's score), md_end (the unclipped 5' end), md_end_entry /
//                    md_pair_entry (what is sorted), md_less (a TOTAL order: the rule's ties by index are part of it, so no
//                    property of the sort shows in the result), md_same_group + md_flagged (the pass over runs)
//   * the copy:      sam_copy_plan (head, aligned body, tail of a line at its destination) and sam_copy_vec (16 destination-
//                    aligned bytes out of a source that is misaligned against it by any amount).  Every source byte read
//                    lies inside the line.
#ifndef BG_SAM_RULE_H
#define BG_SAM_RULE_H
#include <hip/hip_runtime.h>

#include <cstdint>

#include "biogpu.h"

#define SAM_HD __host__ __device__ inline

// ---- placement --------------------------------------------------------------------------------------------------------
// the contig a hit is placed on, -1 if it is not placed: a scored hit whose [ref_start, ref_end) lies inside one contig
SAM_HD int64_t sam_rule_place(const bg_sam_contig_t* contigs, uint64_t n_contigs, const bg_seed_hit_t& h, uint8_t strand) {
    if (h.aln.score == BG_MIN_SCORE || strand == BG_HIT_NONE) return -1;
    const uint64_t s = h.ref_start, e = h.ref_end;
    uint64_t lo = 0, hi = n_contigs;  // the first contig that starts behind s
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (contigs[mid].start <= s) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return -1;
    const uint64_t end = contigs[lo - 1].start + contigs[lo - 1].len;
    return s < end && s <= e && e <= end ? (int64_t)(lo - 1) : -1;
}
// slot k of a read writes a line: slot 0 always, a later one only with BG_SAM_SECONDARY when it and slot 0 are placed
SAM_HD bool sam_rule_writes(uint32_t flags, uint32_t k, bool placed, bool slot0_placed) {
    return k == 0 || ((flags & BG_SAM_SECONDARY) && placed && slot0_placed);
}

// ---- bg_sam_sort_keys: the key of slot K r + k ----------------------------------------------------------------------------
SAM_HD uint64_t sam_rule_key(uint32_t flags, uint32_t K, const bg_sam_contig_t* contigs, uint64_t n_contigs, const bg_seed_hit_t* hits,
                             const uint8_t* strand, uint64_t slot) {
    const uint64_t r = slot / K;
    const uint32_t k = (uint32_t)(slot - r * K);
    const bool placed = sam_rule_place(contigs, n_contigs, hits[slot], strand[slot]) >= 0;
    const bool slot0 = k == 0 ? placed : sam_rule_place(contigs, n_contigs, hits[r * K], strand[r * K]) >= 0;
    if (!sam_rule_writes(flags, k, placed, slot0)) return UINT64_MAX;
    if (placed) return hits[slot].ref_start;
    if (flags & BG_SAM_PAIRED) {  // K == 1: the mate's slot is the neighbouring read's; the line borrows its RNAME and POS
        const uint64_t m = slot ^ 1;
        if (sam_rule_place(contigs, n_contigs, hits[m], strand[m]) >= 0) return hits[m].ref_start;
    }
    return UINT64_MAX;
}

// ---- bg_sam_markdup -------------------------------------------------------------------------------------------------------
#define MD_G 16u  // lanes per read in the score kernel

// this lane's share of score(r): symbols lane, lane + G, ...; the group sums the shares (32-bit, wrapping)
SAM_HD uint32_t md_score_share(const uint8_t* q, uint32_t len, uint32_t phred_offset, uint32_t min_qual, uint32_t lane, uint32_t G) {
    uint32_t s = 0;
    const uint64_t floor_q = (uint64_t)phred_offset + min_qual;
    for (uint64_t i = lane; i < len; i += G)
        if (q[i] >= floor_q) s += q[i] - phred_offset;
    return s;
}
SAM_HD uint32_t md_score_serial(const uint8_t* q, uint32_t len, uint32_t phred_offset, uint32_t min_qual) {
    return md_score_share(q, len, phred_offset, min_qual, 0, 1);
}

struct md_end_t {
    int64_t contig;  // -1: no end
    uint64_t u5;     // the unclipped 5' coordinate in the index text
    uint32_t rev;
};
SAM_HD md_end_t md_end(const bg_sam_contig_t* contigs, uint64_t n_contigs, const bg_seed_hit_t& h, uint8_t strand) {
    md_end_t e = {sam_rule_place(contigs, n_contigs, h, strand), 0, 0};
    if (e.contig < 0) return e;
    e.rev = strand == BG_HIT_REVERSE;
    if (e.rev) e.u5 = h.ref_end - 1 + (uint64_t)(h.aln.xlen - h.aln.xend);
    else e.u5 = h.ref_start >= h.aln.xstart ? h.ref_start - h.aln.xstart : 0;
    return e;
}
// (contig, u5, rev, mate number) of a before that of b
SAM_HD bool md_end_before(const md_end_t& a, uint32_t mate_a, const md_end_t& b, uint32_t mate_b) {
    if (a.contig != b.contig) return a.contig < b.contig;
    if (a.u5 != b.u5) return a.u5 < b.u5;
    if (a.rev != b.rev) return a.rev < b.rev;
    return mate_a < mate_b;
}

// What is sorted: k[0 .. 3] name the group (and, for an end, k[2] its kind), then the inverted score, then the index.
// An entry that takes no part has k[0] = MD_NONE and sorts behind every other.
#define MD_NONE 0xFFFFFFFFFFFFFFFFull
enum { MD_KIND_PAIR_END = 0, MD_KIND_FRAGMENT = 1 };  // an end of a both-ended pair; a fragment's (or a single read's) end
struct md_entry_t {
    uint64_t k[4];
    uint64_t inv_score;  // UINT64_MAX - score: the highest score first
    uint64_t idx;        // the read r or the pair p: the smallest first
};
SAM_HD md_entry_t md_none(uint64_t idx) { return {{MD_NONE, MD_NONE, MD_NONE, MD_NONE}, MD_NONE, idx}; }
SAM_HD uint64_t md_end_word(const md_end_t& e) { return ((uint64_t)e.contig << 1) | e.rev; }
// the entry of read r in the sort over ends: groups are (contig, rev, u5), the ends of pairs in front of the fragments'
SAM_HD md_entry_t md_end_entry(const md_end_t& e, uint32_t kind, uint32_t score, uint64_t r) {
    if (e.contig < 0) return md_none(r);
    return {{md_end_word(e), e.u5, kind, 0}, MD_NONE - score, r};
}
// the entry of pair p (both mates have an end) in the sort over pairs: the group is (lo, hi, whether lo is mate 2)
SAM_HD md_entry_t md_pair_entry(const md_end_t& e1, const md_end_t& e2, uint32_t score1, uint32_t score2, uint64_t p) {
    if (e1.contig < 0 || e2.contig < 0) return md_none(p);
    const bool lo_is_2 = md_end_before(e2, 2, e1, 1);
    const md_end_t& lo = lo_is_2 ? e2 : e1;
    const md_end_t& hi = lo_is_2 ? e1 : e2;
    return {{md_end_word(lo), lo.u5, (md_end_word(hi) << 1) | (lo_is_2 ? 1u : 0u), hi.u5}, MD_NONE - ((uint64_t)score1 + score2), p};
}
SAM_HD bool md_less(const md_entry_t& a, const md_entry_t& b) {
    for (int i = 0; i < 4; i++)
        if (a.k[i] != b.k[i]) return a.k[i] < b.k[i];
    if (a.inv_score != b.inv_score) return a.inv_score < b.inv_score;
    return a.idx < b.idx;
}
// words: 4 for pairs, 2 for ends (k[2], the kind, orders a group but does not split it)
SAM_HD bool md_same_group(const md_entry_t& a, const md_entry_t& b, int words) {
    for (int i = 0; i < words; i++)
        if (a.k[i] != b.k[i]) return false;
    return true;
}
// The pass over runs, for position i of the sorted entries: the entry is flagged if it takes part, is no pair's end, and its
// predecessor belongs to its group — the predecessor is then the group's winner, an earlier loser, or (ends) a pair's end.
SAM_HD bool md_flagged(const md_entry_t* sorted, uint64_t i, int words) {
    const md_entry_t& e = sorted[i];
    if (e.k[0] == MD_NONE || i == 0) return false;
    if (words == 2 && e.k[2] != MD_KIND_FRAGMENT) return false;
    return md_same_group(sorted[i - 1], e, words);
}
// ... and whether a flagged end owes its flag to a pair's end: the first entry of its group is one (binary search)
SAM_HD bool md_group_has_pair_end(const md_entry_t* sorted, uint64_t i) {
    const md_entry_t& e = sorted[i];
    uint64_t lo = 0, hi = i;  // the first position whose (k[0], k[1]) is not below e's
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const md_entry_t& m = sorted[mid];
        if (m.k[0] < e.k[0] || (m.k[0] == e.k[0] && m.k[1] < e.k[1])) lo = mid + 1;
        else hi = mid;
    }
    return sorted[lo].k[2] == MD_KIND_PAIR_END;
}

// ---- bg_sam_sort: the permuted copy ---------------------------------------------------------------------------------------
// A line of len bytes whose destination address is dst_mis mod 16: `head` bytes up to the first 16-byte boundary, `body`
// aligned 16-byte stores, `tail` bytes behind the last one.
#define SAM_LONG_LINE 16384u  // bytes: a longer line is cut into chunks that blocks take, a shorter one is a group's
#define SAM_CHUNK_VECS 256u   // 16-byte vectors of a long line in a chunk
#define SAM_COPY_G 16u        // lanes of the group that serves an ordinary line
struct sam_copy_plan_t {
    uint32_t head, tail;
    uint64_t body;
};
SAM_HD sam_copy_plan_t sam_copy_plan(uint32_t dst_mis, uint64_t len) {
    sam_copy_plan_t p;
    const uint32_t to_boundary = (16u - dst_mis) & 15u;
    p.head = len < to_boundary ? (uint32_t)len : to_boundary;
    p.body = (len - p.head) >> 4;
    p.tail = (uint32_t)((len - p.head) & 15u);
    return p;
}
struct alignas(16) sam_v16 {
    uint32_t w[4];
};
// bytes [sh, sh + 4) of the 8 bytes lo (first), hi
SAM_HD uint32_t sam_align_bytes(uint32_t lo, uint32_t hi, uint32_t sh) { return sh ? (lo >> (8 * sh)) | (hi << (32 - 8 * sh)) : lo; }
// The 16 bytes at p, which lie inside the line [lb, le).  Where the two 16-byte granules around p lie inside the line as
// well they are loaded whole and shifted; otherwise (the line's first and last vectors) the bytes are loaded one by one.
SAM_HD sam_v16 sam_copy_vec(const uint8_t* p, const uint8_t* lb, const uint8_t* le) {
    const uint32_t sh = (uint32_t)((uintptr_t)p & 15u);
    const uint8_t* q = p - sh;
    sam_v16 r;
    if (sh == 0) return *(const sam_v16*)q;
    if (q >= lb && q + 32 <= le) {
        const sam_v16 a = *(const sam_v16*)q, b = *(const sam_v16*)(q + 16);
        const uint32_t w[8] = {a.w[0], a.w[1], a.w[2], a.w[3], b.w[0], b.w[1], b.w[2], b.w[3]};
        const uint32_t ws = sh >> 2, bs = sh & 3u;
        for (int i = 0; i < 4; i++) {
            uint32_t lo = 0, hi = 0;
            for (uint32_t s = 0; s < 4; s++)  // (a select chain: ws is the same for a whole line, no register is indexed)
                if (ws == s) {
                    lo = w[i + s];
                    hi = w[i + s + 1];
                }
            r.w[i] = sam_align_bytes(lo, hi, bs);
        }
        return r;
    }
    for (int i = 0; i < 4; i++) r.w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
    return r;
}
// Lane `lane` of a group of G copies its share of the line src[0 .. len) to dst: body vectors v0 <= v < v1 (clamped to the
// plan's), and, with `ends`, the head and tail bytes.  A group that serves a whole line passes 0, UINT64_MAX, true; a long
// line is cut into ranges of vectors, one of which brings the ends.
SAM_HD void sam_copy_line(const uint8_t* src, uint8_t* dst, uint64_t len, uint32_t lane, uint32_t G, uint64_t v0, uint64_t v1, bool ends) {
    const sam_copy_plan_t p = sam_copy_plan((uint32_t)((uintptr_t)dst & 15u), len);
    if (ends) {
        for (uint32_t i = lane; i < p.head; i += G) dst[i] = src[i];
        const uint64_t t = p.head + 16 * p.body;
        for (uint32_t i = lane; i < p.tail; i += G) dst[t + i] = src[t + i];
    }
    const uint64_t stop = v1 < p.body ? v1 : p.body;
    for (uint64_t v = v0 + lane; v < stop; v += G) *(sam_v16*)(dst + p.head + 16 * v) = sam_copy_vec(src + p.head + 16 * v, src, src + len);
}

#endif
