// The bodies behind the BAI index (bam_index.hip: bg_bam_index[_dev]; THE RULE is in include/biogpu.h) as __host__ __device__
// functions, so that the kernels and tests/bam_index_host_bodies.cpp, which runs them on the CPU under AddressSanitizer,
// share ONE definition of what a record contributes and of where every byte of the index lies.
//   * a record:      bai_get16 / bai_get32 (little-endian fields at any address), bai_decode (the fixed fields, the CIGAR walk
//                    for `end`, every check of the rule that needs one record only, the bin by bam_reg2bin), bai_before (the
//                    order two neighbours must be in)
//   * an offset:     bai_voff, with a block table or by the closed form of bg_bgzf_frame
//   * the keys:      bai_chunk_key ((ref, bin): what the chunk list is sorted by), bai_end_key ((ref, end): its running
//                    maximum over the sorted records is, inside a reference, the prefix maximum of `end`)
//   * the layout:    bai_n_intv, bai_ref_bytes (a reference's bytes from its bins, chunks and windows), bai_bin_at,
//                    bai_pseudo_at, bai_intv_at (where its pieces start), bai_total
//   * the bytes:     bai_put32 / bai_put64, bai_put_head, bai_put_bin, bai_put_chunk, bai_put_pseudo, bai_put_empty_ref
//   * a window:      bai_window_first: the first record of a reference whose prefix maximum of `end` exceeds w << 14
#ifndef BG_BAM_INDEX_RULE_H
#define BG_BAM_INDEX_RULE_H
#include "bam_rule.h"

#define BAI_PSEUDO_BIN 37450u
#define BAI_MAX_END 536870912ll  // 2^29: where BAI's bins stop
#define BAI_LINEAR_SHIFT 14
#define BAI_NONE 0xFFFFFFFFFFFFFFFFull
#define BAI_FRAME_BLOCK (BGZF_PAYLOAD + BGZF_EXTRA)  // bytes of a full stored block
enum { BAI_OK = 0, BAI_INVALID = 1, BAI_UNSUPPORTED = 2 };

SAM_HD uint32_t bai_get16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
SAM_HD uint32_t bai_get32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// what the index keeps of one record; 24 bytes
struct bai_rec_t {
    uint64_t slot;
    int32_t ref, pos;
    uint32_t end;    // at most 2^29 where the record passed its checks
    uint32_t binf;   // the bin, bit 16: FLAG 0x4 is set
};
#define BAI_UNMAPPED_BIT 0x10000u

// The record rec[0 .. len), len > 0, against the contig table.  Reads no byte outside it.  Returns BAI_OK and fills *r (slot
// is left alone), or the kind of the first check that fails: the INVALID ones come first, so that a record is UNSUPPORTED
// only if nothing else is wrong with it.
SAM_HD int bai_decode(const uint8_t* rec, uint64_t len, const bg_sam_contig_t* contigs, uint64_t n_contigs, bai_rec_t* r) {
    r->ref = -1;
    r->pos = -1;
    r->end = 0;
    r->binf = BAM_UNMAPPED_BIN;
    if (len < BAM_FIXED) return BAI_INVALID;
    if ((uint64_t)bai_get32(rec) + 4 != len) return BAI_INVALID;
    const int32_t ref = (int32_t)bai_get32(rec + 4), pos = (int32_t)bai_get32(rec + 8);
    const uint32_t l_name = rec[12], n_cigar = bai_get16(rec + 16), flag = bai_get16(rec + 18);
    const uint64_t l_seq = bai_get32(rec + 20);
    const uint64_t cigar_at = BAM_FIXED + l_name;
    if (cigar_at + 4ull * n_cigar + (l_seq + 1) / 2 + l_seq > len) return BAI_INVALID;
    if (ref >= 0 && (uint64_t)ref >= n_contigs) return BAI_INVALID;
    if (pos < -1) return BAI_INVALID;
    r->ref = ref;
    r->pos = pos;
    if (flag & 4u) r->binf |= BAI_UNMAPPED_BIT;
    if (ref < 0) return BAI_OK;  // counts into n_no_coor only
    uint64_t span = 0;
    for (uint32_t k = 0; k < n_cigar; k++) {
        const uint32_t w = bai_get32(rec + cigar_at + 4ull * k), op = w & 15u;
        if (op == 0 || op == BAM_CIGAR_D || op == BAM_CIGAR_N || op == BAM_CIGAR_EQ || op == BAM_CIGAR_X) span += w >> 4;
    }
    const int64_t end = (int64_t)pos + (int64_t)(span ? span : 1);
    if (end > 0 && (uint64_t)end > contigs[ref].len) return BAI_INVALID;
    if (end > BAI_MAX_END) return BAI_UNSUPPORTED;
    r->end = (uint32_t)end;
    r->binf = bam_reg2bin(pos, end) | (r->binf & BAI_UNMAPPED_BIT);
    return BAI_OK;
}
// record b directly behind record a: does b sort before a by ((uint32) refID, pos)?
SAM_HD bool bai_before(const bai_rec_t& b, const bai_rec_t& a) {
    return (uint32_t)b.ref < (uint32_t)a.ref || (b.ref == a.ref && b.pos < a.pos);
}

// the virtual offset of byte o of the stream (o may be the stream's length: the table's last entry serves a multiple of 65 280)
SAM_HD uint64_t bai_voff(uint64_t o, const uint64_t* block_off, uint64_t base) {
    const uint64_t b = o / BGZF_PAYLOAD, within = o % BGZF_PAYLOAD;
    return ((base + (block_off ? block_off[b] : b * BAI_FRAME_BLOCK)) << 16) | within;
}
// ... of a stream in any framing (bg_bam_index_blocks), from the tables bg_bgzf_blocks fills (n_blocks + 1 rows each): the first
// block whose payload ends behind o; where there is none (o is the stream's length) the first block whose payload starts at o,
// the closing row if no block does.  Empty members in front of a byte are skipped, the stream's end points at the end-of-file
// block where there is one.
SAM_HD uint64_t bai_voff_blocks(uint64_t o, uint64_t n_blocks, const uint64_t* block_off, const uint64_t* out_off) {
    uint64_t lo = 0, hi = n_blocks;  // the first b with out_off[b + 1] > o
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (out_off[mid + 1] > o) hi = mid;
        else lo = mid + 1;
    }
    if (lo == n_blocks) {  // the first b with out_off[b] >= o (== o: o is the stream's length)
        lo = 0;
        hi = n_blocks;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (out_off[mid] >= o) hi = mid;
            else lo = mid + 1;
        }
    }
    return (block_off[lo] << 16) | (o - out_off[lo]);
}
// the three ways: a table of any framing (out_off given), bg_bgzf_deflate's table, bg_bgzf_frame's closed form
SAM_HD uint64_t bai_voff_any(uint64_t o, const uint64_t* block_off, uint64_t base, uint64_t n_blocks, const uint64_t* out_off) {
    return out_off ? bai_voff_blocks(o, n_blocks, block_off, out_off) : bai_voff(o, block_off, base);
}

SAM_HD uint64_t bai_chunk_key(int32_t ref, uint32_t binf) { return ((uint64_t)(uint32_t)ref << 16) | (binf & 0xFFFFu); }
#define BAI_KEY_BITS 48u                 // a key of a chunk lies below 2^47
#define BAI_KEY_PAD (1ull << 47)         // ... and this one, of an entry behind the last chunk, above them all
SAM_HD uint64_t bai_end_key(const bai_rec_t& r) { return ((uint64_t)(uint32_t)r.ref << 32) | r.end; }

SAM_HD uint64_t bai_n_intv(uint32_t max_end) { return max_end ? (((uint64_t)max_end - 1) >> BAI_LINEAR_SHIFT) + 1 : 0; }
// A reference with records: n_bin, its bins (bin, n_chunk, the chunks), the pseudo-bin (bin, n_chunk = 2, two chunks), n_intv,
// the offsets.  One without: n_bin = 0, n_intv = 0.
SAM_HD uint64_t bai_bin_at(uint64_t bins_before, uint64_t chunks_before) { return 4 + 8 * bins_before + 16 * chunks_before; }
SAM_HD uint64_t bai_pseudo_at(uint64_t n_bins, uint64_t n_chunks) { return bai_bin_at(n_bins, n_chunks); }
SAM_HD uint64_t bai_intv_at(uint64_t n_bins, uint64_t n_chunks) { return bai_pseudo_at(n_bins, n_chunks) + 40; }
SAM_HD uint64_t bai_ref_bytes(bool has_records, uint64_t n_bins, uint64_t n_chunks, uint64_t n_intv) {
    return has_records ? bai_intv_at(n_bins, n_chunks) + 4 + 8 * n_intv : 8;
}
// "BAI\1", n_ref, the references, n_no_coor
SAM_HD uint64_t bai_total(uint64_t ref_bytes) { return 8 + ref_bytes + 8; }

SAM_HD void bai_put32(uint8_t* d, uint32_t v) { bam_put32(d, v); }
SAM_HD void bai_put64(uint8_t* d, uint64_t v) {
    bam_put32(d, (uint32_t)v);
    bam_put32(d + 4, (uint32_t)(v >> 32));
}
SAM_HD void bai_put_head(uint8_t* out, uint64_t n_ref) {
    out[0] = 'B';
    out[1] = 'A';
    out[2] = 'I';
    out[3] = 1;
    bai_put32(out + 4, (uint32_t)n_ref);
}
SAM_HD void bai_put_bin(uint8_t* d, uint32_t bin, uint64_t n_chunk) {
    bai_put32(d, bin);
    bai_put32(d + 4, (uint32_t)n_chunk);
}
SAM_HD void bai_put_chunk(uint8_t* d, uint64_t beg, uint64_t end) {
    bai_put64(d, beg);
    bai_put64(d + 8, end);
}
// at ref + bai_pseudo_at(): the pseudo-bin, then n_intv
SAM_HD void bai_put_pseudo(uint8_t* d, uint64_t voff_first, uint64_t voff_last_end, uint64_t n_mapped, uint64_t n_unmapped, uint64_t n_intv) {
    bai_put_bin(d, BAI_PSEUDO_BIN, 2);
    bai_put_chunk(d + 8, voff_first, voff_last_end);
    bai_put_chunk(d + 24, n_mapped, n_unmapped);
    bai_put32(d + 40, (uint32_t)n_intv);
}
SAM_HD void bai_put_empty_ref(uint8_t* d) {
    bai_put32(d, 0);
    bai_put32(d + 4, 0);
}

// end_max[j] is the running maximum of bai_end_key over the sorted records; [first, last) are those of reference `ref`, whose
// maximum exceeds w << 14 at last - 1.  The first j in there whose prefix maximum of `end` exceeds w << 14.
SAM_HD uint64_t bai_window_first(const uint64_t* end_max, uint64_t first, uint64_t last, uint32_t ref, uint64_t w) {
    const uint64_t want = ((uint64_t)ref << 32) | (w << BAI_LINEAR_SHIFT);
    uint64_t lo = first, hi = last - 1;  // end_max[hi] > want
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (end_max[mid] > want) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

#endif
