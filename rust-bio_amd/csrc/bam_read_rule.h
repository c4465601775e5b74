// The bodies behind reading BAM (bam_read.hip: bg_bam_header_parse, bg_bam_records[_dev], bg_bam_reads[_dev], bg_bam_sort_keys
// [_dev]; the rules are in include/biogpu.h) as __host__ __device__ functions, so that the kernels and
// tests/bam_read_host_bodies.cpp, which runs them on the CPU under AddressSanitizer, share ONE definition of what a record
// is and of every byte a read gets.
//   * the header:   bamr_header_parse: "BAM\1", the text, the reference table -> contigs, names, where the records start, or
//                   how long the prefix must at least be
//   * a position:   bamr_verdict: whether an accepted record stands at a position; bamr_slot_ok: whether a slot of a record
//                   table is exactly one
//   * a read:       bamr_fields (the fixed fields a read needs), bamr_kept (require / exclude), bamr_qual_len, bamr_base /
//                   bamr_seq_byte / bamr_qual_byte (one output byte), bamr_column_lane (a lane's share of a read's bases or
//                   qualities, stored 16 bytes wide between the destination's own 16-byte boundaries), bamr_read_record
//   * a key:        bamr_key
// Every field is read byte by byte: a stream may sit at any address.
#ifndef BG_BAM_READ_RULE_H
#define BG_BAM_READ_RULE_H
#include "bam_index_rule.h"

#define BAMR_MIN_RECORD 37u  // the 36 fixed bytes and a name that is its NUL
#define BAMR_MIN_REF 9u      // l_name, a NUL, l_ref
#define BAMR_NONE 0xFFFFFFFFu

// ---- the header -----------------------------------------------------------------------------------------------------------
struct bamr_header_t {
    uint64_t n_contigs, names_bytes, text_off, text_len, body_off;
    uint64_t need;  // BG_ERR_OPS_CAP: the smallest prefix length known to be required
};
// in[0 .. bytes): the start of an uncompressed BAM stream.  contigs / names may be null (nothing is written then); otherwise
// they hold what a first call counted.  BG_OK, BG_ERR_OPS_CAP (the prefix ends inside the header: h->need) or
// BG_ERR_INVALID_ARG.  A reference costs at least BAMR_MIN_REF bytes, so `need` counts that much for every one not yet seen.
inline int bamr_header_parse(const uint8_t* in, uint64_t bytes, bg_sam_contig_t* contigs, char* names, bamr_header_t* h) {
    *h = bamr_header_t{};
    if (bytes >= 4 && !(in[0] == 'B' && in[1] == 'A' && in[2] == 'M' && in[3] == 1)) return BG_ERR_INVALID_ARG;
    if (bytes < 8) {
        h->need = 12;
        return BG_ERR_OPS_CAP;
    }
    const int32_t l_text = (int32_t)bai_get32(in + 4);
    if (l_text < 0) return BG_ERR_INVALID_ARG;
    uint64_t at = 8 + (uint64_t)l_text;
    if (bytes < at + 4) {
        h->need = at + 4;
        return BG_ERR_OPS_CAP;
    }
    const int32_t n_ref = (int32_t)bai_get32(in + at);
    if (n_ref < 0) return BG_ERR_INVALID_ARG;
    at += 4;
    uint64_t start = 0, name_at = 0;
    for (uint64_t i = 0; i < (uint64_t)n_ref; i++) {
        const uint64_t rest = BAMR_MIN_REF * ((uint64_t)n_ref - i - 1);  // the references behind this one
        if (bytes < at + 4) {
            h->need = at + BAMR_MIN_REF + rest;
            return BG_ERR_OPS_CAP;
        }
        const int32_t l_name = (int32_t)bai_get32(in + at);
        if (l_name < 1) return BG_ERR_INVALID_ARG;
        if (bytes < at + 4 + (uint64_t)l_name + 4) {
            h->need = at + 4 + (uint64_t)l_name + 4 + rest;
            return BG_ERR_OPS_CAP;
        }
        if (in[at + 4 + (uint64_t)l_name - 1] != 0) return BG_ERR_INVALID_ARG;
        const int32_t l_ref = (int32_t)bai_get32(in + at + 4 + (uint64_t)l_name);
        if (l_ref < 0) return BG_ERR_INVALID_ARG;
        if (contigs) {
            bg_sam_contig_t c = {};
            c.start = start;
            c.len = (uint64_t)l_ref;
            c.name_off = name_at;
            c.name_len = (uint32_t)l_name - 1;
            contigs[i] = c;
        }
        if (names) memcpy(names + name_at, in + at + 4, (size_t)l_name - 1);
        start += (uint64_t)l_ref + 1;
        name_at += (uint64_t)l_name - 1;
        at += 4 + (uint64_t)l_name + 4;
    }
    h->n_contigs = (uint64_t)n_ref;
    h->names_bytes = name_at;
    h->text_off = 8;
    h->text_len = (uint64_t)l_text;
    h->body_off = at;
    return BG_OK;
}

// ---- a position -----------------------------------------------------------------------------------------------------------
// Whether an accepted record stands at byte o of s[0 .. in_bytes) (THE RULE of bg_bam_records): BG_OK and *size = 4 +
// block_size, or BG_ERR_INVALID_ARG.  Reads no byte outside s[o .. in_bytes), and none behind the record it accepts.
SAM_HD int bamr_verdict(const uint8_t* s, uint64_t in_bytes, uint64_t o, uint64_t n_ref, uint64_t* size) {
    if (o > in_bytes || in_bytes - o < BAM_FIXED) return BG_ERR_INVALID_ARG;
    const uint8_t* r = s + o;
    const uint64_t block = bai_get32(r);
    const int32_t ref = (int32_t)bai_get32(r + 4), pos = (int32_t)bai_get32(r + 8), l_seq = (int32_t)bai_get32(r + 20);
    const int32_t next_ref = (int32_t)bai_get32(r + 24), next_pos = (int32_t)bai_get32(r + 28);
    const uint32_t l_name = r[12], n_cigar = bai_get16(r + 16);
    if (l_name < 1 || l_seq < 0) return BG_ERR_INVALID_ARG;
    const uint64_t ls = (uint64_t)l_seq, need = 32 + (uint64_t)l_name + 4ull * n_cigar + (ls + 1) / 2 + ls;
    if (block < need || block + 4 > in_bytes - o) return BG_ERR_INVALID_ARG;
    if (r[BAM_FIXED + l_name - 1] != 0) return BG_ERR_INVALID_ARG;  // (inside the record: 36 + l_name <= 4 + need)
    if (ref < -1 || (ref >= 0 && (uint64_t)ref >= n_ref) || next_ref < -1 || (next_ref >= 0 && (uint64_t)next_ref >= n_ref)) return BG_ERR_INVALID_ARG;
    if (pos < -1 || next_pos < -1) return BG_ERR_INVALID_ARG;
    *size = block + 4;
    return BG_OK;
}
// slot s[o0 .. o1) of a record table: exactly one accepted record (a table may come from elsewhere).  Reads inside the slot only.
SAM_HD bool bamr_slot_ok(const uint8_t* s, uint64_t o0, uint64_t o1, uint64_t n_ref) {
    uint64_t size = 0;
    return o1 >= o0 && bamr_verdict(s, o1, o0, n_ref, &size) == BG_OK && size == o1 - o0;
}
// rounds of doubling that mark the longest chain n_pos positions can hold
inline uint32_t bamr_rounds(uint64_t n_pos) {
    uint32_t r = 0;
    while ((1ull << r) < n_pos / BAMR_MIN_RECORD + 1) r++;
    return r;
}

// ---- a read ---------------------------------------------------------------------------------------------------------------
struct bamr_fields_t {
    uint32_t l_name, flag, l_seq;
    uint64_t seq_at, qual_at;  // from the record's start
};
SAM_HD bamr_fields_t bamr_fields(const uint8_t* r) {  // r: an accepted record
    bamr_fields_t f;
    f.l_name = r[12];
    f.flag = bai_get16(r + 18);
    f.l_seq = bai_get32(r + 20);
    f.seq_at = (uint64_t)BAM_FIXED + f.l_name + 4ull * bai_get16(r + 16);
    f.qual_at = f.seq_at + ((uint64_t)f.l_seq + 1) / 2;
    return f;
}
SAM_HD bool bamr_kept(uint32_t flag, const bg_bam_reads_t& p) { return (flag & p.require) == p.require && (flag & p.exclude) == 0; }
SAM_HD bool bamr_reversed(uint32_t flag, const bg_bam_reads_t& p) { return (p.flags & BG_BAM_READS_ORIGINAL) && (flag & 0x10u); }
// qualities 0xFF stand for "*": the first byte decides, as it does for every reader
SAM_HD uint32_t bamr_qual_len(const uint8_t* r, const bamr_fields_t& f) { return f.l_seq && r[f.qual_at] == 0xFF ? 0u : f.l_seq; }

constexpr uint64_t bamr_pack8(const char* s) {
    uint64_t v = 0;
    for (int i = 7; i >= 0; i--) v = (v << 8) | (uint8_t)s[i];
    return v;
}
#define BAMR_BASES "=ACMGRSVTWYHKDBN"
#define BAMR_BASES_RC "=TGKCYSBAWRDMHVN"  // dna::complement of each (dna_complement.h; bam_read.hip asserts it): `=` stays
constexpr uint64_t BAMR_FWD_LO = bamr_pack8(BAMR_BASES), BAMR_FWD_HI = bamr_pack8(&BAMR_BASES[8]);
constexpr uint64_t BAMR_RC_LO = bamr_pack8(BAMR_BASES_RC), BAMR_RC_HI = bamr_pack8(&BAMR_BASES_RC[8]);
// the letter of a 4-bit code (rev: of its complement): a shift out of two registers, no table in memory
SAM_HD uint8_t bamr_base(uint32_t code, bool rev) {
    const uint64_t w = rev ? (code < 8 ? BAMR_RC_LO : BAMR_RC_HI) : (code < 8 ? BAMR_FWD_LO : BAMR_FWD_HI);
    return (uint8_t)(w >> (8 * (code & 7u)));
}
// byte j of a read's bases / qualities from the record's n packed bases / n quality bytes; *eq: a base `=` (which
// Record::check refuses), *hi: a quality beyond ASCII
SAM_HD uint8_t bamr_seq_byte(const uint8_t* packed, uint32_t n, uint32_t j, bool rev, uint32_t* eq) {
    const uint32_t k = rev ? n - 1 - j : j, c = (packed[k >> 1] >> ((k & 1u) ? 0 : 4)) & 15u;
    *eq |= c == 0;
    return bamr_base(c, rev);
}
SAM_HD uint8_t bamr_qual_byte(const uint8_t* q, uint32_t n, uint32_t j, bool rev, uint32_t* hi) {
    const uint8_t b = (uint8_t)(q[rev ? n - 1 - j : j] + 33);
    *hi |= b >= 0x80;
    return b;
}
// Lane `lane` of a group of G writes its share of dst[0 .. n): the bytes up to the destination's first 16-byte boundary and
// behind its last one singly, the vectors between as one 16-byte store each.  Returns the lane's eq / hi flag.  Every byte
// read lies in the record's n packed bases (SEQ) or n qualities, every byte written in dst[0 .. n).
template <bool SEQ>
SAM_HD uint32_t bamr_column_lane(const uint8_t* src, uint32_t n, bool rev, uint8_t* dst, uint32_t lane, uint32_t G) {
    uint32_t f = 0;
    const sam_copy_plan_t p = sam_copy_plan((uint32_t)((uintptr_t)dst & 15u), n);
    auto byte = [&](uint32_t j) -> uint32_t { return SEQ ? bamr_seq_byte(src, n, j, rev, &f) : bamr_qual_byte(src, n, j, rev, &f); };
    for (uint32_t i = lane; i < p.head; i += G) dst[i] = (uint8_t)byte(i);
    for (uint32_t v = lane; v < (uint32_t)p.body; v += G) {
        const uint32_t j0 = p.head + 16u * v;
        sam_v16 x;
        for (uint32_t w = 0; w < 4; w++) {
            const uint32_t j = j0 + 4u * w;
            x.w[w] = byte(j) | (byte(j + 1) << 8) | (byte(j + 2) << 16) | (byte(j + 3) << 24);
        }
        *(sam_v16*)(dst + j0) = x;
    }
    const uint32_t t = p.head + 16u * (uint32_t)p.body;
    for (uint32_t i = lane; i < p.tail; i += G) dst[t + i] = (uint8_t)byte(t + i);
    return f;
}
// the FASTQ record of the record at byte o of the stream; eq / hi: the OR of the lanes' flags
SAM_HD bg_fastq_record_t bamr_read_record(const uint8_t* r, uint64_t o, const bamr_fields_t& f, uint32_t qual_len, uint64_t seq_off,
                                          uint64_t qual_off, uint32_t eq, uint32_t hi) {
    bg_fastq_record_t x = {};
    x.id_off = o + BAM_FIXED;
    x.id_len = f.l_name - 1;
    if (x.id_len == 1 && r[BAM_FIXED] == '*') x.id_len = 0;
    x.desc_off = x.id_off + x.id_len;
    x.seq_off = seq_off;
    x.qual_off = qual_off;
    x.seq_len = f.l_seq;
    x.qual_len = qual_len;
    x.check = x.id_len == 0 ? BG_FQCHECK_EMPTY_ID : eq ? BG_FQCHECK_INVALID_SEQ : hi ? BG_FQCHECK_NONASCII_QUAL : x.seq_len != x.qual_len ? BG_FQCHECK_UNEQUAL : BG_FQCHECK_OK;
    return x;
}

// ---- a key ----------------------------------------------------------------------------------------------------------------
// r[0 .. len): an accepted record against a table with refID < n_contigs, or an empty slot
SAM_HD uint64_t bamr_key(const uint8_t* r, uint64_t len, const bg_sam_contig_t* contigs) {
    if (!len) return UINT64_MAX;
    const int32_t ref = (int32_t)bai_get32(r + 4), pos = (int32_t)bai_get32(r + 8);
    return ref >= 0 && pos >= 0 ? contigs[ref].start + (uint64_t)pos : UINT64_MAX;
}

#endif
