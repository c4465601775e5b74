// The bodies behind the BAM record writer (bam_emit.hip) and the BGZF framing (bgzf.hip) as __host__ __device__ functions
// (the rules are in include/biogpu.h), so that the length pass and the writer share ONE definition of a field's size, and so
// that tests/bam_host_bodies.cpp can run them on the CPU under AddressSanitizer.
//   * the record:   bam_reg2bin (SAM v1.6 section 5.3), bam_base_code (4 bits a base), bam_int_type / bam_int_size /
//                   bam_put_int (an integer tag in the smallest type that holds it), bam_put32 / bam_put16 (little-endian
//                   fields at any address)
//   * the checksum: CRC-32 (reflected, polynomial 0xEDB88320) as GF(2) polynomial arithmetic on the 32-bit register.
//                   raw(M) is the register after M from a register of 0 with no final inversion; it is linear, so
//                     raw(A || B) = raw(A) * x^(8 |B|) + raw(B)      and      raw(0^k || M) = raw(M),
//                   and crc32(M) = raw(M) + crc32(0^|M|), where crc32(0^n) = 0xFFFFFFFF * x^(8 n) + 0xFFFFFFFF.
//                   bam_crc_mul multiplies two registers mod P, bam_crc_xpow8(n) is x^(8 n), bam_crc_word / bam_crc_byte
//                   advance a register by four bytes / one byte from the slicing-by-4 table (bam_crc_table_entry fills it).
//   * a payload:    bgzf_lane: lane `lane` of BGZF_LANES copies its destination-aligned vectors of a payload (the plan and
//                   the vectors are sam_rule.h's) and returns the raw CRC of those bytes already multiplied by x^(8 t), t
//                   the number of payload bytes behind them; the XOR over all lanes is raw(payload).
#ifndef BG_BAM_RULE_H
#define BG_BAM_RULE_H
#include "sam_rule.h"

// ---- the record ---------------------------------------------------------------------------------------------------------
#define BAM_FIXED 36u            // bytes of a record in front of read_name, block_size included
#define BAM_MAX_QNAME 254u       // l_read_name counts the NUL and is one byte
#define BAM_MAX_REF 2147483647u  // l_ref, pos and next_pos are int32
#define BAM_MAX_CIGAR 65535u     // n_cigar_op is uint16: more operations go into a CG:B:I tag
#define BAM_UNMAPPED_BIN 4680u   // reg2bin(-1, 0)

// the bin of the 0-based half-open interval [beg, end); the arithmetic shifts make (-1, 0) bin 4680
SAM_HD uint32_t bam_reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}
// the bin field of a record at 0-based pos (-1: none) whose CIGAR consumes ref_len reference bases (0: none, or no CIGAR)
SAM_HD uint16_t bam_bin(int64_t pos, uint64_t ref_len) { return (uint16_t)bam_reg2bin(pos, pos + (int64_t)(ref_len ? ref_len : 1)); }

// the code of a base: its place in "=ACMGRSVTWYHKDBN", lower case as upper case, every other byte 15
SAM_HD uint32_t bam_base_code(uint8_t c) {
    if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
    switch (c) {
        case '=': return 0;
        case 'A': return 1;
        case 'C': return 2;
        case 'M': return 3;
        case 'G': return 4;
        case 'R': return 5;
        case 'S': return 6;
        case 'V': return 7;
        case 'T': return 8;
        case 'W': return 9;
        case 'Y': return 10;
        case 'H': return 11;
        case 'K': return 12;
        case 'D': return 13;
        case 'B': return 14;
        default: return 15;
    }
}

SAM_HD void bam_put16(uint8_t* d, uint32_t v) {
    d[0] = (uint8_t)v;
    d[1] = (uint8_t)(v >> 8);
}
SAM_HD void bam_put32(uint8_t* d, uint32_t v) {
    d[0] = (uint8_t)v;
    d[1] = (uint8_t)(v >> 8);
    d[2] = (uint8_t)(v >> 16);
    d[3] = (uint8_t)(v >> 24);
}
// an integer tag value: the smallest of c s i for a negative one, of C S I otherwise
SAM_HD char bam_int_type(int64_t v) {
    if (v < 0) return v >= -128 ? 'c' : v >= -32768 ? 's' : 'i';
    return v <= 255 ? 'C' : v <= 65535 ? 'S' : 'I';
}
SAM_HD uint32_t bam_int_size(int64_t v) {
    const char t = bam_int_type(v);
    return t == 'c' || t == 'C' ? 1u : t == 's' || t == 'S' ? 2u : 4u;
}
// "XY" type value at d; returns the bytes written: 3 + bam_int_size(v)
SAM_HD uint32_t bam_put_int(uint8_t* d, char c0, char c1, int64_t v) {
    const uint32_t n = bam_int_size(v);
    d[0] = (uint8_t)c0;
    d[1] = (uint8_t)c1;
    d[2] = (uint8_t)bam_int_type(v);
    for (uint32_t i = 0; i < n; i++) d[3 + i] = (uint8_t)((uint64_t)v >> (8 * i));
    return 3 + n;
}
// a CIGAR operation: len << 4 | op, op the place of the letter in "MIDNSHP=X"
enum { BAM_CIGAR_I = 1, BAM_CIGAR_D = 2, BAM_CIGAR_N = 3, BAM_CIGAR_S = 4, BAM_CIGAR_EQ = 7, BAM_CIGAR_X = 8 };
SAM_HD uint32_t bam_cigar_word(uint32_t len, uint32_t op) { return (len << 4) | op; }

// ---- CRC-32 ---------------------------------------------------------------------------------------------------------------
#define BAM_CRC_POLY 0xEDB88320u
// a * b mod P; bit 31 of a register is x^0
SAM_HD uint32_t bam_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        p ^= (a >> i) & 1u ? b : 0u;
        b = (b >> 1) ^ (b & 1u ? BAM_CRC_POLY : 0u);
    }
    return p;
}
// x^(8 * 2^j) mod P (each the square of the one before; tests/bam_host_bodies.cpp squares them again)
SAM_HD uint32_t bam_crc_pow2(uint32_t j) {
    switch (j) {
        case 0: return 0x00800000u;
        case 1: return 0x00008000u;
        case 2: return 0xedb88320u;
        case 3: return 0xb1e6b092u;
        case 4: return 0xa06a2517u;
        case 5: return 0xed627daeu;
        case 6: return 0x88d14467u;
        case 7: return 0xd7bbfe6au;
        case 8: return 0xec447f11u;
        case 9: return 0x8e7ea170u;
        case 10: return 0x6427800eu;
        case 11: return 0x4d47bae0u;
        case 12: return 0x09fe548fu;
        case 13: return 0x83852d0fu;
        case 14: return 0x30362f1au;
        case 15: return 0x7b5a9cc3u;
        default: return 0x31fec169u;  // j == 16
    }
}
// x^(8 n) mod P for n < 2^17
SAM_HD uint32_t bam_crc_xpow8(uint32_t n) {
    uint32_t p = 0x80000000u;
    for (uint32_t j = 0; n; j++, n >>= 1)
        if (n & 1u) p = bam_crc_mul(p, bam_crc_pow2(j));
    return p;
}
// entry t (0 .. 1023) of the slicing-by-4 table, given the entries below 256 (the byte table) for t >= 256
SAM_HD uint32_t bam_crc_byte_entry(uint32_t t) {
    uint32_t c = t;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (c & 1u ? BAM_CRC_POLY : 0u);
    return c;
}
SAM_HD void bam_crc_slices(uint32_t* T, uint32_t t) {  // T[t] is set: fills T[256 + t], T[512 + t], T[768 + t]
    uint32_t c = T[t];
    for (int s = 1; s < 4; s++) {
        c = (c >> 8) ^ T[c & 0xFFu];
        T[256 * s + t] = c;
    }
}
SAM_HD uint32_t bam_crc_byte(const uint32_t* T, uint32_t c, uint8_t b) { return (c >> 8) ^ T[(c ^ b) & 0xFFu]; }
SAM_HD uint32_t bam_crc_word(const uint32_t* T, uint32_t c, uint32_t w) {  // w: the next four bytes, little-endian
    c ^= w;
    return T[768 + (c & 0xFFu)] ^ T[512 + ((c >> 8) & 0xFFu)] ^ T[256 + ((c >> 16) & 0xFFu)] ^ T[c >> 24];
}
// crc32 of an n-byte message whose raw register is `raw`
SAM_HD uint32_t bam_crc_finish(uint32_t raw, uint32_t n) { return raw ^ bam_crc_mul(0xFFFFFFFFu, bam_crc_xpow8(n)) ^ 0xFFFFFFFFu; }

// ---- a BGZF block ---------------------------------------------------------------------------------------------------------
#define BGZF_PAYLOAD 65280u  // 0xff00: the bytes of a full block's payload
#define BGZF_HEAD 23u        // the 18-byte gzip header with its BC subfield, 01, LEN, NLEN
#define BGZF_EXTRA 31u       // ... and CRC-32, ISIZE
#define BGZF_EOF_BYTES 28u
#define BGZF_LANES 256u      // lanes of the workgroup that takes a payload
#define BGZF_LANE_VECS 16u   // 16-byte vectors of a lane at most: 256 * 16 of them hold a full payload's body

// byte i (< BGZF_HEAD) in front of a payload of len bytes
SAM_HD uint8_t bgzf_head_byte(uint32_t i, uint32_t len) {
    const uint32_t bsize1 = len + BGZF_EXTRA - 1;
    switch (i) {
        case 0: return 0x1f;
        case 1: return 0x8b;
        case 2: return 8;
        case 3: return 4;
        case 9: return 0xff;
        case 10: return 6;
        case 12: return 'B';
        case 13: return 'C';
        case 14: return 2;
        case 16: return (uint8_t)bsize1;
        case 17: return (uint8_t)(bsize1 >> 8);
        case 18: return 1;
        case 19: return (uint8_t)len;
        case 20: return (uint8_t)(len >> 8);
        case 21: return (uint8_t)~len;
        case 22: return (uint8_t)(~len >> 8);
        default: return 0;
    }
}
// byte i (< BGZF_EOF_BYTES) of the end-of-file block: an empty payload in a fixed (compressed) deflate block, as htslib writes it
SAM_HD uint8_t bgzf_eof_byte(uint32_t i) { return i == 16 ? 0x1b : i == 18 ? 3 : i < 16 ? bgzf_head_byte(i, 0) : 0; }

// K[256 k + b] = (the register whose byte k is b) * x^(8 * 4096): with these acc * x^(8 * 4096) is four lookups (bam_crc_far)
SAM_HD uint32_t bam_crc_far_entry(uint32_t t) { return bam_crc_mul((t & 0xFFu) << (8 * (t >> 8)), bam_crc_pow2(12)); }
SAM_HD uint32_t bam_crc_far(const uint32_t* K, uint32_t c) {
    return K[c & 0xFFu] ^ K[256 + ((c >> 8) & 0xFFu)] ^ K[512 + ((c >> 16) & 0xFFu)] ^ K[768 + (c >> 24)];
}

// Lane `lane` of BGZF_LANES on the payload src[0 .. len), len <= BGZF_PAYLOAD, that goes to dst.  The plan cuts the payload at
// the destination's 16-byte boundaries; lane l takes the body vectors l, l + 256, ... (at most BGZF_LANE_VECS: neighbouring
// lanes load and store neighbouring vectors), lane 0 the head in front of its first vector, the last lane the tail.  Copies
// them and returns their raw CRC times x^(8 t), t the payload bytes behind the lane's last vector: each vector's own
// register (from 0; lane 0's first from the head's) joins the lane's by acc = acc * x^(8 * 4096) + r, since the lane's
// vectors lie 4096 bytes apart.  T: the slicing table, K: bam_crc_far's.  Every byte read lies in src[0 .. len), every byte
// written in dst[0 .. len).
SAM_HD uint32_t bgzf_lane(const uint32_t* T, const uint32_t* K, const uint8_t* src, uint8_t* dst, uint32_t len, uint32_t lane) {
    const sam_copy_plan_t p = sam_copy_plan((uint32_t)((uintptr_t)dst & 15u), len);
    const uint32_t body = (uint32_t)p.body;
    uint32_t first = 0;  // the register the lane's first vector starts from
    if (lane == 0)
        for (uint32_t i = 0; i < p.head; i++) {
            dst[i] = src[i];
            first = bam_crc_byte(T, first, src[i]);
        }
    sam_v16 x[BGZF_LANE_VECS];
#pragma unroll
    for (uint32_t j = 0; j < BGZF_LANE_VECS; j++) {  // all loads first: nothing below waits on a store
        const uint32_t v = lane + BGZF_LANES * j;
        if (v < body) x[j] = sam_copy_vec(src + p.head + 16u * v, src, src + len);
    }
    uint32_t acc = first, behind = len - p.head;
#pragma unroll
    for (uint32_t j = 0; j < BGZF_LANE_VECS; j++) {
        const uint32_t v = lane + BGZF_LANES * j;
        if (v >= body) continue;
        *(sam_v16*)(dst + p.head + 16u * v) = x[j];
        uint32_t r = j ? 0u : first;
        for (int i = 0; i < 4; i++) r = bam_crc_word(T, r, x[j].w[i]);
        acc = j ? bam_crc_far(K, acc) ^ r : r;
        behind = len - p.head - 16u * (v + 1);
    }
    uint32_t c = acc ? bam_crc_mul(acc, bam_crc_xpow8(behind)) : 0u;
    if (lane == BGZF_LANES - 1) {  // nothing lies behind the tail
        const uint32_t t = p.head + 16u * body;
        uint32_t r = 0;
        for (uint32_t i = 0; i < p.tail; i++) {
            dst[t + i] = src[t + i];
            r = bam_crc_byte(T, r, src[t + i]);
        }
        c ^= r;
    }
    return c;
}
// bgzf_lane without the copy (a payload that leaves compressed still wants its CRC-32): the same shares, cut at the SOURCE's
// 16-byte boundaries, so that every vector is one aligned load.  Every byte read lies in src[0 .. len).
SAM_HD uint32_t bgzf_lane_crc(const uint32_t* T, const uint32_t* K, const uint8_t* src, uint32_t len, uint32_t lane) {
    const sam_copy_plan_t p = sam_copy_plan((uint32_t)((uintptr_t)src & 15u), len);
    const uint32_t body = (uint32_t)p.body;
    uint32_t first = 0;
    if (lane == 0)
        for (uint32_t i = 0; i < p.head; i++) first = bam_crc_byte(T, first, src[i]);
    uint32_t acc = first, behind = len - p.head;
    for (uint32_t j = 0; j < BGZF_LANE_VECS; j++) {
        const uint32_t v = lane + BGZF_LANES * j;
        if (v >= body) break;
        const sam_v16 x = *(const sam_v16*)(src + p.head + 16u * v);
        uint32_t r = j ? 0u : first;
        for (int i = 0; i < 4; i++) r = bam_crc_word(T, r, x.w[i]);
        acc = j ? bam_crc_far(K, acc) ^ r : r;
        behind = len - p.head - 16u * (v + 1);
    }
    uint32_t c = acc ? bam_crc_mul(acc, bam_crc_xpow8(behind)) : 0u;
    if (lane == BGZF_LANES - 1) {
        const uint32_t t = p.head + 16u * body;
        uint32_t r = 0;
        for (uint32_t i = 0; i < p.tail; i++) r = bam_crc_byte(T, r, src[t + i]);
        c ^= r;
    }
    return c;
}

#endif
