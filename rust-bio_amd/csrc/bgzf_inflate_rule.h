// The bodies behind bg_bgzf_blocks and bg_bgzf_inflate (bgzf_inflate.hip; the rules are in include/biogpu.h) as __host__
// __device__ functions, so that tests/bgzf_inflate_host_bodies.cpp can run them on the CPU under AddressSanitizer and the GPU
// must give the CPU's statuses.
//   * a member:   bgzf_member_verdict: whether a complete accepted member starts at a position, and if not, which error it is.
//                 The block table's kernels flag candidates with it and name the error at the chain's end with it.
//   * a block:    inf_block inflates one member into its output range as the 64 lanes of one wavefront do.  It is written
//                 ONCE: where the kernel has "every lane, then a barrier" the host runs lanes 0 .. 63 in turn (INF_EACH ..
//                 INF_JOIN); everything outside such a section is the same in every lane (the bit position, the state, the
//                 tokens), so the host runs it once and the compiler may keep it in scalar registers.
//     bits        inf_bits_t: a 64-bit hold refilled four bytes or a byte at a time; bytes behind the stream read as 0 and
//                 are counted, so "bits wanted beyond the stream" is one comparison (inf_over) after the bits are taken.
//     code sets   inf_set_scan (one lane): counts per length, zlib's legality rule, first codes, the symbols in code order;
//                 inf_set_fill (all lanes): entry i of the first-level table by canonical search over the lengths up to the
//                 root — every lane the same number of steps, no entry written twice.  An entry is symbol << 4 | length, 0
//                 where no code of at most root bits matches.  The second level (inf_decode) is the same search continued over
//                 the lengths root + 1 .. 15 on the bit-reversed hold: at most five steps, and codes that long are rare.
//     tokens      a queue of INF_QUEUE (position, length << 16 | distance or literal byte).  inf_drain: the literals a lane
//                 each, a barrier, then the matches in order, each copied by all lanes with out[p + i] = out[p - d + i mod d].
//                 Every source byte precedes p.  A match whose source reaches into a match copied since the last barrier
//                 waits for one more (`dirty`); most matches reach further back and do not.
//     a token that would end behind the output range is counted and not executed, so decoding goes on to the stream's end and
//     the first error in decode order decides the status; size and CRC come last.
//     CRC-32      bam_rule.h's arithmetic: lane l takes bytes [l c, (l + 1) c) of the payload, c a multiple of 4, from a register
//                 of 0 and multiplies by x^(8 * bytes behind); the XOR of the shares is the raw register.
//   Safety: every read of the member goes through inf_bits_t (bounded by n) or the stored copy (bounded by LEN after the
//   check against n); every store goes through a token with position + length <= isize or the stored copy under the same
//   check; the symbol loop takes at least one bit a turn and ends once inf_over holds.
#ifndef BG_BGZF_INFLATE_RULE_H
#define BG_BGZF_INFLATE_RULE_H
#include "bam_rule.h"

#define BGZF_MIN_MEMBER 28u   // header 18, an empty deflate stream 2, CRC-32, ISIZE
#define BGZF_MAX_ISIZE 65536u
#define BGZF_HEADER 18u
#define INF_LANES 64u
#define INF_LROOT 10u  // bits of the first-level table: literal/length
#define INF_DROOT 8u   // ... distance
#define INF_CROOT 7u   // ... the code-length alphabet (its longest code: no second level)
#define INF_NLIT 288u
#define INF_NDIST 32u
#define INF_NCODE 19u
#define INF_QUEUE 64u
#define INF_NONE 0xFFFFFFFFu
enum { INF_SET_CODES = 0, INF_SET_LIT = 1, INF_SET_DIST = 2 };

#ifdef __HIP_DEVICE_COMPILE__
#define INF_EACH(lane) { const uint32_t lane = threadIdx.x;
#define INF_JOIN __syncthreads(); }
#define INF_END }
#define INF_SYNC __syncthreads()
#define INF_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define INF_EACH(lane) for (uint32_t lane = 0; lane < INF_LANES; lane++) {
#define INF_JOIN }
#define INF_END }
#define INF_SYNC (void)0
#define INF_UNI(x) ((uint32_t)(x))
#endif

// ---- a member -----------------------------------------------------------------------------------------------------------
SAM_HD uint32_t bgzf_le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
SAM_HD uint32_t bgzf_le32(const uint8_t* p) { return bgzf_le16(p) | (bgzf_le16(p + 2) << 16); }
// BG_OK if a complete accepted member starts at p (< or = in_bytes): *size = BSIZE + 1, *isize = its ISIZE; otherwise the
// error of a chain that arrives at p, decided in this order: no gzip magic (1f 8b) or fewer than 12 bytes left: INVALID_ARG;
// CM != 8, FLG != 4 or XLEN != 6: UNSUPPORTED; fewer than 18 bytes left: INVALID_ARG; a subfield other than 42 43 02 00:
// UNSUPPORTED; BSIZE + 1 < 28, a member running past in_bytes, ISIZE > 65 536: INVALID_ARG.
SAM_HD int bgzf_member_verdict(const uint8_t* in, uint64_t in_bytes, uint64_t p, uint32_t* size, uint32_t* isize) {
    const uint64_t left = in_bytes - p;
    if (left < 2 || in[p] != 0x1f || in[p + 1] != 0x8b || left < 12) return BG_ERR_INVALID_ARG;
    if (in[p + 2] != 8 || in[p + 3] != 4 || in[p + 10] != 6 || in[p + 11] != 0) return BG_ERR_UNSUPPORTED;
    if (left < BGZF_HEADER) return BG_ERR_INVALID_ARG;
    if (in[p + 12] != 'B' || in[p + 13] != 'C' || in[p + 14] != 2 || in[p + 15] != 0) return BG_ERR_UNSUPPORTED;
    const uint32_t n = bgzf_le16(in + p + 16) + 1;
    if (n < BGZF_MIN_MEMBER || n > left) return BG_ERR_INVALID_ARG;
    const uint32_t sz = bgzf_le32(in + p + n - 4);
    if (sz > BGZF_MAX_ISIZE) return BG_ERR_INVALID_ARG;
    *size = n;
    *isize = sz;
    return BG_OK;
}

// ---- bits ---------------------------------------------------------------------------------------------------------------
struct inf_bits_t {
    const uint8_t* p;  // the deflate stream
    uint32_t n, at;    // its bytes; the next byte to load (beyond n: zeros)
    uint64_t hold;
    uint32_t have;
};
// at least 57 bits in hold
SAM_HD void inf_refill(inf_bits_t& b) {
    if (b.have <= 32 && b.at + 4 <= b.n) {
        const uint8_t* q = b.p + b.at;
        const uint32_t w = INF_UNI((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24));
        b.hold |= (uint64_t)w << b.have;
        b.at += 4;
        b.have += 32;
    }
    _Pragma("nounroll") while (b.have <= 56) {
        const uint32_t v = b.at < b.n ? INF_UNI(b.p[b.at]) : 0u;
        b.hold |= (uint64_t)v << b.have;
        b.at++;
        b.have += 8;
    }
}
SAM_HD uint32_t inf_take(inf_bits_t& b, uint32_t k) {  // k <= 32 <= have
    const uint32_t v = (uint32_t)(b.hold & ((1ull << k) - 1));
    b.hold >>= k;
    b.have -= k;
    return v;
}
SAM_HD uint32_t inf_bitpos(const inf_bits_t& b) { return 8 * b.at - b.have; }
SAM_HD bool inf_over(const inf_bits_t& b) { return inf_bitpos(b) > 8 * b.n; }  // bits were taken from behind the stream

// ---- code sets ----------------------------------------------------------------------------------------------------------
struct inf_set_t {
    const uint8_t* lens;
    uint32_t n, root;
    uint16_t *tab, *sorted;      // [1 << root]; [n] the symbols in code order
    uint16_t *cnt, *first, *offs;  // [16] each, by code length: codes, the first code, where its symbols start in sorted
};
// One lane: 1 if the set is legal (zlib's rule: never over-subscribed; incomplete only as a literal/length or distance set
// whose longest code has 1 bit; no code at all only as a distance set), and then cnt, first, offs, sorted are set.
SAM_HD uint32_t inf_set_scan(const inf_set_t& s, uint32_t kind) {
    for (uint32_t l = 0; l < 16; l++) s.cnt[l] = 0;
    _Pragma("nounroll") for (uint32_t i = 0; i < s.n; i++) s.cnt[s.lens[i]]++;
    uint32_t max = 15;
    while (max && !s.cnt[max]) max--;
    if (max == 0) {
        for (uint32_t l = 0; l < 16; l++) s.first[l] = s.offs[l] = 0;
        return kind == INF_SET_DIST;
    }
    int32_t left = 1;
    for (uint32_t l = 1; l < 16; l++) {
        left = 2 * left - (int32_t)s.cnt[l];
        if (left < 0) return 0;
    }
    if (left > 0 && (kind == INF_SET_CODES || max != 1)) return 0;
    uint32_t code = 0, off = 0, shorter = 0;  // shorter: the codes one bit shorter
    s.first[0] = s.offs[0] = 0;
    for (uint32_t l = 1; l < 16; l++) {
        code = (code + shorter) << 1;
        shorter = s.cnt[l];
        s.first[l] = (uint16_t)code;
        s.offs[l] = (uint16_t)off;
        off += shorter;
        s.cnt[l] = 0;
    }
    _Pragma("nounroll") for (uint32_t i = 0; i < s.n; i++) {
        const uint32_t l = s.lens[i];
        if (l) s.sorted[s.offs[l] + s.cnt[l]++] = (uint16_t)i;  // cnt ends as the counts again
    }
    return 1;
}
// symbol << 4 | l if the l-bit code `code` (first bit highest) is assigned, else 0
SAM_HD uint32_t inf_set_code(const inf_set_t& s, uint32_t code, uint32_t l) {
    const uint32_t f = s.first[l];
    return code >= f && code - f < s.cnt[l] ? ((uint32_t)s.sorted[s.offs[l] + code - f] << 4) | l : 0u;
}
SAM_HD void inf_set_fill(const inf_set_t& s, uint32_t lane) {
    for (uint32_t idx = lane; idx < (1u << s.root); idx += INF_LANES) {
        uint32_t e = 0, code = 0;
        _Pragma("nounroll") for (uint32_t l = 1; l <= s.root && !e; l++) {
            code = (code << 1) | ((idx >> (l - 1)) & 1u);
            e = inf_set_code(s, code, l);
        }
        s.tab[idx] = (uint16_t)e;
    }
}
SAM_HD uint32_t inf_rev16(uint32_t x) {
    x = ((x & 0x5555u) << 1) | ((x >> 1) & 0x5555u);
    x = ((x & 0x3333u) << 2) | ((x >> 2) & 0x3333u);
    x = ((x & 0x0F0Fu) << 4) | ((x >> 4) & 0x0F0Fu);
    return ((x & 0x00FFu) << 8) | ((x >> 8) & 0x00FFu);
}
// the symbol at the front of `bits` (the next 16 bits of the stream): symbol << 4 | length, 0 if no code matches
SAM_HD uint32_t inf_decode(const inf_set_t& s, uint32_t bits) {
    uint32_t e = INF_UNI(s.tab[bits & ((1u << s.root) - 1)]);
    if (e || s.root == INF_CROOT) return e;  // (the code-length alphabet has no code beyond its root: a miss there is final)
    const uint32_t r = inf_rev16(bits & 0xFFFFu);
    _Pragma("nounroll") for (uint32_t l = s.root + 1; l < 16 && !e; l++) e = INF_UNI(inf_set_code(s, r >> (16 - l), l));
    return e;
}

// ---- the working set of a block (LDS in the kernel, heap arrays of exactly these sizes in the test program) ---------------
struct inf_ws_t {
    uint16_t* lit;     // [1 << INF_LROOT]
    uint16_t* dst;     // [1 << INF_DROOT]; the code-length alphabet's table while the lengths are read
    uint16_t* sorted;  // [INF_NLIT + INF_NDIST]: literal/length symbols, then distance symbols (or the code-length alphabet's)
    uint16_t* meta;    // [2 * 48]: cnt, first, offs of the literal/length set, then of the distance (or code-length) set
    uint8_t* lens;     // [INF_NLIT + INF_NDIST]
    uint8_t* clens;    // [INF_NCODE]
    uint32_t* q;       // [2 * INF_QUEUE]
    uint32_t* T;       // [1024] the CRC's slicing table
    uint32_t* part;    // [INF_LANES] the lanes' CRC shares
    uint32_t* word;    // [1] one lane's verdict for all
};
SAM_HD inf_set_t inf_set(const inf_ws_t& w, uint32_t kind, uint32_t nlit, uint32_t ndist) {
    if (kind == INF_SET_LIT) return {w.lens, nlit, INF_LROOT, w.lit, w.sorted, w.meta, w.meta + 16, w.meta + 32};
    if (kind == INF_SET_DIST) return {w.lens + nlit, ndist, INF_DROOT, w.dst, w.sorted + INF_NLIT, w.meta + 48, w.meta + 64, w.meta + 80};
    return {w.clens, INF_NCODE, INF_CROOT, w.dst, w.sorted + INF_NLIT, w.meta + 48, w.meta + 64, w.meta + 80};
}
SAM_HD uint32_t inf_build(const inf_ws_t& w, const inf_set_t& s, uint32_t kind) {
    INF_EACH(lane)
    if (lane == 0) *w.word = inf_set_scan(s, kind);
    INF_JOIN
    if (!INF_UNI(*w.word)) return 0;
    INF_EACH(lane)
    inf_set_fill(s, lane);
    INF_JOIN
    return 1;
}
SAM_HD void inf_fixed_lens(const inf_ws_t& w, uint32_t lane) {
    for (uint32_t i = lane; i < INF_NLIT + INF_NDIST; i += INF_LANES) w.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < INF_NLIT ? 8 : 5;
}
SAM_HD uint32_t inf_code_order(uint32_t i) {  // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1u) ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1);
}

// ---- tokens -------------------------------------------------------------------------------------------------------------
SAM_HD void inf_drain_lits(const inf_ws_t& w, uint8_t* out, uint32_t nq, uint32_t lane) {
    if (lane >= nq) return;
    const uint32_t t = w.q[2 * lane + 1];
    if (!(t >> 16)) out[w.q[2 * lane]] = (uint8_t)t;
}
SAM_HD void inf_copy_match(uint8_t* out, uint32_t p, uint32_t len, uint32_t d, uint32_t lane) {
    for (uint32_t i = lane; i < len; i += INF_LANES) out[p + i] = out[p - d + (d >= len ? i : i % d)];
}
// all tokens of the queue; dirty: the position of the first match copied since the last barrier
SAM_HD void inf_drain(const inf_ws_t& w, uint8_t* out, uint32_t nq, uint32_t& dirty) {
    if (!nq) return;
#ifdef INF_KO_COPIES  // knock-out build (tools/exp/ko_build.sh; timing only): tokens are decoded and dropped
    return;
#endif
    INF_EACH(lane)
    inf_drain_lits(w, out, nq, lane);
    INF_JOIN
    dirty = INF_NONE;
    _Pragma("nounroll") for (uint32_t j = 0; j < nq; j++) {
        const uint32_t t = INF_UNI(w.q[2 * j + 1]), len = t >> 16, d = t & 0xFFFFu;
        if (!len) continue;
        const uint32_t p = INF_UNI(w.q[2 * j]);
        if (dirty != INF_NONE && p - d + (len < d ? len : d) > dirty) {
            INF_SYNC;
            dirty = INF_NONE;
        }
        INF_EACH(lane)
        inf_copy_match(out, p, len, d, lane);
        INF_END  // (no barrier behind a match)
        if (dirty == INF_NONE) dirty = p;
    }
}

// ---- CRC-32 -------------------------------------------------------------------------------------------------------------
SAM_HD uint32_t inf_crc_share(const uint32_t* T, const uint8_t* out, uint32_t len, uint32_t lane) {
    const uint32_t chunk = ((len + INF_LANES - 1) / INF_LANES + 3) & ~3u;
    const uint32_t a = lane * chunk < len ? lane * chunk : len, e = a + chunk < len ? a + chunk : len;
    uint32_t r = 0, i = a;
    for (; i + 4 <= e; i += 4) r = bam_crc_word(T, r, bgzf_le32(out + i));
    for (; i < e; i++) r = bam_crc_byte(T, r, out[i]);
    return r ? bam_crc_mul(r, bam_crc_xpow8(len - e)) : 0u;
}

// ---- a block ------------------------------------------------------------------------------------------------------------
// member[0 .. size), size >= 28, into out[0 .. isize), isize <= 65 536.  Returns the block's BG_INFLATE_* status.
SAM_HD uint32_t inf_block(const inf_ws_t& w, const uint8_t* member, uint32_t size, uint8_t* out, uint32_t isize) {
    inf_bits_t b = {member + BGZF_HEADER, size - BGZF_HEADER - 8, 0, 0, 0};
    uint32_t produced = 0, status = BG_INFLATE_OK, dirty = INF_NONE, last = 0;
    _Pragma("nounroll") while (!last && !status) {
        inf_refill(b);
        last = inf_take(b, 1);
        const uint32_t type = inf_take(b, 2);
        if (inf_over(b)) {
            status = BG_INFLATE_TRUNCATED;
        } else if (type == 3) {
            status = BG_INFLATE_BAD_TYPE;
        } else if (type == 0) {  // stored: to the byte boundary, LEN, NLEN, the bytes
            inf_take(b, b.have & 7u);
            inf_refill(b);
            const uint32_t len = inf_take(b, 16), nlen = inf_take(b, 16);
            const uint32_t from = inf_bitpos(b) >> 3;
            if (inf_over(b)) {
                status = BG_INFLATE_TRUNCATED;
            } else if ((len ^ nlen) != 0xFFFFu) {
                status = BG_INFLATE_BAD_STORED;
            } else if (from + len > b.n) {
                status = BG_INFLATE_TRUNCATED;
            } else {
                if (produced + len <= isize) {
                    INF_EACH(lane)
                    sam_copy_line(b.p + from, out + produced, len, lane, INF_LANES, 0, UINT64_MAX, true);
                    INF_JOIN
                    dirty = INF_NONE;
                }
                produced += len;
                b.at = from + len;
                b.hold = 0;
                b.have = 0;
            }
        } else {
            uint32_t nlit = INF_NLIT, ndist = INF_NDIST;
            if (type == 1) {
                INF_EACH(lane)
                inf_fixed_lens(w, lane);
                INF_JOIN
            } else {  // the dynamic header, in zlib's order of checks
                inf_refill(b);
                nlit = inf_take(b, 5) + 257;
                ndist = inf_take(b, 5) + 1;
                const uint32_t ncode = inf_take(b, 4) + 4;
                if (inf_over(b)) status = BG_INFLATE_TRUNCATED;
                else if (nlit > 286 || ndist > 30) status = BG_INFLATE_BAD_LENGTHS;
                for (uint32_t i = 0; i < INF_NCODE; i++) w.clens[i] = 0;
                _Pragma("nounroll") for (uint32_t i = 0; i < ncode && !status; i++) {
                    inf_refill(b);
                    w.clens[inf_code_order(i)] = (uint8_t)inf_take(b, 3);
                    if (inf_over(b)) status = BG_INFLATE_TRUNCATED;
                }
                INF_SYNC;
                const inf_set_t cs = inf_set(w, INF_SET_CODES, 0, 0);
                if (!status && !inf_build(w, cs, INF_SET_CODES)) status = BG_INFLATE_BAD_LENGTHS;
                uint32_t i = 0;
                _Pragma("nounroll") while (!status && i < nlit + ndist) {
                    inf_refill(b);
                    const uint32_t e = inf_decode(cs, (uint32_t)b.hold & 0xFFFFu);
                    if (!e) {
                        status = BG_INFLATE_BAD_LENGTHS;
                        break;
                    }
                    inf_take(b, e & 15u);
                    const uint32_t sym = e >> 4;
                    uint32_t rep = 1, val = sym;
                    if (sym == 16) rep = 3 + inf_take(b, 2);
                    else if (sym == 17) rep = 3 + inf_take(b, 3), val = 0;
                    else if (sym == 18) rep = 11 + inf_take(b, 7), val = 0;
                    if (inf_over(b)) {
                        status = BG_INFLATE_TRUNCATED;
                    } else if ((sym == 16 && i == 0) || i + rep > nlit + ndist) {
                        status = BG_INFLATE_BAD_LENGTHS;
                    } else {
                        if (sym == 16) val = INF_UNI(w.lens[i - 1]);
                        for (uint32_t k = 0; k < rep; k++) w.lens[i + k] = (uint8_t)val;
                        i += rep;
                    }
                }
                INF_SYNC;
                if (!status && !INF_UNI(w.lens[256])) status = BG_INFLATE_BAD_LENGTHS;
            }
            const inf_set_t ls = inf_set(w, INF_SET_LIT, nlit, ndist), ds = inf_set(w, INF_SET_DIST, nlit, ndist);
            if (!status && !inf_build(w, ls, INF_SET_LIT)) status = BG_INFLATE_BAD_LENGTHS;
            if (!status && !inf_build(w, ds, INF_SET_DIST)) status = BG_INFLATE_BAD_LENGTHS;
            uint32_t nq = 0;
#ifdef INF_KO_DECODE  // knock-out build (timing only): the tables of a block's first deflate block, no symbol is decoded
            status = BG_INFLATE_TRUNCATED;
#endif
            _Pragma("nounroll") while (!status) {  // a symbol a turn: at least one bit
                inf_refill(b);
                uint32_t e = inf_decode(ls, (uint32_t)b.hold & 0xFFFFu);
                if (!e) {
                    status = BG_INFLATE_BAD_SYMBOL;
                    break;
                }
                inf_take(b, e & 15u);
                const uint32_t sym = e >> 4;
                if (inf_over(b)) {
                    status = BG_INFLATE_TRUNCATED;
                    break;
                }
                if (sym == 256) break;
                uint32_t len = 0, t = sym;  // a literal: length 0, the byte
                if (sym > 256) {
                    if (sym > 285) {
                        status = BG_INFLATE_BAD_SYMBOL;
                        break;
                    }
                    const uint32_t s = sym - 257, lx = s < 8 || s == 28 ? 0 : (s >> 2) - 1;
                    len = (s < 8 ? 3 + s : s == 28 ? 258 : 3 + ((4 + (s & 3u)) << lx)) + inf_take(b, lx);
                    e = inf_decode(ds, (uint32_t)b.hold & 0xFFFFu);
                    if (!e) {
                        status = inf_over(b) ? BG_INFLATE_TRUNCATED : BG_INFLATE_BAD_SYMBOL;
                        break;
                    }
                    inf_take(b, e & 15u);
                    const uint32_t c = e >> 4;
                    if (inf_over(b)) {
                        status = BG_INFLATE_TRUNCATED;
                        break;
                    }
                    if (c > 29) {
                        status = BG_INFLATE_BAD_SYMBOL;
                        break;
                    }
                    const uint32_t dx = c < 4 ? 0 : (c >> 1) - 1;
                    t = (c < 4 ? 1 + c : 1 + ((2 + (c & 1u)) << dx)) + inf_take(b, dx);
                    if (inf_over(b)) {
                        status = BG_INFLATE_TRUNCATED;
                        break;
                    }
                    if (t > produced) {
                        status = BG_INFLATE_BAD_DISTANCE;
                        break;
                    }
                }
                const uint32_t end = produced + (len ? len : 1);
                if (end <= isize) {  // a token that would leave the range is counted, not executed
                    w.q[2 * nq] = produced;
                    w.q[2 * nq + 1] = (len << 16) | t;
                    if (++nq == INF_QUEUE) {
                        inf_drain(w, out, nq, dirty);
                        nq = 0;
                    }
                }
                produced = end;
            }
            inf_drain(w, out, nq, dirty);
        }
        INF_SYNC;  // the next block rebuilds the tables
    }
    if (status) return status;
    if (((inf_bitpos(b) + 7) >> 3) < b.n) return BG_INFLATE_TRAILING;
    if (produced != isize || bgzf_le32(member + size - 4) != isize) return BG_INFLATE_SIZE;
    INF_EACH(lane)
    for (uint32_t k = 0; k < 4; k++) w.T[lane + INF_LANES * k] = bam_crc_byte_entry(lane + INF_LANES * k);
    INF_JOIN
    INF_EACH(lane)
    for (uint32_t k = 0; k < 4; k++) bam_crc_slices(w.T, lane + INF_LANES * k);
    INF_JOIN
    INF_EACH(lane)
    w.part[lane] = inf_crc_share(w.T, out, isize, lane);
    INF_JOIN
    uint32_t raw = 0;
    _Pragma("nounroll") for (uint32_t l = 0; l < INF_LANES; l++) raw ^= INF_UNI(w.part[l]);
    return bam_crc_finish(raw, isize) == bgzf_le32(member + size - 8) ? BG_INFLATE_OK : BG_INFLATE_CRC;
}

#endif
