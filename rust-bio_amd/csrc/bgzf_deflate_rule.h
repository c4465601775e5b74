// The bodies behind bg_bgzf_deflate[_dev] (bgzf_deflate.hip; the rule is in include/biogpu.h) as __host__ __device__ functions:
// one BGZF block whose payload is deflate-compressed, as the 256 lanes of a workgroup make it.  tests/bgzf_deflate_host_bodies.cpp
// runs the same functions lane by lane on the CPU under AddressSanitizer, and gives the bytes the GPU must give.
//
// A block is made in PHASES with a barrier behind each (dfl_phases(len) of them; dfl_phase(w, k, lane) is lane `lane` in phase
// k).  Inside a phase no lane reads what another lane writes in that phase, except through dfl_min / dfl_max / dfl_add / dfl_or
// (atomics on the device, plain operations on the host: all four commute), so the result does not depend on the order the
// lanes run in, and running lane 0 .. 255 one after the other on the CPU gives the GPU's bytes.
//   matches   Positions go in tiles of 256, in order.  A lane hashes the 4 bytes at its position (14 bits).  Candidates: the
//             distances 1 .. 4, the FIRST position of its own tile with the same low 10 hash bits (`near`, filled by a min and
//             emptied behind every tile), and the LAST position of the earlier tiles with the same hash (`tab`, filled by a
//             max behind every tile).  Each is extended byte by byte to at most 258 and at most the payload's end, the
//             longest wins, among equals the nearest; distance <= 32 768; a match of 3 farther than 4096 is dropped (it
//             costs more than its literals).  m[p] = length << 16 | distance, 0: a literal.
//   the parse Greedy from byte 0: next(p) = p + (length or 1).  The payload is cut into 256 segments of 255 positions.  Lane l
//             walks segment l backwards: f[p] = the first position behind the segment that the chain from p reaches.  Lane 0
//             follows f from 0 (one step a segment: at most 256) and notes where the chain enters each segment; every lane
//             then walks its segment forward from there.  Nobody walks 65 280 steps, and nothing is stored per token.
//   codes     The walk counts the 286 literal / length and the 30 distance symbols.  Every used symbol gets its place by
//             (count, symbol) (dfl_huff_rank: a lane a symbol); dfl_huff_build makes the Huffman tree from that order with two
//             queues, caps the depths at the limit and repairs the Kraft sum by moving codes down from the deepest level (the
//             rarest symbols keep the longest codes).  The code lengths are run-length coded (16, 17, 18) and those
//             symbols get a code of at most 7 bits the same way.  Exact bit counts of the three encodings come from the same
//             counts: stored wins a tie, then fixed.
//   bits      A second walk gives every lane its number of bits, lane 0 scans the 256 numbers and writes the gzip header, the
//             block header and the end-of-block code, a third walk ORs every token's bits into the block's image (LDS on the
//             device: 64 KiB, the hash table's memory), and the image goes to the block's slot 16 bytes wide.  A stored
//             block is bgzf_head_byte's header and a copy of the payload (sam_copy_line): bg_bgzf_frame's block byte for byte.
//             The CRC-32 is bgzf_lane_crc's (bam_rule.h) in every encoding.
// The loops of the functions that one lane runs alone (the trees, the header, the frame) carry _Pragma("nounroll"): they are
// serial and short, and unrolled they cost the kernel its second workgroup a CU (288 registers a lane instead of 124).
#ifndef BG_BGZF_DEFLATE_RULE_H
#define BG_BGZF_DEFLATE_RULE_H
#include "bam_rule.h"

#define DFL_HD __host__ __device__ __forceinline__

#define DFL_TILE 256u           // positions of a tile: one per lane
#define DFL_HASH_BITS 14u
#define DFL_TAB (1u << DFL_HASH_BITS)
#define DFL_NEAR 1024u          // entries of the table over a tile's own positions
#define DFL_SEG 255u            // positions of a lane's segment: 256 * 255 = 65 280
#define DFL_WINDOW 32768u
#define DFL_MIN_MATCH 3u
#define DFL_MAX_MATCH 258u
#define DFL_FAR3 4096u          // a match of 3 at a greater distance is not taken
#define DFL_NLIT 286u           // literal / length symbols
#define DFL_NDIST 30u
#define DFL_NCL 19u             // symbols of the code-length alphabet
#define DFL_D0 288u             // hist / lens / code / srt: literals and lengths at 0, distances at 288, the code-length alphabet at 320
#define DFL_C0 320u
#define DFL_SYMS 352u
#define DFL_NONE 0xFFFFFFFFu
#define DFL_IMAGE_WORDS 16384u  // a compressed block is shorter than its stored form: at most 65 311 bytes
#define DFL_WORK_LIT 1168u      // words of dfl_huff_build's work for 286 symbols: 4 * 286 + 16 (also serves the 19)
#define DFL_WORK 1312u          // ... and behind them the 30 distance symbols': 4 * 30 + 16, rounded
enum { DFL_STORED = 0, DFL_FIXED = 1, DFL_DYNAMIC = 2 };

#if defined(__HIP_DEVICE_COMPILE__)
#define dfl_min(p, v) atomicMin((p), (v))
#define dfl_max(p, v) atomicMax((p), (v))
#define dfl_add(p, v) atomicAdd((p), (v))
#define dfl_or(p, v) atomicOr((p), (v))
#else
#define dfl_min(p, v) (*(p) = *(p) < (v) ? *(p) : (v))
#define dfl_max(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define dfl_add(p, v) (*(p) += (v))
#define dfl_or(p, v) (*(p) |= (v))
#endif

// ---- the alphabets ----------------------------------------------------------------------------------------------------------
DFL_HD uint32_t dfl_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }  // v > 0
// a match length L + 3: its code (symbol 257 + code), extra bits and their value
DFL_HD uint32_t dfl_len_extra_bits(uint32_t code) { return code < 8 || code == 28 ? 0u : (code >> 2) - 1; }
DFL_HD uint32_t dfl_len_code(uint32_t L) {
    if (L < 8) return L;
    if (L == 255) return 28;
    const uint32_t eb = dfl_log2(L) - 2;
    return 4 * eb + 4 + ((L >> eb) & 3u);
}
// a distance D + 1
DFL_HD uint32_t dfl_dist_extra_bits(uint32_t code) { return code < 4 ? 0u : (code >> 1) - 1; }
DFL_HD uint32_t dfl_dist_code(uint32_t D) {
    if (D < 4) return D;
    const uint32_t eb = dfl_log2(D) - 1;
    return 2 * eb + 2 + ((D >> eb) & 1u);
}
DFL_HD uint32_t dfl_fixed_len(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }
// the order in which a dynamic block's header lists the code-length alphabet's own lengths
DFL_HD uint32_t dfl_cl_order(uint32_t i) {
    switch (i) {
        case 0: return 16;
        case 1: return 17;
        case 2: return 18;
        case 3: return 0;
        default: return i & 1u ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1);  // 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    }
}
DFL_HD uint32_t dfl_cl_extra_bits(uint32_t s) { return s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u; }

// ---- Huffman code lengths under a limit ---------------------------------------------------------------------------------------
// the place of the used symbol s among the used symbols of freq[0 .. n), by (count, symbol)
DFL_HD uint32_t dfl_huff_rank(const uint32_t* freq, uint32_t n, uint32_t s) {
    const uint32_t fs = freq[s];
    uint32_t r = 0;
    _Pragma("nounroll") for (uint32_t t = 0; t < n; t++) {
        const uint32_t ft = freq[t];
        r += ft && (ft < fs || (ft == fs && t < s)) ? 1u : 0u;
    }
    return r;
}
// srt[0 .. nu): the used symbols in that order.  Sets lens[s] of each to its code length, 1 .. limit (2^limit >= nu): the
// Kraft sum is exactly 1 for nu >= 2; one symbol gets length 1.  work: 4 nu + 16 words.
DFL_HD void dfl_huff_build(const uint32_t* freq, const uint16_t* srt, uint32_t nu, uint32_t limit, uint8_t* lens, uint32_t* work) {
    if (nu == 0) return;
    if (nu == 1) {
        lens[srt[0]] = 1;
        return;
    }
    uint32_t* wt = work;            // nodes: the leaves 0 .. nu - 1 in order, the inner nodes nu .. 2 nu - 2 as they are made
    uint32_t* par = work + 2 * nu;
    uint32_t* cnt = work + 4 * nu;  // codes of each length
    _Pragma("nounroll") for (uint32_t i = 0; i < nu; i++) wt[i] = freq[srt[i]];
    uint32_t i = 0, j = nu;
    _Pragma("nounroll") for (uint32_t k = nu; k < 2 * nu - 1; k++) {  // the two lightest of the next leaf and the next inner node; a leaf wins a tie
        const uint32_t a = i < nu && (j >= k || wt[i] <= wt[j]) ? i++ : j++;
        const uint32_t b = i < nu && (j >= k || wt[i] <= wt[j]) ? i++ : j++;
        wt[k] = wt[a] + wt[b];
        par[a] = par[b] = k;
    }
    wt[2 * nu - 2] = 0;  // from here wt is a node's depth
    _Pragma("nounroll") for (uint32_t v = 2 * nu - 2; v-- > 0;) wt[v] = wt[par[v]] + 1;
    _Pragma("nounroll") for (uint32_t d = 0; d < 16; d++) cnt[d] = 0;
    _Pragma("nounroll") for (uint32_t v = 0; v < nu; v++) cnt[wt[v] < limit ? wt[v] : limit]++;
    uint32_t total = 0;  // the Kraft sum in units of 2^-limit
    _Pragma("nounroll") for (uint32_t d = 1; d <= limit; d++) total += cnt[d] << (limit - d);
    _Pragma("nounroll") while (total > (1u << limit)) {  // one code leaves the deepest level; a code above it becomes two one level down
        cnt[limit]--;
        _Pragma("nounroll") for (uint32_t d = limit - 1; d > 0; d--)
            if (cnt[d]) {
                cnt[d]--;
                cnt[d + 1] += 2;
                break;
            }
        total--;
    }
    uint32_t at = nu;  // the most frequent symbols take the shortest codes
    _Pragma("nounroll") for (uint32_t d = 1; d <= limit; d++)
        _Pragma("nounroll") for (uint32_t c = cnt[d]; c > 0; c--) lens[srt[--at]] = (uint8_t)d;
}
// the whole of it by one caller: lens[0 .. n) from freq[0 .. n).  Returns the number of used symbols.  srt: n entries.
DFL_HD uint32_t dfl_huff_lengths(const uint32_t* freq, uint32_t n, uint32_t limit, uint8_t* lens, uint16_t* srt, uint32_t* work) {
    uint32_t nu = 0;
    _Pragma("nounroll") for (uint32_t s = 0; s < n; s++) {
        lens[s] = 0;
        if (freq[s]) {
            srt[dfl_huff_rank(freq, n, s)] = (uint16_t)s;
            nu++;
        }
    }
    dfl_huff_build(freq, srt, nu, limit, lens, work);
    return nu;
}
// canonical codes of lens[0 .. n): code[s] = the code with its first bit lowest | length << 16.  nxt: 16 words.
DFL_HD void dfl_huff_codes(const uint8_t* lens, uint32_t n, uint32_t* code, uint32_t* nxt) {
    _Pragma("nounroll") for (uint32_t d = 0; d < 16; d++) nxt[d] = 0;
    _Pragma("nounroll") for (uint32_t s = 0; s < n; s++) nxt[lens[s]]++;
    uint32_t c = 0, prev = 0;
    _Pragma("nounroll") for (uint32_t d = 1; d < 16; d++) {
        c = (c + prev) << 1;
        prev = nxt[d];
        nxt[d] = c;
    }
    _Pragma("nounroll") for (uint32_t s = 0; s < n; s++) {
        const uint32_t l = lens[s];
        uint32_t r = 0;
        if (l) {
            const uint32_t v = nxt[l]++;
            _Pragma("nounroll") for (uint32_t b = 0; b < l; b++) r |= ((v >> b) & 1u) << (l - 1 - b);
        }
        code[s] = r | (l << 16);
    }
}

// ---- a block's working set ------------------------------------------------------------------------------------------------------
struct dfl_state_t {
    uint32_t mode;      // DFL_STORED / DFL_FIXED / DFL_DYNAMIC
    uint32_t hdr_bits;  // bits of the deflate block in front of its first token
    uint32_t n_tok, hlit, hdist, hclen;
    uint32_t total;     // bytes of the finished block
    uint32_t cost[3];   // bits of the three encodings
};
// On the device src, m, f and slot are global memory (m and f a scratch slot of the block's own), everything else LDS; the
// host program gives each its own allocation of exactly these sizes.  The comments name what may share memory.
struct dfl_ws_t {
    const uint8_t* src;  // the payload
    uint32_t len;        // 1 .. BGZF_PAYLOAD
    uint32_t* m;         // [len] length << 16 | distance of the match at a position, 0: none
    uint16_t* f;         // [len] the first position behind its segment that the chain from a position reaches
    uint8_t* slot;       // [(len + 31 + 15) & ~15] the finished block; 16-byte aligned
    uint32_t* tab;       // [DFL_TAB] hash -> position + 1 of the last occurrence in the earlier tiles, 0: none
    uint32_t* near;      // [DFL_NEAR] low hash bits -> the first position of this tile, DFL_NONE: none
    uint32_t* hsh;       // [256] a lane's hash in this tile
    uint32_t* entry;     // [256] where the chain enters a segment, DFL_NONE: it does not
    uint32_t* hist;      // [DFL_SYMS] symbol counts
    uint8_t* lens;       // [DFL_SYMS] code lengths
    uint32_t* code;      // [DFL_SYMS] code | length << 16
    uint16_t* srt;       // [DFL_SYMS] used symbols by (count, symbol)            (behind the matches: may lie in tab)
    uint32_t* work;      // [DFL_WORK] dfl_huff_build's, dfl_huff_codes'            (may lie in tab)
    uint16_t* tok;       // [DFL_D0 + DFL_NDIST + 2] the run-length coded header: symbol | extra << 5   (may lie in hsh)
    uint32_t* T;         // [1024] bam_crc_word's table                             (may lie in near)
    uint32_t* K;         // [1024] bam_crc_far's
    uint32_t* crcp;      // [256] a lane's share of the raw CRC
    uint32_t* bits;      // [256] a lane's bits, then the bit in the image where they start
    uint32_t* img;       // [DFL_IMAGE_WORDS] the block as it is built, gzip header first (may be tab)
    dfl_state_t* st;
};

DFL_HD uint32_t dfl_tiles(uint32_t len) { return (len + DFL_TILE - 1) / DFL_TILE; }
enum { DFL_PHASES_HEAD = 1, DFL_PHASES_TAIL = 11 };
DFL_HD uint32_t dfl_phases(uint32_t len) { return DFL_PHASES_HEAD + 3 * dfl_tiles(len) + DFL_PHASES_TAIL; }

// v (n <= 32 bits, nothing above them) at bit `bit` of the image
DFL_HD void dfl_put(uint32_t* img, uint32_t bit, uint32_t v, uint32_t n) {
    if (!n) return;
    const uint32_t w = bit >> 5, sh = bit & 31u;
    dfl_or(img + w, v << sh);
    if (sh + n > 32) dfl_or(img + w + 1, v >> (32 - sh));
}

// ---- matches ----------------------------------------------------------------------------------------------------------------------
DFL_HD uint32_t dfl_hash(const uint8_t* s) {
    const uint32_t w = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
    return (w * 2654435761u) >> (32 - DFL_HASH_BITS);
}
DFL_HD void dfl_tile_hash(const dfl_ws_t& w, uint32_t tile, uint32_t lane) {
    const uint32_t p = tile * DFL_TILE + lane;
    uint32_t h = DFL_NONE;
    if (p + 4 <= w.len) {
        h = dfl_hash(w.src + p);
        dfl_min(w.near + (h & (DFL_NEAR - 1)), p);
    }
    w.hsh[lane] = h;
}
// the bytes at q (< p) and at p agree in this many places, at most maxl; every byte read lies in front of p + maxl
DFL_HD uint32_t dfl_extend(const uint8_t* src, uint32_t q, uint32_t p, uint32_t maxl) {
    uint32_t l = 0;
#ifndef DFL_KO_EXTEND  // knock-out build (timing only): no candidate is extended, every token is a literal
    while (l < maxl && src[q + l] == src[p + l]) l++;
#endif
    return l;
}
DFL_HD void dfl_tile_match(const dfl_ws_t& w, uint32_t tile, uint32_t lane) {
    const uint32_t p = tile * DFL_TILE + lane;
    if (p >= w.len) return;
    const uint32_t maxl = w.len - p < DFL_MAX_MATCH ? w.len - p : DFL_MAX_MATCH;
    uint32_t best = 0, dist = 0;
    if (maxl >= DFL_MIN_MATCH) {
        // nearest first: a later candidate has to be longer
        for (uint32_t d = 1; d <= 4 && d <= p && best < maxl; d++) {
            const uint32_t l = dfl_extend(w.src, p - d, p, maxl);
            if (l > best) best = l, dist = d;
        }
        const uint32_t h = w.hsh[lane];
        if (h != DFL_NONE) {
            const uint32_t q = w.near[h & (DFL_NEAR - 1)];  // in this tile: p - q < 256
            if (q < p && p - q > 4 && best < maxl) {
                const uint32_t l = dfl_extend(w.src, q, p, maxl);
                if (l > best) best = l, dist = p - q;
            }
            const uint32_t e = w.tab[h];  // in an earlier tile
            if (e && p - (e - 1) <= DFL_WINDOW && p - (e - 1) > 4 && best < maxl) {
                const uint32_t l = dfl_extend(w.src, e - 1, p, maxl);
                if (l > best) best = l, dist = p - (e - 1);
            }
        }
    }
    if (best < DFL_MIN_MATCH || (best == DFL_MIN_MATCH && dist > DFL_FAR3)) best = dist = 0;
    w.m[p] = (best << 16) | dist;
}
DFL_HD void dfl_tile_insert(const dfl_ws_t& w, uint32_t tile, uint32_t lane) {
    const uint32_t h = w.hsh[lane];
    if (h != DFL_NONE) dfl_max(w.tab + h, tile * DFL_TILE + lane + 1);
    for (uint32_t k = 0; k < DFL_NEAR / DFL_TILE; k++) w.near[lane * (DFL_NEAR / DFL_TILE) + k] = DFL_NONE;
}

// ---- the parse ------------------------------------------------------------------------------------------------------------------
DFL_HD uint32_t dfl_seg_end(uint32_t len, uint32_t lane) { return DFL_SEG * (lane + 1) < len ? DFL_SEG * (lane + 1) : len; }
DFL_HD void dfl_seg_exits(const dfl_ws_t& w, uint32_t lane) {
    w.entry[lane] = DFL_NONE;
    const uint32_t lo = DFL_SEG * lane, hi = dfl_seg_end(w.len, lane);
    for (uint32_t p = hi; p-- > lo;) {
        const uint32_t mv = w.m[p], nx = p + (mv ? mv >> 16 : 1u);
        w.f[p] = nx >= hi ? (uint16_t)nx : w.f[nx];
    }
}
DFL_HD void dfl_seg_entries(const dfl_ws_t& w) {
    for (uint32_t p = 0; p < w.len; p = w.f[p]) w.entry[p / DFL_SEG] = p;
}
// A lane's tokens.  PASS 0: counted into hist; 1: returns their bits under `code`; 2: written into the image from bits[lane].
template <int PASS>
DFL_HD uint32_t dfl_walk(const dfl_ws_t& w, uint32_t lane) {
    uint32_t p = w.entry[lane], n = 0;
    if (p == DFL_NONE) return 0;
    const uint32_t hi = dfl_seg_end(w.len, lane);
    uint32_t bit = PASS == 2 ? w.bits[lane] : 0;
    while (p < hi) {
        const uint32_t mv = w.m[p];
        if (mv) {
            const uint32_t L = (mv >> 16) - 3, D = (mv & 0xFFFFu) - 1;
            const uint32_t lc = dfl_len_code(L), dc = dfl_dist_code(D);
            const uint32_t leb = dfl_len_extra_bits(lc), deb = dfl_dist_extra_bits(dc);
            if (PASS == 0) {
                dfl_add(w.hist + 257 + lc, 1u);
                dfl_add(w.hist + DFL_D0 + dc, 1u);
            } else {
                const uint32_t c1 = w.code[257 + lc], c2 = w.code[DFL_D0 + dc];
                const uint32_t n1 = (c1 >> 16) + leb, n2 = (c2 >> 16) + deb;
                if (PASS == 2) {  // at most 15 + 5 and 15 + 13 bits
                    dfl_put(w.img, bit, (c1 & 0xFFFFu) | ((L & ((1u << leb) - 1)) << (c1 >> 16)), n1);
                    dfl_put(w.img, bit + n1, (c2 & 0xFFFFu) | ((D & ((1u << deb) - 1)) << (c2 >> 16)), n2);
                    bit += n1 + n2;
                }
                n += n1 + n2;
            }
            p += mv >> 16;
        } else {
            const uint32_t s = w.src[p];
            if (PASS == 0) dfl_add(w.hist + s, 1u);
            else {
                const uint32_t c = w.code[s];
                if (PASS == 2) {
                    dfl_put(w.img, bit, c & 0xFFFFu, c >> 16);
                    bit += c >> 16;
                }
                n += c >> 16;
            }
            p++;
        }
    }
    return n;
}

// ---- codes ----------------------------------------------------------------------------------------------------------------------
// One lane: the header of a dynamic block from lens, the cost of the three encodings, the choice, and the chosen codes.
DFL_HD void dfl_choose(const dfl_ws_t& w) {
    dfl_state_t& st = *w.st;
    uint8_t* lens = w.lens;
    uint32_t hlit = DFL_NLIT, hdist = DFL_NDIST;
    _Pragma("nounroll") while (hlit > 257 && !lens[hlit - 1]) hlit--;
    _Pragma("nounroll") while (hdist > 1 && !lens[DFL_D0 + hdist - 1]) hdist--;
    // the hlit + hdist lengths as one sequence, run-length coded
    uint32_t* clf = w.hist + DFL_C0;
    _Pragma("nounroll") for (uint32_t s = 0; s < DFL_NCL; s++) clf[s] = 0;
    const uint32_t nseq = hlit + hdist;
    uint32_t n_tok = 0, extra_bits = 0;
    _Pragma("nounroll") for (uint32_t i = 0; i < nseq;) {
        const uint32_t v = i < hlit ? lens[i] : lens[DFL_D0 + i - hlit];
        uint32_t run = 1;
        _Pragma("nounroll") while (i + run < nseq && (i + run < hlit ? lens[i + run] : lens[DFL_D0 + i + run - hlit]) == v) run++;
        i += run;
        if (v) {  // the length itself, then repeats of it
            w.tok[n_tok++] = (uint16_t)v;
            clf[v]++;
            run--;
        }
        _Pragma("nounroll") while (run >= 3) {
            const uint32_t sym = v ? 16u : run >= 11 ? 18u : 17u;
            const uint32_t base = v ? 3u : run >= 11 ? 11u : 3u, most = v ? 6u : run >= 11 ? 138u : 10u;
            const uint32_t take = run < most ? run : most;
            w.tok[n_tok++] = (uint16_t)(sym | ((take - base) << 5));
            clf[sym]++;
            extra_bits += dfl_cl_extra_bits(sym);
            run -= take;
        }
        _Pragma("nounroll") for (; run; run--) {
            w.tok[n_tok++] = (uint16_t)v;
            clf[v]++;
        }
    }
    uint8_t* cl = lens + DFL_C0;
    const uint32_t nu = dfl_huff_lengths(clf, DFL_NCL, 7, cl, w.srt + DFL_C0, w.work);
    if (nu == 1) cl[w.srt[DFL_C0] == 0 ? 1 : 0] = 1;  // an inflater wants this code complete: a second code of one bit, never sent
    uint32_t hclen = DFL_NCL;
    _Pragma("nounroll") while (hclen > 4 && !cl[dfl_cl_order(hclen - 1)]) hclen--;
    uint32_t hdr = 3 + 14 + 3 * hclen + extra_bits;
    _Pragma("nounroll") for (uint32_t s = 0; s < DFL_NCL; s++) hdr += clf[s] * cl[s];
    // the bits of the tokens and the end-of-block code under both sets of codes
    uint32_t dyn = hdr, fix = 3;
    _Pragma("nounroll") for (uint32_t s = 0; s < DFL_NLIT; s++) {
        const uint32_t eb = s > 256 ? dfl_len_extra_bits(s - 257) : 0u;
        dyn += w.hist[s] * (lens[s] + eb);
        fix += w.hist[s] * (dfl_fixed_len(s) + eb);
    }
    _Pragma("nounroll") for (uint32_t s = 0; s < DFL_NDIST; s++) {
        const uint32_t eb = dfl_dist_extra_bits(s);
        dyn += w.hist[DFL_D0 + s] * (lens[DFL_D0 + s] + eb);
        fix += w.hist[DFL_D0 + s] * (5 + eb);
    }
    const uint32_t stored = 8 * (w.len + 5);  // 3 bits, padding to the byte, LEN, NLEN, the payload
    st.cost[DFL_STORED] = stored;
    st.cost[DFL_FIXED] = fix;
    st.cost[DFL_DYNAMIC] = dyn;
    st.mode = stored <= fix && stored <= dyn ? DFL_STORED : fix <= dyn ? DFL_FIXED : DFL_DYNAMIC;
    st.n_tok = n_tok;
    st.hlit = hlit;
    st.hdist = hdist;
    st.hclen = hclen;
    st.hdr_bits = st.mode == DFL_DYNAMIC ? hdr : 3;
    if (st.mode == DFL_STORED) return;
    if (st.mode == DFL_FIXED) {
        _Pragma("nounroll") for (uint32_t s = 0; s < DFL_D0; s++) lens[s] = (uint8_t)dfl_fixed_len(s);
        _Pragma("nounroll") for (uint32_t s = 0; s < DFL_NDIST; s++) lens[DFL_D0 + s] = 5;
    }
    dfl_huff_codes(lens, DFL_D0, w.code, w.work);
    dfl_huff_codes(lens + DFL_D0, DFL_NDIST, w.code + DFL_D0, w.work);
    dfl_huff_codes(cl, DFL_NCL, w.code + DFL_C0, w.work);
}

// One lane, behind the second walk: bits[] becomes where each lane's tokens start; everything of the block that is no token.
DFL_HD void dfl_frame(const dfl_ws_t& w) {
    dfl_state_t& st = *w.st;
    uint32_t raw = 0;
    _Pragma("nounroll") for (uint32_t l = 0; l < BGZF_LANES; l++) raw ^= w.crcp[l];
    const uint32_t crc = bam_crc_finish(raw, w.len);
    if (st.mode == DFL_STORED) {  // the header and the payload are in the slot
        bam_put32(w.slot + BGZF_HEAD + w.len, crc);
        bam_put32(w.slot + BGZF_HEAD + w.len + 4, w.len);
        st.total = w.len + BGZF_EXTRA;
        return;
    }
    uint32_t at = 8 * 18;
    dfl_put(w.img, at, 1u | (st.mode << 1), 3);  // BFINAL, BTYPE
    at += 3;
    if (st.mode == DFL_DYNAMIC) {
        dfl_put(w.img, at, (st.hlit - 257) | ((st.hdist - 1) << 5) | ((st.hclen - 4) << 10), 14);
        at += 14;
        _Pragma("nounroll") for (uint32_t i = 0; i < st.hclen; i++, at += 3) dfl_put(w.img, at, w.lens[DFL_C0 + dfl_cl_order(i)], 3);
        _Pragma("nounroll") for (uint32_t i = 0; i < st.n_tok; i++) {
            const uint32_t sym = w.tok[i] & 31u, c = w.code[DFL_C0 + sym], eb = dfl_cl_extra_bits(sym);
            dfl_put(w.img, at, (c & 0xFFFFu) | ((uint32_t)(w.tok[i] >> 5) << (c >> 16)), (c >> 16) + eb);
            at += (c >> 16) + eb;
        }
    }
    _Pragma("nounroll") for (uint32_t l = 0; l < BGZF_LANES; l++) {
        const uint32_t b = w.bits[l];
        w.bits[l] = at;
        at += b;
    }
    dfl_put(w.img, at, w.code[256] & 0xFFFFu, w.code[256] >> 16);
    at += w.code[256] >> 16;
    const uint32_t tail = (at + 7) >> 3;  // the byte of the CRC-32
    st.total = tail + 8;
    _Pragma("nounroll") for (uint32_t i = 0; i < 18; i++) dfl_put(w.img, 8 * i, bgzf_head_byte(i, st.total - BGZF_EXTRA), 8);
    dfl_put(w.img, 8 * tail, crc, 32);
    dfl_put(w.img, 8 * tail + 32, w.len, 32);
}

// ---- the phases -----------------------------------------------------------------------------------------------------------------
DFL_HD void dfl_phase(const dfl_ws_t& w, uint32_t k, uint32_t lane) {
    const uint32_t nt = dfl_tiles(w.len);
    if (k == 0) {
        for (uint32_t i = lane; i < DFL_TAB; i += BGZF_LANES) w.tab[i] = 0;
        for (uint32_t i = lane; i < DFL_NEAR; i += BGZF_LANES) w.near[i] = DFL_NONE;
        for (uint32_t i = lane; i < DFL_SYMS; i += BGZF_LANES) {
            w.hist[i] = 0;
            w.lens[i] = 0;
        }
        return;
    }
    k -= DFL_PHASES_HEAD;
    if (k < 3 * nt) {
        const uint32_t tile = k / 3, step = k - 3 * tile;
        if (step == 0) dfl_tile_hash(w, tile, lane);
        else if (step == 1) dfl_tile_match(w, tile, lane);
        else dfl_tile_insert(w, tile, lane);
        return;
    }
    k -= 3 * nt;
    const dfl_state_t& st = *w.st;
    switch (k) {
        case 0: dfl_seg_exits(w, lane); break;
        case 1:
            if (lane == 0) dfl_seg_entries(w);
            break;
        case 2:
            dfl_walk<0>(w, lane);
            if (lane == 0) dfl_add(w.hist + 256, 1u);  // the end-of-block code
            break;
        case 3:  // near and tab are free from here
            for (uint32_t s = lane; s < DFL_NLIT; s += BGZF_LANES)
                if (w.hist[s]) w.srt[dfl_huff_rank(w.hist, DFL_NLIT, s)] = (uint16_t)s;
            if (lane < DFL_NDIST && w.hist[DFL_D0 + lane]) w.srt[DFL_D0 + dfl_huff_rank(w.hist + DFL_D0, DFL_NDIST, lane)] = (uint16_t)lane;
            break;
        case 4: {
            if (lane == 0 || lane == 64) {  // two wavefronts: the two trees at the same time
                const uint32_t n = lane ? DFL_NDIST : DFL_NLIT, at = lane ? DFL_D0 : 0u;
                uint32_t nu = 0;
                for (uint32_t s = 0; s < n; s++) nu += w.hist[at + s] ? 1u : 0u;
                dfl_huff_build(w.hist + at, w.srt + at, nu, 15, w.lens + at, w.work + (lane ? DFL_WORK_LIT : 0u));
                if (lane && !nu) w.lens[DFL_D0] = 1;  // no match: there is still one distance code
            }
            w.T[lane] = bam_crc_byte_entry(lane);
            break;
        }
        case 5:
            if (lane == 0) dfl_choose(w);
            bam_crc_slices(w.T, lane);
            for (uint32_t i = 0; i < 4; i++) w.K[256 * i + lane] = bam_crc_far_entry(256 * i + lane);
            break;
        case 6:
            w.crcp[lane] = bgzf_lane_crc(w.T, w.K, w.src, w.len, lane);
            if (st.mode == DFL_STORED) {
                if (lane < BGZF_HEAD) w.slot[lane] = bgzf_head_byte(lane, w.len);
                sam_copy_line(w.src, w.slot + BGZF_HEAD, w.len, lane, BGZF_LANES, 0, UINT64_MAX, true);
            } else {
                for (uint32_t i = lane; i < DFL_IMAGE_WORDS; i += BGZF_LANES) w.img[i] = 0;
            }
            break;
        case 7:
            if (st.mode != DFL_STORED) w.bits[lane] = dfl_walk<1>(w, lane);
            break;
        case 8:
            if (lane == 0) dfl_frame(w);
            break;
        case 9:
            if (st.mode != DFL_STORED) dfl_walk<2>(w, lane);
            break;
        default:  // 10
            if (st.mode != DFL_STORED)
                for (uint32_t v = lane; 16 * v < st.total; v += BGZF_LANES) {
                    const sam_v16 x = {{w.img[4 * v], w.img[4 * v + 1], w.img[4 * v + 2], w.img[4 * v + 3]}};
                    *(sam_v16*)(w.slot + 16 * v) = x;
                }
            break;
    }
}

#endif
