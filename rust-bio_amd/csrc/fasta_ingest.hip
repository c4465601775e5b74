// FASTA ingest on the device: bio::io::fasta::Reader::read / Records and Record::check (io/fasta.rs:334-359, 982-1009,
// 1090-1111) over a text that is already in HBM, and the reference builder that turns the parsed records into the index
// text (S0 $ S1 $ ... $, or T $ R $ for an FMD index) with the contig table and names of the SAM writer.  Rules:
// include/biogpu.h.
//
// Unlike FASTQ, a line's role is decided by its own first byte ('>' or not), so nothing has to be guessed and there is ONE
// path for every input.  What a byte needs to know from outside its tile is small:
//   * forwards: whether the line open at the tile's start is a header (FA_HDR) or a sequence line (FA_SEQ);
//   * backwards: whether the white space the tile ends in is followed, in the same line, by a character that is not white
//     space (then str::trim_end keeps it) or by the line's end (then it is trimmed) — a run may span any number of tiles;
//   * the running counts of header lines and of sequence bytes.
// So:
//   A1  fa_summary_kernel   a tile of 8 KB per block, staged in LDS with four bytes either side (a multi-byte character may
//                           straddle the boundary); every thread owns 32 bytes and builds bit masks of them — newlines, last
//                           bytes of characters that are not White_Space, line starts, header starts — and the tile's summary:
//                           headers, sequence bytes kept for sure (split into those of the line open at the tile's start and the
//                           rest), bytes pending at its end, the type of its last line, its first event (newline or character);
//                           the first byte that breaks UTF-8 goes to a global minimum;
//   A2  fa_scan_kernel      one block composes the summaries (1024 contiguous chunks, then the chunks' carries) into every
//                           tile's incoming line type, the fate of its pending bytes, and its record / sequence bases;
//   A3  fa_apply_kernel     the tile again, now with its carries: kept bytes are compacted in LDS and leave in aligned 16-byte
//                           stores, every header start files its record's id_off and seq_off, bytes Record::check rejects
//                           raise their record's flags;
//   A4  fa_records_kernel   one thread per record: header split (io/fasta.rs:346-348), lengths, check, the first empty record;
//   A5  fa_error_kernel     only if some byte broke UTF-8: the start of its line and the headers in front of it.
// The text is read twice and the sequences written once.  The first-line rule, the first I/O error and the first empty
// record are global minima that clip n_records on the host.
#include <algorithm>

#include "bg_common.h"
#include "dna_complement.h"
#include "white_space.h"

namespace {

constexpr uint32_t kFaTile = BG_FASTA_TILE, kFaThreads = 256, kFaSpan = 32, kFaHalo = 16;
static_assert(kFaTile == kFaThreads * kFaSpan, "a thread owns 32 bytes: its masks are 32-bit words");
enum : uint32_t { FA_CARRY = 0, FA_SEQ = 1, FA_HDR = 2 };    // type of the line a byte lies in (CARRY: the line open at the tile's start)
enum : uint32_t { FA_EV_NONE = 0, FA_EV_CHAR = 1, FA_EV_NL = 2 };  // next event at or after a byte: a non-white-space character ends, a newline
constexpr uint64_t kFaNone = ~0ull;

struct FaTileSum {   // A1 -> A2
    uint32_t n_hdr;      // header line starts
    uint32_t k_first;    // bytes kept for sure in the line open at the tile's start, if that is a sequence line
    uint32_t k_rest;     // bytes kept for sure in sequence lines that start in the tile
    uint32_t pend;       // white space behind the tile's last event, if its line is not a header for sure
    uint32_t last_state; // line type at the tile's last byte (FA_CARRY: no line starts in the tile)
    uint32_t first_ev;   // the tile's first event
    uint32_t has_nl;     // the tile holds a newline (A5 looks for a line's start by it)
    uint32_t pad;
};
struct FaTileIn {    // A2 -> A3
    uint64_t rec_base, seq_base;  // header lines / kept bytes in front of the tile
    uint32_t h_in;       // FA_SEQ / FA_HDR: the line open at the tile's start
    uint32_t res_out;    // 1: the tile's pending bytes are kept
    uint32_t pad[2];
};
static_assert(sizeof(FaTileSum) == 32 && sizeof(FaTileIn) == 32, "");

__device__ __forceinline__ bool fa_ascii_ws(uint32_t c) { return c == 0x20 || (c >= 9 && c <= 13); }
__device__ __forceinline__ bool fa_cont(uint32_t c) { return (c & 0xC0) == 0x80; }
__device__ __forceinline__ uint32_t fa_bits_below(uint32_t b) { return (uint32_t)((1ull << b) - 1); }  // b <= 32

// what a thread knows of its 32 bytes
struct FaMasks {
    uint32_t in;   // inside the text
    uint32_t nl;   // '\n'
    uint32_t ch;   // last byte of a character that is not White_Space (char::is_whitespace; '\n' is)
    uint32_t ls;   // first byte of a line
    uint32_t hs;   // ... that is '>'
    bool hi;       // some byte >= 0x80
};

// Stage the tile at t0 (with kFaHalo bytes either side, of which four are filled) in s and build the caller's masks.  Bytes outside
// the text read as 0: neither a newline nor white space nor a continuation byte.  Ends with the block synchronised.
__device__ __forceinline__ FaMasks fa_stage(const uint8_t* __restrict__ t, uint64_t len, uint64_t t0, uint8_t* s) {
    const uint32_t tid = threadIdx.x;
    const uint64_t base = t0 + (uint64_t)tid * kFaSpan;
    uint32_t w[8];
    uint4* s4 = (uint4*)(s + kFaHalo + tid * kFaSpan);
    // a whole tile of a 16-byte aligned text: two vector loads per thread; otherwise (the text's last tile, a text at an odd
    // address) the block copies the tile a byte per thread and step, 64 consecutive bytes per wavefront
    const bool whole = (((uintptr_t)t) & 15) == 0 && t0 + kFaTile <= len;
    if (whole) {
        s4[0] = *(const uint4*)(t + base);
        s4[1] = *(const uint4*)(t + base + 16);
    } else {
        for (uint32_t j = tid; j < kFaTile; j += kFaThreads) s[kFaHalo + j] = t0 + j < len ? t[t0 + j] : 0;
    }
    if (tid < 4) {
        const uint64_t p = t0 + tid;  // t0 - 4 + tid
        s[kFaHalo - 4 + tid] = p >= 4 ? t[p - 4] : 0;
    } else if (tid < 8) {
        const uint64_t p = t0 + kFaTile + (tid - 4);
        s[kFaHalo + kFaTile + (tid - 4)] = p < len ? t[p] : 0;
    }
    __syncthreads();
    {
        const uint4 a = s4[0], b = s4[1];
        w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
    }
    FaMasks m;
    const uint64_t left = base < len ? len - base : 0;
    m.in = left >= kFaSpan ? ~0u : fa_bits_below((uint32_t)left);
    m.nl = 0, m.ch = 0;
    uint32_t gt = 0;
#pragma unroll
    for (int i = 0; i < (int)kFaSpan; i++) {
        const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 0xFF;
        m.nl |= (uint32_t)(c == '\n') << i;
        gt |= (uint32_t)(c == '>') << i;
        m.ch |= (uint32_t)(c < 0x80 && !fa_ascii_ws(c)) << i;
    }
    m.hi = ((w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) & 0x80808080u) != 0;
    if (m.hi) {  // a character >= U+0080 counts at its last byte; the multi-byte members of White_Space do not count
        const uint8_t* p = s + kFaHalo + tid * kFaSpan;
        for (int i = 0; i < (int)kFaSpan; i++) {
            const uint32_t c = p[i];
            if (c < 0x80 || !fa_cont(c) || fa_cont(p[i + 1])) continue;
            const uint32_t b = p[i - 1], a = p[i - 2];
            const bool ws = (b == 0xC2 && (c == 0x85 || c == 0xA0)) || (a == 0xE1 && b == 0x9A && c == 0x80) ||
                            (a == 0xE2 && b == 0x80 && ((c >= 0x80 && c <= 0x8A) || c == 0xA8 || c == 0xA9 || c == 0xAF)) ||
                            (a == 0xE2 && b == 0x81 && c == 0x9F) || (a == 0xE3 && b == 0x80 && c == 0x80);
            if (!ws) m.ch |= 1u << i;
        }
    }
    m.ch &= m.in;
    m.nl &= m.in;
    const bool prev_nl = base == 0 || s[kFaHalo + tid * kFaSpan - 1] == '\n';
    m.ls = ((m.nl << 1) | (prev_nl ? 1u : 0u)) & m.in;
    m.hs = m.ls & gt;
    return m;
}

// Line type of each of the thread's bytes: `hdr` where it is FA_HDR, `carry` where it is `h_in` itself (no line start between the
// tile's start and the byte).  h_in: FA_CARRY in A1, the scanned type in A3.  *last: the type at the thread's last byte.
// s_f: 4 words of LDS.  Synchronises the block once.
__device__ __forceinline__ void fa_line_types(const FaMasks& m, uint32_t h_in, uint32_t* s_f, uint32_t& hdr, uint32_t& carry, uint32_t& last) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool has = m.ls != 0;
    const bool last_hdr = has && ((m.hs >> (31 - __clz(m.ls))) & 1);
    const uint64_t bl = __ballot(has), bh = __ballot(last_hdr);
    if (lane == 0) s_f[wave] = bl ? (((bh >> (63 - __clzll((long long)bl))) & 1) ? FA_HDR : FA_SEQ) : FA_CARRY;
    __syncthreads();
    uint32_t st = h_in;
    const uint64_t before = bl & ((1ull << lane) - 1);
    if (before) {
        st = ((bh >> (63 - __clzll((long long)before))) & 1) ? FA_HDR : FA_SEQ;
    } else {
        for (int w = (int)wave - 1; w >= 0; w--)
            if (s_f[w] != FA_CARRY) {
                st = s_f[w];
                break;
            }
    }
    hdr = 0, carry = 0;
    uint32_t pos = 0, rem = m.ls;
    while (true) {  // segments between line starts
        const uint32_t b = rem ? (uint32_t)__ffs((int)rem) - 1 : 32;
        const uint32_t seg = fa_bits_below(b) & ~fa_bits_below(pos);
        if (st == FA_HDR) hdr |= seg;
        if (st == h_in && pos == 0) carry |= seg;
        if (!rem) break;
        rem &= rem - 1;
        st = ((m.hs >> b) & 1) ? FA_HDR : FA_SEQ;
        pos = b;
        if (pos == 0) carry = 0;
    }
    last = st;
}

// `keep`: bytes whose next event, themselves included, is a character's end (str::trim_end keeps them); `pend`: bytes behind the
// tile's last event (their fate lies in later tiles).  ev_out: FA_EV_NONE in A1, the scanned fate in A3 (then pend is empty).
// *first: the tile's first event.  s_b: 4 words of LDS.  Synchronises the block once.
__device__ __forceinline__ void fa_keep(const FaMasks& m, uint32_t ev_out, uint32_t* s_b, uint32_t& keep, uint32_t& pend, uint32_t& first) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ev = m.ch | m.nl;
    const bool has = ev != 0;
    const bool first_ch = has && ((m.ch >> (__ffs((int)ev) - 1)) & 1);
    const uint64_t bl = __ballot(has), bc = __ballot(first_ch);
    if (lane == 0) s_b[wave] = bl ? (((bc >> (__ffsll((long long)bl) - 1)) & 1) ? FA_EV_CHAR : FA_EV_NL) : FA_EV_NONE;
    __syncthreads();
    uint32_t cur = ev_out;
    const uint64_t after = lane == 63 ? 0 : bl & ~((2ull << lane) - 1);
    if (after) {
        cur = ((bc >> (__ffsll((long long)after) - 1)) & 1) ? FA_EV_CHAR : FA_EV_NL;
    } else {
        for (uint32_t w = wave + 1; w < kFaThreads / 64; w++)
            if (s_b[w] != FA_EV_NONE) {
                cur = s_b[w];
                break;
            }
    }
    first = FA_EV_NONE;
    for (uint32_t w = 0; w < kFaThreads / 64; w++)
        if (s_b[w] != FA_EV_NONE) {
            first = s_b[w];
            break;
        }
    keep = 0, pend = 0;
    uint32_t hi = 32, rem = ev;
    while (true) {  // segments between events, from the top
        const uint32_t lo = rem ? 32 - (uint32_t)__clz(rem) : 0;  // one past the highest event left
        const uint32_t seg = fa_bits_below(hi) & ~fa_bits_below(lo);
        if (cur == FA_EV_CHAR) keep |= seg;
        if (cur == FA_EV_NONE) pend |= seg;
        if (!rem) break;
        const uint32_t b = lo - 1;
        cur = ((m.ch >> b) & 1) ? FA_EV_CHAR : FA_EV_NL;
        rem &= ~(1u << b);
        hi = lo;
    }
    keep &= m.in;
    pend &= m.in;
}

// first byte of the thread's span at which a strict UTF-8 decoder fails, or kFaNone.  p: the span in LDS (four bytes either side readable)
__device__ uint64_t fa_first_bad(const uint8_t* p, uint32_t in, uint64_t base) {
    for (int i = 0; i < (int)kFaSpan; i++) {
        if (!((in >> i) & 1)) break;
        const uint32_t c = p[i];
        if (c < 0x80) continue;
        bool ok;
        if (fa_cont(c)) {  // covered by a lead byte one, two or three bytes back
            const uint32_t b1 = p[i - 1], b2 = p[i - 2], b3 = p[i - 3];
            ok = (b1 >= 0xC2 && b1 <= 0xF4) || (fa_cont(b1) && b2 >= 0xE0 && b2 <= 0xF4) || (fa_cont(b1) && fa_cont(b2) && b3 >= 0xF0 && b3 <= 0xF4);
        } else if (c >= 0xC2 && c <= 0xDF) {
            ok = fa_cont(p[i + 1]);
        } else if (c >= 0xE0 && c <= 0xEF) {
            const uint32_t n1 = p[i + 1];
            const uint32_t lo = c == 0xE0 ? 0xA0 : 0x80, hi = c == 0xED ? 0x9F : 0xBF;  // no overlong forms, no surrogates
            ok = n1 >= lo && n1 <= hi && fa_cont(p[i + 2]);
        } else if (c >= 0xF0 && c <= 0xF4) {
            const uint32_t n1 = p[i + 1];
            const uint32_t lo = c == 0xF0 ? 0x90 : 0x80, hi = c == 0xF4 ? 0x8F : 0xBF;  // U+10000 .. U+10FFFF
            ok = n1 >= lo && n1 <= hi && fa_cont(p[i + 2]) && fa_cont(p[i + 3]);
        } else {
            ok = false;
        }
        if (!ok) return base + i;
    }
    return kFaNone;
}

__device__ __forceinline__ uint64_t fa_wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
        v += (uint64_t)hi << 32 | lo;
    }
    return v;
}

// ---- A1 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFaThreads) void fa_summary_kernel(const uint8_t* __restrict__ t, uint64_t len, FaTileSum* __restrict__ sum,
                                                                unsigned long long* __restrict__ first_bad) {
    __shared__ uint4 s_tile4[(kFaHalo + kFaTile + kFaHalo) / 16];
    __shared__ uint32_t s_f[4], s_b[4];
    __shared__ uint64_t s_sum[4];
    uint8_t* s = (uint8_t*)s_tile4;
    const uint32_t tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * kFaTile;
    const FaMasks m = fa_stage(t, len, t0, s);
    if (m.hi) {
        const uint64_t bad = fa_first_bad(s + kFaHalo + tid * kFaSpan, m.in, t0 + (uint64_t)tid * kFaSpan);
        if (bad != kFaNone) atomicMin(first_bad, (unsigned long long)bad);
    }
    uint32_t hdr, carry, last, keep, pend, first;
    fa_line_types(m, FA_CARRY, s_f, hdr, carry, last);
    fa_keep(m, FA_EV_NONE, s_b, keep, pend, first);
    const int any_nl = __syncthreads_or(m.nl != 0);
    // four counts of at most 8192 in one word
    uint64_t v = (uint64_t)__popc(m.hs) | (uint64_t)__popc(keep & carry) << 16 | (uint64_t)__popc(keep & ~carry & ~hdr) << 32 | (uint64_t)__popc(pend) << 48;
    v = fa_wave_sum(v);
    if ((tid & 63) == 0) s_sum[tid >> 6] = v;
    __syncthreads();
    if (tid == kFaThreads - 1) {
        const uint64_t a = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        FaTileSum o = {};
        o.n_hdr = (uint32_t)(a & 0xFFFF);
        o.k_first = (uint32_t)((a >> 16) & 0xFFFF);
        o.k_rest = (uint32_t)((a >> 32) & 0xFFFF);
        o.pend = last == FA_HDR ? 0u : (uint32_t)(a >> 48);  // (pending bytes lie in the tile's last line)
        o.last_state = last;
        o.first_ev = first;
        o.has_nl = any_nl ? 1u : 0u;
        sum[blockIdx.x] = o;
    }
}

// ---- A2 ---------------------------------------------------------------------------------------------------------------
// out[0] = header lines, out[1] = sequence bytes of the whole text
__global__ __launch_bounds__(1024) void fa_scan_kernel(const FaTileSum* __restrict__ sum, FaTileIn* __restrict__ tin, uint32_t n_tiles,
                                                       uint64_t* __restrict__ out) {
    __shared__ uint32_t s_f[1024], s_b[1024];
    __shared__ uint64_t s_h[1024], s_k[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t chunk = (n_tiles + 1023) / 1024;
    const uint32_t lo = min(tid * chunk, n_tiles), hi = min(lo + chunk, n_tiles);
    uint32_t fwd = FA_CARRY, bwd = FA_EV_NONE;
#pragma unroll 4
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t ls = sum[i].last_state, fe = sum[i].first_ev;
        if (ls != FA_CARRY) fwd = ls;
        if (bwd == FA_EV_NONE) bwd = fe;
    }
    s_f[tid] = fwd;
    s_b[tid] = bwd;
    __syncthreads();
    uint32_t h = FA_SEQ;  // (tile 0 starts a line: its carry is never looked at)
    for (int j = (int)tid - 1; j >= 0; j--)
        if (s_f[j] != FA_CARRY) {
            h = s_f[j];
            break;
        }
    uint32_t r = FA_EV_NL;  // the end of the text ends the line
    for (uint32_t j = tid + 1; j < 1024; j++)
        if (s_b[j] != FA_EV_NONE) {
            r = s_b[j];
            break;
        }
    for (uint32_t i = hi; i > lo; i--) {  // fate of every tile's pending bytes
        tin[i - 1].res_out = r == FA_EV_CHAR ? 1u : 0u;
        const uint32_t fe = sum[i - 1].first_ev;
        if (fe != FA_EV_NONE) r = fe;
    }
    uint64_t sh = 0, sk = 0;
    for (uint32_t i = lo; i < hi; i++) {  // incoming line type and kept bytes of every tile
        const FaTileSum S = sum[i];
        const uint32_t eff = S.last_state == FA_CARRY ? h : S.last_state;
        const uint64_t kept = (uint64_t)S.k_rest + (h == FA_SEQ ? S.k_first : 0u) + ((tin[i].res_out && eff == FA_SEQ) ? S.pend : 0u);
        tin[i].h_in = h;
        tin[i].seq_base = kept;
        sh += S.n_hdr;
        sk += kept;
        h = eff;
    }
    s_h[tid] = sh;
    s_k[tid] = sk;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint64_t uh = tid >= o ? s_h[tid - o] : 0, uk = tid >= o ? s_k[tid - o] : 0;
        __syncthreads();
        s_h[tid] += uh;
        s_k[tid] += uk;
        __syncthreads();
    }
    uint64_t rh = s_h[tid] - sh, rk = s_k[tid] - sk;
    for (uint32_t i = lo; i < hi; i++) {
        const uint64_t kept = tin[i].seq_base;
        tin[i].rec_base = rh;
        tin[i].seq_base = rk;
        rh += sum[i].n_hdr;
        rk += kept;
    }
    if (tid == 1023) {
        out[0] = s_h[1023];
        out[1] = s_k[1023];
    }
}

// ---- A3 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFaThreads) void fa_apply_kernel(const uint8_t* __restrict__ t, uint64_t len, const FaTileIn* __restrict__ tin,
                                                              bg_fasta_record_t* __restrict__ recs, uint64_t* __restrict__ seq_off, uint64_t cap,
                                                              uint8_t* __restrict__ seq, uint32_t* __restrict__ chk) {
    __shared__ uint4 s_tile4[(kFaHalo + kFaTile + kFaHalo) / 16];
    __shared__ uint4 s_out4[(kFaTile + 32) / 16];
    __shared__ uint32_t s_f[4], s_b[4];
    __shared__ uint64_t s_w[4];
    uint8_t* s = (uint8_t*)s_tile4;
    uint8_t* s_out = (uint8_t*)s_out4;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * kFaTile;
    const FaTileIn ti = tin[blockIdx.x];
    const FaMasks m = fa_stage(t, len, t0, s);
    uint32_t hdr, carry, last, keep, pend, first;
    fa_line_types(m, ti.h_in, s_f, hdr, carry, last);
    fa_keep(m, ti.res_out ? FA_EV_CHAR : FA_EV_NL, s_b, keep, pend, first);
    const uint32_t K = keep & ~hdr;
    // exclusive prefixes over the block: kept bytes (low half), header starts (high half)
    const uint64_t mine = (uint64_t)__popc(K) | (uint64_t)__popc(m.hs) << 32;
    uint64_t inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t l = (uint32_t)__shfl_up((int)(uint32_t)inc, o), h = (uint32_t)__shfl_up((int)(uint32_t)(inc >> 32), o);
        if ((int)lane >= o) inc += (uint64_t)h << 32 | l;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint64_t wbase = 0, total = 0;
    for (uint32_t w = 0; w < kFaThreads / 64; w++) {
        if (w < wave) wbase += s_w[w];
        total += s_w[w];
    }
    const uint64_t ex = wbase + inc - mine;
    const uint32_t kept_before = (uint32_t)ex, hdr_before = (uint32_t)(ex >> 32), n_kept = (uint32_t)total;
    uint8_t* const D = seq + ti.seq_base;
    const uint32_t a = (uint32_t)((uintptr_t)D & 15);
    const uint8_t* p = s + kFaHalo + tid * kFaSpan;
    // kept bytes -> their place in the tile's output, shifted so that LDS vector q is the aligned global vector q
    uint32_t flags = 0;
    {
        uint32_t rem = K, d = a + kept_before;
        while (rem) {
            const uint32_t b = (uint32_t)__ffs((int)rem) - 1;
            rem &= rem - 1;
            const uint32_t c = p[b];
            s_out[d++] = (uint8_t)c;
            // Record::check (io/fasta.rs:997-1006): ASCII, then letters and - . *
            if (c >= 0x80) flags |= 1u;
            else if (!(((c | 0x20) >= 'a' && (c | 0x20) <= 'z') || c == '-' || c == '.' || c == '*')) flags |= 2u;
        }
    }
    if (flags) {  // (rare) file the flags with the record each offending byte belongs to
        uint32_t rem = K;
        while (rem) {
            const uint32_t b = (uint32_t)__ffs((int)rem) - 1;
            rem &= rem - 1;
            const uint32_t c = p[b];
            const uint32_t f = c >= 0x80 ? 1u : !(((c | 0x20) >= 'a' && (c | 0x20) <= 'z') || c == '-' || c == '.' || c == '*') ? 2u : 0u;
            const uint64_t k1 = ti.rec_base + hdr_before + __popc(m.hs & fa_bits_below(b + 1));  // headers up to the byte
            if (f && k1 >= 1 && k1 - 1 < cap) atomicOr(&chk[k1 - 1], f);
        }
    }
    {  // header starts: the record's id_off (the rest of the record: A4) and seq_off
        uint32_t rem = m.hs, j = 0;
        while (rem) {
            const uint32_t b = (uint32_t)__ffs((int)rem) - 1;
            rem &= rem - 1;
            const uint64_t k = ti.rec_base + hdr_before + j++;
            if (k < cap) recs[k].id_off = t0 + (uint64_t)tid * kFaSpan + b + 1;
            if (k <= cap) seq_off[k] = ti.seq_base + kept_before + __popc(K & fa_bits_below(b));
        }
    }
    __syncthreads();
    const uint32_t end = a + n_kept, nv = (end + 15) / 16;
    for (uint32_t q = tid; q < nv; q += kFaThreads) {
        const uint32_t lo = q * 16, hi = lo + 16;
        if (lo >= a && hi <= end) {
            *(uint4*)(D - a + lo) = s_out4[q];
        } else {
            for (uint32_t j = max(lo, a); j < min(hi, end); j++) D[j - a] = s_out[j];
        }
    }
}

// ---- A4 ---------------------------------------------------------------------------------------------------------------
// one thread per record: line[1..].trim_end().splitn(2, char::is_whitespace) (io/fasta.rs:346-348), the sequence's place and
// length, Record::check, and the first record that is_empty() (io/fasta.rs:982-984, 1102)
__global__ __launch_bounds__(256) void fa_records_kernel(const uint8_t* __restrict__ t, uint64_t len, bg_fasta_record_t* __restrict__ recs,
                                                         const uint64_t* __restrict__ seq_off, uint64_t n, const uint32_t* __restrict__ chk,
                                                         unsigned long long* __restrict__ first_empty) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t a = recs[k].id_off;
    uint64_t i = a, first_ws = kFaNone, ws_len = 0, trimmed = a;
    while (i < len && t[i] != '\n') {
        const uint32_t c = t[i];
        uint32_t cp = c, nb = 1;
        if (c >= 0xC2) {
            nb = c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4;
            cp = c & (0xFFu >> (nb + 1));
            for (uint32_t j = 1; j < nb; j++) cp = (cp << 6) | (i + j < len ? (t[i + j] & 0x3Fu) : 0u);
        }
        if (is_ws(cp)) {
            if (first_ws == kFaNone) first_ws = i, ws_len = nb;
        } else {
            trimmed = i + nb;
        }
        i += nb;
    }
    bg_fasta_record_t o = {};
    o.id_off = a;
    if (first_ws != kFaNone && first_ws < trimmed) {
        o.id_len = (uint32_t)(first_ws - a);
        o.desc_off = first_ws + ws_len;
        o.desc_len = (uint32_t)(trimmed - o.desc_off);
        o.has_desc = 1;
    } else {
        o.id_len = (uint32_t)(trimmed - a);
    }
    o.seq_off = seq_off[k];
    o.seq_len = seq_off[k + 1] - o.seq_off;
    const uint32_t f = chk[k];
    o.check = o.id_len == 0 ? BG_FACHECK_EMPTY_ID : (f & 1) ? BG_FACHECK_NONASCII_SEQ : (f & 2) ? BG_FACHECK_INVALID_SEQ : BG_FACHECK_OK;
    recs[k] = o;
    if (o.id_len == 0 && !o.has_desc && o.seq_len == 0) atomicMin(first_empty, (unsigned long long)k);
}

// ---- A5 ---------------------------------------------------------------------------------------------------------------
// out[0] = start of the line that holds byte `bad`, out[1] = header lines that start in front of it.  The newline in front of the
// byte is sought in its own tile, then (a line may be a whole chromosome) over the summaries for the nearest tile that holds one.
__global__ __launch_bounds__(256) void fa_error_kernel(const uint8_t* __restrict__ t, const FaTileSum* __restrict__ sum, const FaTileIn* __restrict__ tin,
                                                       const unsigned long long* __restrict__ bad_p, uint64_t* __restrict__ out) {
    __shared__ unsigned long long s_best, s_tile;
    __shared__ uint32_t s_cnt;
    const uint32_t tid = threadIdx.x;
    const uint64_t bad = *bad_p;
    if (tid == 0) s_best = 0, s_tile = 0, s_cnt = 0;
    __syncthreads();
    // one past the last newline in [lo, hi), or 0
    auto last_newline = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo + tid; i < hi; i += 256)
            if (t[i] == '\n') atomicMax(&s_best, (unsigned long long)(i + 1));
        __syncthreads();
        return (uint64_t)s_best;
    };
    const uint64_t tile_b = bad / kFaTile;
    uint64_t eo = last_newline(tile_b * kFaTile, bad);
    if (eo == 0) {  // (uniform: every thread read the same s_best behind the barrier)
        for (uint64_t hi = tile_b; hi > 0;) {  // 256 tiles a step, nearest first
            const uint64_t lo = hi > 256 ? hi - 256 : 0;
            const uint64_t i = lo + tid;
            if (i < hi && sum[i].has_nl) atomicMax(&s_tile, (unsigned long long)(i + 1));
            __syncthreads();
            const uint64_t found = s_tile;
            __syncthreads();  // (every thread has read s_tile before the next step may raise it)
            if (found) {
                eo = last_newline((found - 1) * kFaTile, found * kFaTile);
                break;
            }
            hi = lo;
        }
    }
    const uint64_t tile = eo / kFaTile;
    uint32_t c = 0;
    for (uint64_t i = tile * kFaTile + tid; i < eo; i += 256) c += t[i] == '>' && (i == 0 || t[i - 1] == '\n');
    if (c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (tid == 0) {
        out[0] = eo;
        out[1] = tin[tile].rec_base + s_cnt;
    }
}

// ---- the reference builder ----------------------------------------------------------------------------------------------
// R1: starts[i] = sum over j < i of (seq_len_j + 1), name_off[i] = sum of id_len_j (n + 1 entries each); the first record whose
// check is not OK.  One block; contigs are few next to the bases they hold.
__global__ __launch_bounds__(1024) void fa_ref_layout_kernel(const bg_fasta_record_t* __restrict__ recs, uint64_t n, uint64_t* __restrict__ starts,
                                                             uint64_t* __restrict__ name_off, unsigned long long* __restrict__ first_bad) {
    __shared__ uint64_t s_a[1024], s_b[1024];
    const uint32_t tid = threadIdx.x;
    const uint64_t chunk = (n + 1023) / 1024;
    const uint64_t lo = std::min<uint64_t>(tid * chunk, n), hi = std::min<uint64_t>(lo + chunk, n);
    uint64_t sa = 0, sb = 0;
    for (uint64_t i = lo; i < hi; i++) {
        sa += recs[i].seq_len + 1;
        sb += recs[i].id_len;
        if (recs[i].check != BG_FACHECK_OK) atomicMin(first_bad, (unsigned long long)i);
    }
    s_a[tid] = sa;
    s_b[tid] = sb;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint64_t ua = tid >= o ? s_a[tid - o] : 0, ub = tid >= o ? s_b[tid - o] : 0;
        __syncthreads();
        s_a[tid] += ua;
        s_b[tid] += ub;
        __syncthreads();
    }
    uint64_t ra = s_a[tid] - sa, rb = s_b[tid] - sb;
    for (uint64_t i = lo; i < hi; i++) {
        starts[i] = ra;
        name_off[i] = rb;
        ra += recs[i].seq_len + 1;
        rb += recs[i].id_len;
    }
    if (tid == 1023) {
        starts[n] = s_a[1023];
        name_off[n] = s_b[1023];
    }
}
// R2: the contig table and the names, one thread per record
__global__ __launch_bounds__(256) void fa_ref_contigs_kernel(const bg_fasta_record_t* __restrict__ recs, uint64_t n, const uint8_t* __restrict__ fasta,
                                                             const uint64_t* __restrict__ starts, const uint64_t* __restrict__ name_off,
                                                             bg_sam_contig_t* __restrict__ contigs, char* __restrict__ names) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bg_fasta_record_t r = recs[i];
    bg_sam_contig_t c = {};
    c.start = starts[i];
    c.len = r.seq_len;
    c.name_off = name_off[i];
    c.name_len = r.id_len;
    contigs[i] = c;
    for (uint32_t j = 0; j < r.id_len; j++) names[c.name_off + j] = (char)fasta[r.id_off + j];
}
// R3: a segmented gather, 16 bytes of the output per thread.  Byte q of the output is byte o of T (T = S0 $ S1 $ ..., n_t bytes:
// without BG_FASTA_REF_FMD all of starts[n], with it one less — no '$' behind the last sequence) for q = o < n_t, its complement
// for q = 2 n_t - o (R written mirrored), and '$' at n_t and 2 n_t + 1.  The contig of o: binary search in starts, then
// followed up or down as the thread moves on.
__global__ __launch_bounds__(256) void fa_ref_text_kernel(const bg_fasta_record_t* __restrict__ recs, uint64_t n, const uint8_t* __restrict__ seq,
                                                          const uint64_t* __restrict__ starts, uint64_t n_t, uint64_t n_text, int upper,
                                                          uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(4))) uint8_t s_comp[256];
    load_complement(s_comp);
    const uint64_t q0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (q0 >= n_text) return;
    uint64_t ci = kFaNone;
    uint32_t w[4] = {0, 0, 0, 0};
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(16, n_text - q0);
    for (uint32_t j = 0; j < cnt; j++) {
        const uint64_t q = q0 + j;
        uint32_t c = '$';
        if (q != n_t && q < 2 * n_t + 1) {
            const bool rev = q > n_t;
            const uint64_t o = rev ? 2 * n_t - q : q;
            if (ci == kFaNone) {  // largest i with starts[i] <= o
                uint64_t lo = 0, hi = n;
                while (hi - lo > 1) {
                    const uint64_t mid = lo + (hi - lo) / 2;
                    if (starts[mid] <= o) lo = mid;
                    else hi = mid;
                }
                ci = lo;
            }
            while (o < starts[ci]) ci--;
            while (ci + 1 < n && o >= starts[ci + 1]) ci++;
            const uint64_t r = o - starts[ci];
            if (r < recs[ci].seq_len) {
                c = seq[recs[ci].seq_off + r];
                if (upper && c >= 'a' && c <= 'z') c -= 32;
                if (rev) c = s_comp[c];
            }
        }
        w[j >> 2] |= c << (8 * (j & 3));
    }
    if (cnt == 16 && ((uintptr_t)out & 15) == 0) {
        *(uint4*)(out + q0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (uint32_t j = 0; j < cnt; j++) out[q0 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
}

}  // namespace

extern "C" int bg_fasta_parse_dev(bg_ctx* ctx, const uint8_t* d_text, uint64_t len, bg_fasta_record_t* d_recs, uint64_t rec_cap, uint8_t* d_seq,
                                  uint64_t* d_seq_off, uint64_t* n_records, int32_t* status, uint64_t* err_pos, void* stream) {
    if (!ctx || !n_records || !status || !err_pos) return BG_ERR_INVALID_ARG;
    *n_records = 0;
    *status = BG_FASTA_OK;
    *err_pos = 0;
    hipStream_t st = (hipStream_t)stream;
    bg_scratch_guard guard(ctx, st);
    BG_HIP(hipSetDevice(ctx->device));
    const uint64_t zero = 0;
    if (len == 0) {
        if (d_seq_off) BG_HIP(hipMemcpyAsync(d_seq_off, &zero, 8, hipMemcpyHostToDevice, st));
        BG_HIP(hipStreamSynchronize(st));
        return BG_OK;
    }
    if (!d_text || !d_recs || !d_seq || !d_seq_off) return BG_ERR_INVALID_ARG;
    const uint64_t n_tiles = (len + kFaTile - 1) / kFaTile;
    if (n_tiles >= (1ull << 31)) return BG_ERR_TOO_LARGE;
    int rc;
    // aux: tile summaries, tile carries, misc = {first bad byte, headers, sequence bytes, first empty record, error line, headers in front of it}
    FaTileSum* d_sum;
    FaTileIn* d_tin;
    uint64_t* d_misc;
    if ((rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_sum = cv.take<FaTileSum>(n_tiles), d_tin = cv.take<FaTileIn>(n_tiles);
        d_misc = cv.take<uint64_t>(8);
    }))) return rc;
    uint64_t misc[6] = {kFaNone, 0, 0, kFaNone, 0, 0};
    BG_HIP(hipMemcpyAsync(d_misc, misc, sizeof(misc), hipMemcpyHostToDevice, st));
    fa_summary_kernel<<<dim3((uint32_t)n_tiles), dim3(kFaThreads), 0, st>>>(d_text, len, d_sum, (unsigned long long*)d_misc);
    fa_scan_kernel<<<dim3(1), dim3(1024), 0, st>>>(d_sum, d_tin, (uint32_t)n_tiles, d_misc + 1);
    BG_HIP(hipGetLastError());
    uint8_t first_byte = 0;
    BG_HIP(hipMemcpyAsync(misc, d_misc, 24, hipMemcpyDeviceToHost, st));
    BG_HIP(hipMemcpyAsync(&first_byte, d_text, 1, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    const uint64_t first_bad = misc[0], n_raw = misc[1], kept = misc[2];
    // more header lines than rec_cap: the records go to scratch, so that the count (which an empty record or an error beyond
    // rec_cap may still clip) is exact; they are copied out if it fits after all
    const bool spill = n_raw > rec_cap;
    uint32_t* d_chk;
    bg_fasta_record_t* recs;
    uint64_t* seq_off;
    if ((rc = bg_reserve_carved(&ctx->tb, &ctx->tb_bytes, [&](bg_carve& cv) {
        d_chk = cv.take<uint32_t>(n_raw);
        recs = spill ? cv.take<bg_fasta_record_t>(n_raw) : d_recs;
        seq_off = spill ? cv.take<uint64_t>(n_raw + 1) : d_seq_off;
    }))) return rc;
    if (first_bad != kFaNone) fa_error_kernel<<<dim3(1), dim3(256), 0, st>>>(d_text, d_sum, d_tin, (const unsigned long long*)d_misc, d_misc + 4);
    if (n_raw) {
        BG_HIP(hipMemsetAsync(d_chk, 0, n_raw * 4, st));
        fa_apply_kernel<<<dim3((uint32_t)n_tiles), dim3(kFaThreads), 0, st>>>(d_text, len, d_tin, recs, seq_off, n_raw, d_seq, d_chk);
        BG_HIP(hipMemcpyAsync(seq_off + n_raw, &kept, 8, hipMemcpyHostToDevice, st));
        fa_records_kernel<<<dim3((uint32_t)((n_raw + 255) / 256)), dim3(256), 0, st>>>(d_text, len, recs, seq_off, n_raw, d_chk,
                                                                                       (unsigned long long*)(d_misc + 3));
    }
    BG_HIP(hipGetLastError());
    BG_HIP(hipMemcpyAsync(misc + 3, d_misc + 3, 24, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    const uint64_t first_empty = misc[3], err_line = misc[4], hdr_before = misc[5];
    uint64_t n = 0;
    if (first_bad != kFaNone && err_line == 0) {  // read_line fails on the first line
        *status = BG_FASTA_IO;
    } else if (first_byte != '>') {
        *status = BG_FASTA_MISSING_GT;
    } else {
        // the line that fails is read by the record whose header is the last one in front of it (io/fasta.rs:351): that record is lost
        const uint64_t k_err = first_bad != kFaNone ? hdr_before - 1 : kFaNone;
        if (k_err != kFaNone && k_err <= first_empty) {
            *status = BG_FASTA_IO;
            *err_pos = err_line;
            n = k_err;
        } else {
            n = std::min(n_raw, first_empty);  // Records ends at the first empty record (io/fasta.rs:1102)
        }
    }
    *n_records = n;
    if (n > rec_cap) return BG_ERR_TOO_LARGE;
    if (n == 0) {
        BG_HIP(hipMemcpyAsync(d_seq_off, &zero, 8, hipMemcpyHostToDevice, st));
    } else if (spill) {
        BG_HIP(hipMemcpyAsync(d_recs, recs, n * sizeof(bg_fasta_record_t), hipMemcpyDeviceToDevice, st));
        BG_HIP(hipMemcpyAsync(d_seq_off, seq_off, (n + 1) * 8, hipMemcpyDeviceToDevice, st));
    }
    BG_HIP(hipStreamSynchronize(st));
    return BG_OK;
}

extern "C" int bg_fasta_parse(bg_ctx* ctx, const uint8_t* text, uint64_t len, bg_fasta_record_t* recs, uint64_t rec_cap, uint8_t* seq,
                              uint64_t* seq_off, uint64_t* n_records, int32_t* status, uint64_t* err_pos) {
    if (!ctx || !n_records || !status || !err_pos) return BG_ERR_INVALID_ARG;
    if (len && (!text || !recs || !seq || !seq_off)) return BG_ERR_INVALID_ARG;
    BG_HIP(hipSetDevice(ctx->device));
    int rc;
    const size_t need[4] = {std::max<uint64_t>(len, 16), std::max<uint64_t>(len, 16), (rec_cap + 1) * 8,
                            std::max<uint64_t>(rec_cap, 1) * sizeof(bg_fasta_record_t)};
    const int slot[4] = {0, 1, 2, 4};
    for (int i = 0; i < 4; i++)
        if ((rc = bg_reserve(&ctx->io[slot[i]], &ctx->io_cap[slot[i]], need[i]))) return rc;
    uint8_t *d_text = (uint8_t*)ctx->io[0], *d_seq = (uint8_t*)ctx->io[1];
    uint64_t* d_so = (uint64_t*)ctx->io[2];
    bg_fasta_record_t* d_recs = (bg_fasta_record_t*)ctx->io[4];
    hipStream_t st = ctx->stream;
    if (len) BG_HIP(hipMemcpyAsync(d_text, text, len, hipMemcpyHostToDevice, st));
    rc = bg_fasta_parse_dev(ctx, d_text, len, d_recs, rec_cap, d_seq, d_so, n_records, status, err_pos, st);
    if (rc) return rc;
    const uint64_t n = *n_records;
    if (seq_off) BG_HIP(hipMemcpyAsync(seq_off, d_so, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (n) BG_HIP(hipMemcpyAsync(recs, d_recs, n * sizeof(bg_fasta_record_t), hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    if (n && seq_off[n]) {
        BG_HIP(hipMemcpyAsync(seq, d_seq, seq_off[n], hipMemcpyDeviceToHost, st));
        BG_HIP(hipStreamSynchronize(st));
    }
    return BG_OK;
}

// sizes and refusals shared by the two flavours of the builder, from the layout's totals
static int fa_ref_admit(uint64_t sum_len1, uint64_t names_total, uint32_t flags, const void* text_out, uint64_t text_cap, const void* contigs,
                        const void* names, uint64_t names_cap, uint64_t* n_t, uint64_t* n_text, uint64_t* names_bytes, bool* sizing) {
    *n_t = (flags & BG_FASTA_REF_FMD) ? sum_len1 - 1 : sum_len1;
    *n_text = (flags & BG_FASTA_REF_FMD) ? 2 * *n_t + 2 : sum_len1;
    *names_bytes = names_total;
    *sizing = !text_out && text_cap == 0;
    if (*sizing) return BG_OK;
    if (!text_out || !contigs || (names_total && !names)) return BG_ERR_INVALID_ARG;
    if (text_cap < *n_text || names_cap < names_total) return BG_ERR_OPS_CAP;
    return BG_OK;
}

extern "C" int bg_fasta_reference_dev(bg_ctx* ctx, uint64_t n_records, const bg_fasta_record_t* d_recs, const uint8_t* d_fasta_text,
                                      const uint8_t* d_seq, uint32_t flags, uint8_t* d_text_out, uint64_t text_cap, bg_sam_contig_t* d_contigs,
                                      char* d_names, uint64_t names_cap, uint64_t* n_text, uint64_t* names_bytes, uint64_t* first_bad,
                                      void* stream) {
    if (!ctx || !n_text || !names_bytes || !first_bad) return BG_ERR_INVALID_ARG;
    *n_text = 0;
    *names_bytes = 0;
    *first_bad = kFaNone;
    if (n_records == 0 || (flags & ~(uint32_t)(BG_FASTA_REF_FMD | BG_FASTA_REF_UPPER)) || !d_recs || !d_fasta_text || !d_seq) return BG_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    bg_scratch_guard guard(ctx, st);
    BG_HIP(hipSetDevice(ctx->device));
    int rc;
    uint64_t *d_starts, *d_name_off, *d_bad;
    if ((rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_starts = cv.take<uint64_t>(n_records + 1), d_name_off = cv.take<uint64_t>(n_records + 1);
        d_bad = cv.take<uint64_t>(1);
    }))) return rc;
    BG_HIP(hipMemcpyAsync(d_bad, first_bad, 8, hipMemcpyHostToDevice, st));
    fa_ref_layout_kernel<<<dim3(1), dim3(1024), 0, st>>>(d_recs, n_records, d_starts, d_name_off, (unsigned long long*)d_bad);
    BG_HIP(hipGetLastError());
    uint64_t sum_len1 = 0, names_total = 0;
    BG_HIP(hipMemcpyAsync(&sum_len1, d_starts + n_records, 8, hipMemcpyDeviceToHost, st));
    BG_HIP(hipMemcpyAsync(&names_total, d_name_off + n_records, 8, hipMemcpyDeviceToHost, st));
    BG_HIP(hipMemcpyAsync(first_bad, d_bad, 8, hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    if (*first_bad != kFaNone) return BG_ERR_INVALID_ARG;  // (an empty name, or maybe '$' in a sequence)
    uint64_t n_t = 0;
    bool sizing = false;
    if ((rc = fa_ref_admit(sum_len1, names_total, flags, d_text_out, text_cap, d_contigs, d_names, names_cap, &n_t, n_text, names_bytes, &sizing)) || sizing)
        return rc;
    fa_ref_contigs_kernel<<<dim3((uint32_t)((n_records + 255) / 256)), dim3(256), 0, st>>>(d_recs, n_records, d_fasta_text, d_starts, d_name_off,
                                                                                           d_contigs, d_names);
    const uint64_t n_vec = (*n_text + 15) / 16;
    fa_ref_text_kernel<<<dim3((uint32_t)((n_vec + 255) / 256)), dim3(256), 0, st>>>(d_recs, n_records, d_seq, d_starts, n_t, *n_text,
                                                                                    (flags & BG_FASTA_REF_UPPER) ? 1 : 0, d_text_out);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

// host flavour: plain loops over the caller's buffers, no GPU (ctx may be null)
extern "C" int bg_fasta_reference(bg_ctx* ctx, uint64_t n_records, const bg_fasta_record_t* recs, const uint8_t* fasta_text, const uint8_t* seq,
                                  uint32_t flags, uint8_t* text_out, uint64_t text_cap, bg_sam_contig_t* contigs, char* names, uint64_t names_cap,
                                  uint64_t* n_text, uint64_t* names_bytes, uint64_t* first_bad) {
    (void)ctx;
    if (!n_text || !names_bytes || !first_bad) return BG_ERR_INVALID_ARG;
    *n_text = 0;
    *names_bytes = 0;
    *first_bad = kFaNone;
    if (n_records == 0 || (flags & ~(uint32_t)(BG_FASTA_REF_FMD | BG_FASTA_REF_UPPER)) || !recs || !fasta_text || !seq) return BG_ERR_INVALID_ARG;
    uint64_t sum_len1 = 0, names_total = 0;
    for (uint64_t i = 0; i < n_records; i++) {
        if (recs[i].check != BG_FACHECK_OK) {
            *first_bad = i;
            return BG_ERR_INVALID_ARG;
        }
        sum_len1 += recs[i].seq_len + 1;
        names_total += recs[i].id_len;
    }
    uint64_t n_t = 0;
    bool sizing = false;
    int rc;
    if ((rc = fa_ref_admit(sum_len1, names_total, flags, text_out, text_cap, contigs, names, names_cap, &n_t, n_text, names_bytes, &sizing)) || sizing)
        return rc;
    const bool fmd = (flags & BG_FASTA_REF_FMD) != 0, upper = (flags & BG_FASTA_REF_UPPER) != 0;
    uint64_t o = 0, no = 0;
    for (uint64_t i = 0; i < n_records; i++) {
        const bg_fasta_record_t& r = recs[i];
        bg_sam_contig_t c = {};
        c.start = o;
        c.len = r.seq_len;
        c.name_off = no;
        c.name_len = r.id_len;
        contigs[i] = c;
        memcpy(names + no, fasta_text + r.id_off, r.id_len);
        no += r.id_len;
        for (uint64_t j = 0; j < r.seq_len; j++) {
            uint8_t b = seq[r.seq_off + j];
            if (upper && b >= 'a' && b <= 'z') b -= 32;
            text_out[o + j] = b;
        }
        o += r.seq_len;
        if (o < n_t || !fmd) text_out[o++] = '$';
    }
    if (fmd) {  // T $ R $ with R = dna::revcomp(T)
        constexpr ComplementTable comp = make_complement();
        text_out[n_t] = '$';
        for (uint64_t j = 0; j < n_t; j++) text_out[2 * n_t - j] = comp.v[text_out[j]];
        text_out[2 * n_t + 1] = '$';
    }
    return BG_OK;
}
