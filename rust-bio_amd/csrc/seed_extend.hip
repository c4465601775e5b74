// Seed-and-extend read mapping behind the C ABI (bg_seed_extend_batch[_dev]; BASELINE configs[4]).
//
// rust-bio has no read mapper: its callers compose one out of three calls
// (/root/reference/src/lib.rs:129-165, benches/fmindex.rs:20-38):
//     FMIndex::backward_search(seed)        fmindex.rs:144-208      K5 (fm_index.hip), the seed windows read in place
//     Interval::occ(&suffix_array)          fmindex.rs:75-79        K6 (sa_locate.hip), raw or sampled suffix array
//     Aligner::semiglobal(read, window)     pairwise/mod.rs:954     K1p / K1 + K2 (sw_*.hip)
// This file is the glue between them, all of it on the device: which seeds vote, hit -> proposed read start, the
// per-read sort + dedup of the proposals, the gather of the (read, window) pairs the aligner consumes, and the
// best-hit reduction that hands back one alignment (with its operations) per read.  Definition of the
// composition: include/biogpu.h (the tests hold a CPU statement of the same thing).
//
// Every entry point describes its call in one SeedCall (absent outputs and mode parameters are null) and hands it to se_run,
// which cuts it into passes; a pass is the four functions below, in this order, on the named buffers of bg_seed_scratch.
// Per pass (S = seed slots per read; the stages run on "virtual reads": each read as it is, or its revcomp, or both, the
// read followed by its revcomp):
//   se_candidates
//   S0 strands          one wavefront per read: read + revcomp -> scratch (virtual reads other than the reads themselves)
//   S1 K5<SEEDS>        n_reads * S backward searches                                  -> tag, lower, upper
//   S2 votes            cnt[q] = interval size if Complete and 1 <= size <= max_occ     -> scan -> hit offsets
//      (the total and the flag word are the FIRST host round trip)
//   S3 K6               Interval::occ of every voting interval                          -> text positions
//   S4 propose          one wavefront per read: s = pos - seed offset, sort, dedup      -> per-read candidate lists
//      (scan of the per-read candidate / x-byte / y-byte counts; the three totals are the SECOND host round trip)
//      SMEM mode (SeedCall::smem, seed_smem.hip) instead of S1, S2, S4: a length check with a host round trip of its own, S1' K7
//      over the caller's reads, S2' votes of the record slots, S4' one wavefront per caller read proposes for both strands
//      tiered mode (SeedCall::tiered, seed_tiered.hip), tier 1: S1 on the caller's reads, S1" the windows as records, then S2', S4'
//   se_align
//   S5 gather           (read, text window) pairs, offsets                              -> x, x_off, y, y_off
//   S6 align            Aligner::semiglobal on every candidate (bg_align_batch_dev)      -> records + operations
//   se_reduce           on the pass view of seed_pass.h (SeedPass, SeedOut), by mode:
//   S7 best             per read: highest score, smallest start among equals           -> bg_seed_hit_t + its ops
//      pair mode        per pair of interleaved mates the best proper FR combination of their candidates, or each mate's
//                       own best -> two bg_seed_hit_t + their ops, bg_pair_hit_t (seed_pairs.hip)
//      pairs-mapq mode  pair mode plus a bg_multi_hit_t per mate, its MAPQ judged against the pair (seed_pairq.hip)
//      multi mode       per read up to K loci that do not touch, in rank order -> K bg_seed_hit_t + their ops, bg_multi_hit_t
//                       with the runner-up's score and MAPQ (seed_multi.hip)
//   se_rescue           rescue modes, instead of se_reduce: (pairs-mapq records of every pair,) R1 plan, one more host
//                       round trip, R2 gather, R3 align, R4 pick (seed_rescue.hip), (records of the rescued pairs,
//                       seed_rescueq.hip)
//   se_reseed           tiered mode, after se_reduce: T1 select, one more host round trip, T2 gather, the SMEM mode's pass on the
//                       re-seeded reads into scratch slots (tier 2), T3 merge (seed_tiered.hip)
// The rules the reduction kernels share are device functions in seed_rule.h, seed_pair_rule.h and seed_rescue_rule.h.
#include <algorithm>

#include "dna_complement.h"
#include "seed_rule.h"

// The pass scratch: one growing device buffer per name (bg_reserve), kept by the context between calls.
enum SeedBuf {
    kTag, kLower, kUpper,  // S1: per seed slot
    kVotes,                // S1 writes the seeds' matched lengths here (not read), S2 the votes over them
    kHitOff,               // S2: scan of the votes
    kScanPartials,         // bg_scan_u32's own scratch, every scan of a pass
    kFlags,                // 64 bytes: bit 0 a seed out of the alphabet, bit 1 a read longer than max_read_len, bit 2 (SMEM mode) a
                           // read with more than max_smems records
    kPos,                  // S3: text positions; S4 leaves each read's candidate starts at the front of its slice
    kPerReadCounts,        // S4: n_cand | n_hits | x_bytes | y_bytes per virtual read
    kPerReadOffsets,       // their scans: coff | xoff | yoff
    kX, kY, kCandOff,      // S5: the aligner's input; kCandOff: x_off | y_off per candidate
    kWLo,                  // S5: the window's first text offset per candidate
    kAln, kCandOps,        // S6: the candidates' alignments and operations
    kVreads,               // S0: voff | the virtual reads' bytes
    kRescuePlan,           // R1: plan entries
    kPerPairCounts,        // R1: own_sum | n_res | x_bytes | y_bytes per pair
    kPerPairOffsets,       // their scans: roff | xoff | yoff
    kRescueX, kRescueY, kRescueOff, kRescueAln, kRescueOps,  // R2, R3: as kX .. kCandOps, for the rescue alignments
    kRescuedCount,         // 64 bytes: the call's rescued pairs (totals[3])
    kSmemCount, kSmemRec,  // S1': K7's count per caller read and its max_smems records of six uint64 (S1": the window records)
    kStartOff,             // S4': where each virtual read's kept starts begin in kPos
    kReseedCounts,         // T1: flag | bytes per read of the pass
    kReseedOffsets,        // their scans: compact index | byte offset
    kReseedReads, kReseedReadOff, kReseedMap,  // T2: the re-seeded reads back to back, their offsets, compact index -> read of the pass
    kTier1Strand,          // tier 1's strand per read of the call, where the caller has no strand array
    kTier2Hits, kTier2Strand, kTier2Ops,  // tier 2's answers: one slot per re-seeded read of the pass
    kSeedBufs
};
struct bg_seed_scratch {
    void* p[kSeedBufs] = {};
    size_t cap[kSeedBufs] = {};
    uint64_t* h_tot = nullptr;  // pinned: totals read back in the host round trips of a pass
};
void bg_seed_scratch_free(bg_seed_scratch* s) {
    if (!s) return;
    for (void* q : s->p) hipFree(q);
    if (s->h_tot) hipHostFree(s->h_tot);
    delete s;
}

namespace {

using namespace bgseed;

constexpr uint32_t kMaxProposals = kMaxCand;  // seed slots x max_occ per read (sorted in LDS by one wavefront)
// proposals are sorted as uint32 on an index with 32-bit positions and as uint64 on one with 64-bit positions (round 6:
// the kernels below are templates over that type; ~P(0) marks a dropped proposal)
struct SeedPrm {
    uint32_t S, stride, seed_len, max_occ, pad;
    uint64_t n_text;  // text length without the final sentinel
};

// S2: votes of every seed slot
__global__ __launch_bounds__(256) void se_votes_kernel(uint64_t n_q, const uint8_t* __restrict__ tag, const uint64_t* __restrict__ lower,
                                                       const uint64_t* __restrict__ upper, uint32_t max_occ, uint32_t* __restrict__ cnt,
                                                       uint32_t* __restrict__ panics) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    uint32_t c = 0;
    if (tag[q] == BG_FM_PANIC) atomicOr(panics, 1u);  // the seed reached a byte outside the alphabet: fmindex.rs:229 panics
    if (tag[q] == BG_FM_COMPLETE) {
        const uint64_t sz = upper[q] - lower[q];
        if (sz >= 1 && sz <= max_occ) c = (uint32_t)sz;
    }
    cnt[q] = c;
}

// S4: one wavefront per read.  The read's hits are pos[hoff[r * S] .. hoff[(r + 1) * S)), grouped by seed slot.  Every
// hit proposes s = p - k * stride (dropped if negative or >= n_text); the proposals are sorted, merged (equal ones, and those
// within pad / 2 of the last start kept), and written back over the read's own slice of `pos`; per read: candidates, hits,
// y bytes, x bytes.
template <typename T>
__global__ __launch_bounds__(64) void se_propose_kernel(SeedPrm prm, uint64_t n_reads, const uint64_t* __restrict__ read_off,
                                                        const uint64_t* __restrict__ hoff, uint64_t* __restrict__ pos,
                                                        uint32_t* __restrict__ n_cand, uint32_t* __restrict__ n_hits,
                                                        uint32_t* __restrict__ x_bytes, uint32_t* __restrict__ y_bytes) {
    constexpr T kNoStart = ~(T)0;
    __shared__ T s_val[kMaxProposals];
    __shared__ uint64_t s_off[65];
    const uint64_t r = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    if (r >= n_reads) return;
    const uint32_t L = (uint32_t)(read_off[r + 1] - read_off[r]);
    for (uint32_t k = lane; k <= prm.S; k += 64) s_off[k] = hoff[r * prm.S + k];  // S <= 64 (checked by the host)
    __syncthreads();
    const uint64_t h0 = s_off[0];
    const uint32_t nh = (uint32_t)(s_off[prm.S] - h0);
    uint32_t n_unique = 0;
    if (nh) {
        uint32_t P = 64;
        while (P < nh) P <<= 1;
        auto proposal = [&](uint32_t i) -> T {
            T v = kNoStart;
            if (i < nh) {
                uint32_t k = 0;  // the seed slot of hit i: last k with s_off[k] - h0 <= i
                while (k + 1 < prm.S && s_off[k + 1] - h0 <= i) k++;
                const uint64_t p = pos[h0 + i];
                const uint64_t o = (uint64_t)k * prm.stride;
                if (p >= o && p - o < prm.n_text) v = (T)(p - o);  // also drops BG_SA_NONE / BG_SA_PANIC
            }
            return v;
        };
        if (nh <= 64) {
            // the usual read (a handful of hits): every lane finds its proposal's rank among the wavefront's by looking at each
            // of the nh values once (a broadcast per value) — no LDS passes, no barriers (the bitonic network below takes 21)
            const T v = proposal(lane);
            uint32_t rank = 0;
            for (uint32_t j = 0; j < nh; j++) {
                T u;
                if constexpr (sizeof(T) == 8)
                    u = (T)((uint64_t)(uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), (int)j) << 32 | (uint32_t)__shfl((int)(uint32_t)v, (int)j));
                else
                    u = (T)(uint32_t)__shfl((int)(uint32_t)v, (int)j);
                rank += (u < v || (u == v && j < lane)) ? 1u : 0u;
            }
            // (lanes >= nh hold kNoStart, the largest value: their ranks are nh .. 63 in lane order)
            s_val[lane < nh ? rank : lane] = v;
            __syncthreads();
        } else {
        for (uint32_t i = lane; i < P; i += 64) s_val[i] = proposal(i);
        __syncthreads();
        // bitonic sort of P values by the 64 lanes
        for (uint32_t k2 = 2; k2 <= P; k2 <<= 1) {
            for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
                for (uint32_t i = lane; i < P; i += 64) {
                    const uint32_t ixj = i ^ j;
                    if (ixj > i) {
                        const T a = s_val[i], b = s_val[ixj];
                        const bool up = (i & k2) == 0;
                        if ((a > b) == up) {
                            s_val[i] = b;
                            s_val[ixj] = a;
                        }
                    }
                }
                __syncthreads();
            }
        }
        }
        // merge equal proposals (compacted in place: a value never moves up, and a step reads before it writes) ...
        uint32_t base = 0;
        for (uint32_t b0 = 0; b0 < P; b0 += 64) {
            const uint32_t i = b0 + lane;
            const T v = s_val[i];
            const bool keep = v != kNoStart && (i == 0 || s_val[i - 1] != v);
            const uint64_t m = __ballot(keep);
            if (keep) s_val[base + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = v;
            base += (uint32_t)__popcll(m);
        }
        __syncthreads();
        // ... and starts within pad / 2 of the last one kept (the seeds either side of an indel propose the same locus a few
        // bases apart: its window holds both alignments) — in order, so a run of proposals a few bases apart each (a tandem
        // repeat) keeps a start every pad / 2 + 1 bases; the kept starts go back over the read's own slots of `pos`
        if (lane == 0) {
            const T merge = (T)(prm.pad / 2);
            uint32_t kept = 0;
            T last = 0;
            for (uint32_t i = 0; i < base; i++) {
                const T v = s_val[i];
                if (kept == 0 || v - last > merge) {
                    pos[h0 + kept++] = v;
                    last = v;
                }
            }
            s_off[0] = kept;  // (s_off is not read again)
        }
        __syncthreads();
        n_unique = (uint32_t)s_off[0];
    }
    // window bytes of this read's candidates (second pass: the starts are final now)
    __syncthreads();
    uint32_t yl = 0;
    for (uint32_t c = lane; c < n_unique; c += 64) {
        const uint64_t v = pos[h0 + c];
        const uint64_t lo = v > prm.pad ? v - prm.pad : 0u;
        const uint64_t hi = min(prm.n_text, v + L + prm.pad);
        yl += (uint32_t)(hi - lo);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) yl += (uint32_t)__shfl_xor((int)yl, o);
    if (lane == 0) {
        n_cand[r] = n_unique;
        n_hits[r] = nh;
        x_bytes[r] = n_unique * L;
        y_bytes[r] = yl;
    }
}

// S5: one wavefront per read: the (read, window) pairs of its candidates + their offsets.  The read's starts are pos[soff[r *
// soff_stride] + c]: its hits' first slot where S4 left them (soff = hoff, soff_stride = S), or the array S4' wrote.
__global__ __launch_bounds__(64) void se_gather_kernel(SeedPrm prm, uint64_t n_reads, const uint8_t* __restrict__ reads,
                                                       const uint64_t* __restrict__ read_off, const uint8_t* __restrict__ text,
                                                       const uint64_t* __restrict__ soff, uint32_t soff_stride,
                                                       const uint64_t* __restrict__ pos, const uint64_t* __restrict__ coff,
                                                       const uint64_t* __restrict__ xoff, const uint64_t* __restrict__ yoff,
                                                       uint8_t* __restrict__ x,
                                                       uint64_t* __restrict__ x_off, uint8_t* __restrict__ y, uint64_t* __restrict__ y_off,
                                                       uint64_t* __restrict__ w_lo) {
    const uint64_t r = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    if (r >= n_reads) return;
    const uint64_t c0 = coff[r];
    const uint32_t nc = (uint32_t)(coff[r + 1] - c0);
    if (r + 1 == n_reads && lane == 0) {  // closing offsets
        x_off[coff[n_reads]] = xoff[n_reads];
        y_off[coff[n_reads]] = yoff[n_reads];
    }
    if (!nc) return;
    const uint64_t ro = read_off[r];
    const uint32_t L = (uint32_t)(read_off[r + 1] - ro);
    const uint64_t h0 = soff[r * soff_stride];
    uint64_t yo = yoff[r];
    for (uint32_t c = 0; c < nc; c++) {
        const uint64_t v = pos[h0 + c];
        const uint64_t lo = v > prm.pad ? v - prm.pad : 0u;
        const uint64_t hi = min(prm.n_text, v + L + prm.pad);
        const uint64_t xo = xoff[r] + (uint64_t)c * L;
        if (lane == 0) {
            x_off[c0 + c] = xo;
            y_off[c0 + c] = yo;
            w_lo[c0 + c] = lo;
        }
        for (uint32_t i = lane; i < L; i += 64) x[xo + i] = reads[ro + i];
        for (uint32_t i = lane; i < (uint32_t)(hi - lo); i += 64) y[yo + i] = text[lo + i];
        yo += hi - lo;
    }
}

// bg_revcomp_batch_dev: one wavefront per sequence, four per block
__global__ __launch_bounds__(256) void se_revcomp_kernel(uint64_t n, const uint8_t* __restrict__ in, const uint64_t* __restrict__ off,
                                                         uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(4))) uint8_t s_comp[256];
    load_complement(s_comp);
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const uint64_t o = off[r];
    revcomp_wave(s_comp, in + o, out + o, off[r + 1] - o, threadIdx.x & 63);
}

// S0 of the stranded call: the pass's virtual reads, one wavefront per read of the caller, four per block.  G = 2: virtual
// read 2r is read r, 2r + 1 its revcomp, back to back at 2 (off[r] - off[0]); G = 1: the revcomp alone at off[r] - off[0].
// Offsets relative to the pass's first read, G * nr + 1 of them.  `cap` = G * nr * max_read_len bytes of scratch: a read
// longer than max_read_len (the caller's error) sets bit 1 of *flags, and offsets and bytes stay inside the scratch.
template <int G>
__global__ __launch_bounds__(256) void se_strands_kernel(uint64_t nr, const uint8_t* __restrict__ reads, const uint64_t* __restrict__ read_off,
                                                         uint64_t cap, uint8_t* __restrict__ vreads, uint64_t* __restrict__ voff,
                                                         uint32_t* __restrict__ flags) {
    __shared__ __attribute__((aligned(4))) uint8_t s_comp[256];
    load_complement(s_comp);
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (r >= nr) return;
    const uint64_t base = read_off[0], ro = read_off[r], L = read_off[r + 1] - ro;
    const uint64_t vo = G * (ro - base);
    if (lane == 0) {
        voff[G * r] = min(vo, cap);
        if (G == 2) voff[2 * r + 1] = min(vo + L, cap);
        if (r + 1 == nr) voff[G * nr] = min(G * (read_off[nr] - base), cap);
    }
    if (vo + G * L > cap) {
        if (lane == 0) atomicOr(flags, 2u);
        return;
    }
    if (G == 2)
        for (uint64_t i = lane; i < L; i += 64) vreads[vo + i] = reads[ro + i];
    revcomp_wave(s_comp, reads + ro, vreads + vo + (G - 1) * L, L, lane);
}

// S7: 16 lanes per read: best candidate (highest score, first = smallest start among equals), record + operations.
// Read r0 + r of the call owns slot r0 + r.  Read r's candidates are those of its G virtual reads, coff[G r] .. coff[G r + G):
// with G = 2 the forward strand's come first, so the same key makes it win a tie; with G = 1 every winner is on strand `strand1`.
template <int G>
__global__ __launch_bounds__(256) void se_best_kernel(SeedPass P, SeedOut O, uint8_t strand1) {
    const uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t l16 = threadIdx.x & 15;
    if (r >= P.n) return;  // uniform per group of 16
    const uint64_t c0 = P.coff[G * r];
    const uint32_t nc = (uint32_t)(P.coff[G * r + G] - c0);
    uint64_t best = 0;
    for (uint32_t c = l16; c < nc; c += 16) best = max(best, own_key(P.aln[c0 + c].score, c));
    const uint32_t c = key_cand(max16(best));
    const uint8_t won = !nc ? BG_HIT_NONE : G == 2 ? (c >= P.coff[2 * r + 1] - c0 ? BG_HIT_REVERSE : BG_HIT_FORWARD) : strand1;
    write_cand(P, O, P.r0 + r, l16, c0 + c, won, nc, G == 2 ? P.n_hits[2 * r] + P.n_hits[2 * r + 1] : P.n_hits[r]);
}

}  // namespace

extern "C" int bg_fm_set_text(bg_fm* fm, const uint8_t* text, uint64_t n) {
    if (!fm || !text || n != fm_len(fm)) return BG_ERR_INVALID_ARG;
    BG_HIP(hipSetDevice(fm->ctx->device));
    if (fm->text_owned) hipFree(fm->d_text);
    fm->d_text = nullptr;
    fm->text_owned = false;
    BG_HIP(hipMalloc(&fm->d_text, n));
    fm->text_owned = true;
    if (bg_copy_pieces(fm->d_text, text, n, hipMemcpyHostToDevice, fm->ctx->stream) != hipSuccess || hipStreamSynchronize(fm->ctx->stream) != hipSuccess)
        return BG_ERR_HIP;
    fm->n_text = n - 1;
    fm->bytes += n;
    return BG_OK;
}

extern "C" int bg_fm_set_text_dev(bg_fm* fm, const uint8_t* d_text, uint64_t n) {
    if (!fm || !d_text || n != fm_len(fm)) return BG_ERR_INVALID_ARG;
    if (fm->text_owned) hipFree(fm->d_text);
    fm->d_text = (void*)d_text;
    fm->text_owned = false;
    fm->n_text = n - 1;
    return BG_OK;
}

namespace {

// One call of any flavour: absent outputs and mode parameters are null.
//   strands      0: the caller's reads as they are, no strand array; BG_STRAND_FORWARD: the same, with the strand array;
//                BG_STRAND_REVERSE: the revcomps; BG_STRAND_BOTH: read and revcomp (G = 2 virtual reads per read)
//   pair         pair mode (strands = BG_STRAND_BOTH, n_reads = 2 n_pairs interleaved mates): passes hold whole pairs; `pairs`
//   pairq        with pair: one `multi` record per mate
//   rescue       with pair: `rescued` one byte per pair, `totals` 4 entries (otherwise 2)
//   multi_prm    multi mode: hits / strand / ops hold max_hits slots per read, `multi` one record per read
//   smem         SMEM mode: seeds are the SMEMs of the caller's reads on an FMD index, `prm` is null
//   tiered       tiered mode: `prm` and `smem` are null; tier 1 seeds with tiered->window on the FMD index, tier 2 is an SMEM-mode
//                call of its own on the re-seeded reads (se_reseed); `tier` one byte per read, `totals` 3 entries
struct SeedCall {
    bg_fm* fm = nullptr;
    const bg_scoring_t* sc = nullptr;
    const bg_seed_params_t* prm = nullptr;
    uint32_t strands = 0;
    uint64_t n_reads = 0;
    const uint8_t* reads = nullptr;
    const uint64_t* read_off = nullptr;
    uint32_t max_read_len = 0;
    bg_seed_hit_t* hits = nullptr;
    uint8_t* strand = nullptr;
    uint8_t* ops = nullptr;
    uint64_t ops_stride = 0;
    bg_pair_hit_t* pairs = nullptr;
    bg_multi_hit_t* multi = nullptr;
    uint8_t* rescued = nullptr;
    uint64_t* totals = nullptr;
    const bg_pair_params_t* pair = nullptr;
    const bg_multi_params_t* multi_prm = nullptr;
    const bg_rescue_params_t* rescue = nullptr;
    const bg_pairq_params_t* pairq = nullptr;
    const bg_smem_seed_params_t* smem = nullptr;
    const bg_tiered_seed_params_t* tiered = nullptr;
    uint8_t* tier = nullptr;
    void* stream = nullptr;
    uint32_t pad() const { return tiered ? tiered->window.pad : smem ? smem->pad : prm->pad; }
};

// consecutive arrays out of one scratch buffer
struct Carve {
    uint8_t* at;
    template <typename T>
    T* take(size_t n) {
        T* q = (T*)at;
        at += n * sizeof(T);
        return q;
    }
};

// what a call's passes share
struct SeedRun {
    const SeedCall& call;
    bg_seed_scratch& W;
    bg_ctx* ctx = nullptr;
    hipStream_t st = nullptr;
    SeedPrm prm = {};
    SeedSmemPrm smem = {};  // SMEM and tiered modes: the record slots of a read
    uint32_t G = 1;         // virtual reads per read
    bool virt = false;      // the virtual reads are materialised (S0)
    uint32_t win_max = 0;   // the longest candidate window
    uint32_t rwin_max = 0;  // the longest rescue window
    SeedOut out = {};

    int need(SeedBuf b, size_t bytes) { return bg_reserve(&W.p[b], &W.cap[b], std::max<size_t>(bytes, 64)); }
    template <typename T>
    T* buf(SeedBuf b) const {
        return (T*)W.p[b];
    }
    uint8_t strand1() const { return call.strands == BG_STRAND_REVERSE ? BG_HIT_REVERSE : BG_HIT_FORWARD; }
};

// one pass: reads r0 .. r0 + nr of the call, and what its stages hand on
struct SeedPassRun {
    uint64_t r0, nr, nv, nq;  // caller reads, virtual reads, seed slots
    const uint8_t* vreads;    // the virtual reads and their nv + 1 offsets
    const uint64_t* roff;
    uint64_t* hoff;           // S2
    const uint64_t* soff;     // S4: virtual read v's kept starts begin at pos[soff[v * soff_stride]]
    uint32_t soff_stride;
    uint64_t* pos;            // S3, S4
    uint32_t* n_hits;         // S4: per virtual read, and the scans of its other counts
    SeedXYOff off;
    uint64_t n_sa_rows, C, X, Y;  // the host round trips: suffix-array rows, candidates, their x and y bytes
    SeedPass view;                // S5, S6: what the reduction reads
    uint64_t n_rescue;            // R1: rescue alignments
};

// S0-S4: seeds -> votes -> text positions -> per-read candidate lists.  Two host round trips: the hit total with the flag word
// (sizes the position array), then the candidate / x-byte / y-byte totals (size the aligner's input).
int se_candidates(SeedRun& R, SeedPassRun& p, bool* any_panic, bool* any_truncated) {
    int rc;
    const SeedCall& c = R.call;
    const uint64_t nv = p.nv, nq = p.nq;
    if ((rc = R.need(kTag, nq))) return rc;
    if ((rc = R.need(kLower, nq * 8))) return rc;
    if ((rc = R.need(kUpper, nq * 8))) return rc;
    if ((rc = R.need(kVotes, nq * 4))) return rc;
    if ((rc = R.need(kHitOff, (nq + 1) * 8))) return rc;
    if ((rc = R.need(kScanPartials, bg_scan_sums_words(nq) * 8))) return rc;
    if ((rc = R.need(kFlags, 64))) return rc;
    uint8_t* d_tag = R.buf<uint8_t>(kTag);
    uint64_t *d_lo = R.buf<uint64_t>(kLower), *d_hi = R.buf<uint64_t>(kUpper), *d_sums = R.buf<uint64_t>(kScanPartials);
    uint32_t* d_votes = R.buf<uint32_t>(kVotes);
    uint32_t* d_matched_len = d_votes;  // the search must write them somewhere; S2 overwrites them
    uint32_t* d_flags = R.buf<uint32_t>(kFlags);
    p.hoff = R.buf<uint64_t>(kHitOff);
    BG_HIP(hipMemsetAsync(d_flags, 0, 8, R.st));
    if (c.smem) {
        // K7 sizes its interval lists by max_read_len: a longer read (the caller's error) ends the call before it runs
        if ((rc = bg_seed_smem_lengths_launch(p.nr, c.read_off + p.r0, c.max_read_len, d_flags, R.st))) return rc;
        BG_HIP(hipMemcpyAsync(&R.W.h_tot[4], d_flags, 8, hipMemcpyDeviceToHost, R.st));
        BG_HIP(hipStreamSynchronize(R.st));
        if (R.W.h_tot[4] & kFlagLongRead) return BG_ERR_INVALID_ARG;
    }
    // ---- S0: the virtual reads and their offsets, relative to the pass's first read
    p.vreads = c.reads;
    p.roff = c.read_off + p.r0;
    if (R.virt) {
        const uint64_t cap = nv * (uint64_t)c.max_read_len;
        if ((rc = R.need(kVreads, (nv + 1) * 8 + cap))) return rc;
        Carve v{R.buf<uint8_t>(kVreads)};
        uint64_t* d_voff = v.take<uint64_t>(nv + 1);
        uint8_t* d_vreads = v.take<uint8_t>(cap);
        const dim3 grid((unsigned)((p.nr + 3) / 4)), block(256);
        if (R.G == 2)
            se_strands_kernel<2><<<grid, block, 0, R.st>>>(p.nr, c.reads, p.roff, cap, d_vreads, d_voff, d_flags);
        else
            se_strands_kernel<1><<<grid, block, 0, R.st>>>(p.nr, c.reads, p.roff, cap, d_vreads, d_voff, d_flags);
        BG_HIP(hipGetLastError());
        p.vreads = d_vreads;
        p.roff = d_voff;
    }
    // ---- S1/S2: seeds -> votes -> hit offsets
    const uint64_t* d_rec = nullptr;
    if (c.tiered) {
        // S1, S1", S2': the windows of the pass's caller reads, searched once on the FMD index, as records
        if (!R.prm.S) {  // no window fits in max_read_len: one empty slot per read
            BG_HIP(hipMemsetAsync(d_votes, 0, nq * 4, R.st));
        } else {
            if ((rc = R.need(kSmemCount, p.nr * 4))) return rc;
            if ((rc = R.need(kSmemRec, nq * 6 * 8))) return rc;
            d_rec = R.buf<uint64_t>(kSmemRec);
            if ((rc = bg_fm_search_seeds_dev(c.fm, p.nr, c.reads, c.read_off + p.r0, R.prm.S, R.prm.stride, R.prm.seed_len, d_tag, d_lo, d_hi,
                                             d_matched_len, R.st)))
                return rc;
            if ((rc = bg_seed_tiered_records_launch(p.nr, R.prm.S, R.prm.stride, R.prm.seed_len, c.read_off + p.r0, d_tag, d_lo, d_hi,
                                                    R.buf<uint32_t>(kSmemCount), R.buf<uint64_t>(kSmemRec), d_flags, R.st)))
                return rc;
            if ((rc = bg_seed_smem_votes_launch(nq, R.smem, R.buf<uint32_t>(kSmemCount), d_rec, d_votes, d_lo, d_flags, R.st))) return rc;
        }
    } else if (c.smem) {
        // S1', S2': the SMEMs of the pass's caller reads (not of their revcomps: the index holds both strands)
        if ((rc = R.need(kSmemCount, p.nr * 4))) return rc;
        if ((rc = R.need(kSmemRec, nq * 6 * 8))) return rc;
        d_rec = R.buf<uint64_t>(kSmemRec);
        if ((rc = bg_seed_smem_seeds_launch(c.fm, R.smem, c.smem->min_seed_len, p.nr, c.reads, c.read_off + p.r0, c.max_read_len,
                                            R.buf<uint32_t>(kSmemCount), R.buf<uint64_t>(kSmemRec), d_votes, d_lo, d_flags, R.st)))
            return rc;
    } else if (R.prm.S) {
        if ((rc = bg_fm_search_seeds_dev(c.fm, nv, p.vreads, p.roff, R.prm.S, R.prm.stride, R.prm.seed_len, d_tag, d_lo, d_hi, d_matched_len,
                                         R.st)))
            return rc;
        se_votes_kernel<<<dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, R.st>>>(nq, d_tag, d_lo, d_hi, R.prm.max_occ, d_votes, d_flags);
    } else {
        BG_HIP(hipMemsetAsync(d_votes, 0, nq * 4, R.st));
    }
    if ((rc = bg_scan_u32(d_votes, nq, p.hoff, d_sums, R.st))) return rc;
    BG_HIP(hipMemcpyAsync(&R.W.h_tot[0], p.hoff + nq, 8, hipMemcpyDeviceToHost, R.st));
    BG_HIP(hipMemcpyAsync(&R.W.h_tot[4], d_flags, 8, hipMemcpyDeviceToHost, R.st));
    BG_HIP(hipStreamSynchronize(R.st));  // sizes the position array
    p.n_sa_rows = R.W.h_tot[0];
    if (R.W.h_tot[4] & kFlagPanic) *any_panic = true;
    if (R.W.h_tot[4] & kFlagTruncated) *any_truncated = true;
    if (R.W.h_tot[4] & kFlagLongRead) return BG_ERR_INVALID_ARG;  // a read longer than max_read_len (S0 kept within its scratch)
    // ---- S3: Interval::occ of the voting intervals
    if ((rc = R.need(kPos, p.n_sa_rows * 8))) return rc;
    p.pos = R.buf<uint64_t>(kPos);
    if (p.n_sa_rows && (rc = bg_interval_occ_batch_dev(c.fm, nq, d_lo, p.hoff, p.n_sa_rows, p.pos, R.st))) return rc;
    // ---- S4: proposals -> sorted unique candidates per read, scans of the per-read counts
    if ((rc = R.need(kPerReadCounts, 4 * nv * 4))) return rc;
    if ((rc = R.need(kPerReadOffsets, 3 * (nv + 1) * 8))) return rc;
    Carve counts{R.buf<uint8_t>(kPerReadCounts)}, offsets{R.buf<uint8_t>(kPerReadOffsets)};
    uint32_t* d_nc = counts.take<uint32_t>(nv);
    p.n_hits = counts.take<uint32_t>(nv);
    uint32_t *d_xb = counts.take<uint32_t>(nv), *d_yb = counts.take<uint32_t>(nv);
    uint64_t *d_coff = offsets.take<uint64_t>(nv + 1), *d_xoff = offsets.take<uint64_t>(nv + 1), *d_yoff = offsets.take<uint64_t>(nv + 1);
    p.off = SeedXYOff{d_coff, d_xoff, d_yoff};
    p.soff = p.hoff, p.soff_stride = R.prm.S;
    if (c.smem || c.tiered) {
        if ((rc = R.need(kStartOff, nv * 8))) return rc;
        uint64_t* d_soff = R.buf<uint64_t>(kStartOff);
        p.soff = d_soff, p.soff_stride = 1;
        if ((rc = bg_seed_smem_propose_launch(c.fm->wide, R.smem, p.nr, c.read_off + p.r0, p.hoff, d_rec, p.pos, d_soff, d_nc, p.n_hits, d_xb,
                                              d_yb, R.st)))
            return rc;
    } else if (c.fm->wide)
        se_propose_kernel<uint64_t><<<dim3((unsigned)nv), dim3(64), 0, R.st>>>(R.prm, nv, p.roff, p.hoff, p.pos, d_nc, p.n_hits, d_xb, d_yb);
    else
        se_propose_kernel<uint32_t><<<dim3((unsigned)nv), dim3(64), 0, R.st>>>(R.prm, nv, p.roff, p.hoff, p.pos, d_nc, p.n_hits, d_xb, d_yb);
    BG_HIP(hipGetLastError());
    if ((rc = bg_scan_u32(d_nc, nv, d_coff, d_sums, R.st))) return rc;
    if ((rc = bg_scan_u32(d_xb, nv, d_xoff, d_sums, R.st))) return rc;
    if ((rc = bg_scan_u32(d_yb, nv, d_yoff, d_sums, R.st))) return rc;
    BG_HIP(hipMemcpyAsync(&R.W.h_tot[1], d_coff + nv, 8, hipMemcpyDeviceToHost, R.st));
    BG_HIP(hipMemcpyAsync(&R.W.h_tot[2], d_xoff + nv, 8, hipMemcpyDeviceToHost, R.st));
    BG_HIP(hipMemcpyAsync(&R.W.h_tot[3], d_yoff + nv, 8, hipMemcpyDeviceToHost, R.st));
    BG_HIP(hipStreamSynchronize(R.st));  // sizes the candidate pairs
    p.C = R.W.h_tot[1], p.X = R.W.h_tot[2], p.Y = R.W.h_tot[3];
    return BG_OK;
}

// S5-S6: the (read, window) pairs of every candidate, and Aligner::semiglobal on them -> the pass view
int se_align(SeedRun& R, SeedPassRun& p) {
    int rc;
    const SeedCall& c = R.call;
    const uint64_t cstride = c.ops ? (uint64_t)c.max_read_len + R.win_max + 4 : 0;
    if ((rc = R.need(kX, p.X))) return rc;
    if ((rc = R.need(kY, p.Y))) return rc;
    if ((rc = R.need(kCandOff, 2 * (p.C + 1) * 8))) return rc;
    if ((rc = R.need(kWLo, p.C * 8))) return rc;
    if ((rc = R.need(kAln, p.C * sizeof(bg_alignment_t)))) return rc;
    if ((rc = R.need(kCandOps, p.C * cstride))) return rc;
    Carve o{R.buf<uint8_t>(kCandOff)};
    const SeedPairsXY xy{R.buf<uint8_t>(kX), o.take<uint64_t>(p.C + 1), R.buf<uint8_t>(kY), o.take<uint64_t>(p.C + 1)};
    uint64_t* d_wlo = R.buf<uint64_t>(kWLo);
    bg_alignment_t* d_aln = R.buf<bg_alignment_t>(kAln);
    uint8_t* d_cops = c.ops ? R.buf<uint8_t>(kCandOps) : nullptr;
    se_gather_kernel<<<dim3((unsigned)p.nv), dim3(64), 0, R.st>>>(R.prm, p.nv, p.vreads, p.roff, (const uint8_t*)c.fm->d_text, p.soff, p.soff_stride,
                                                                  p.pos, p.off.roff, p.off.xoff, p.off.yoff, xy.x, xy.x_off, xy.y, xy.y_off, d_wlo);
    BG_HIP(hipGetLastError());
    if (p.C && (rc = bg_align_batch_dev_hint(R.ctx, c.sc, BG_MODE_SEMIGLOBAL, p.C, xy.x, xy.x_off, xy.y, xy.y_off, c.max_read_len, R.win_max,
                                             d_aln, d_cops, cstride, R.st, -1)))
        return rc;
    p.view = SeedPass{p.r0, c.pair ? p.nr / 2 : p.nr, p.off.roff, p.n_hits, d_aln, d_cops, d_wlo, p.roff};
    return BG_OK;
}

// S7: one answer per read, per pair in the pair modes
int se_reduce(SeedRun& R, SeedPassRun& p) {
    const SeedCall& c = R.call;
    if (c.pairq) return bg_seed_pairq_launch(p.view, R.out, c.pair, c.pairq, R.st);
    if (c.pair) return bg_seed_pairs_launch(p.view, R.out, c.pair, R.st);
    if (c.multi_prm) return bg_seed_multi_launch(p.view, R.out, c.multi_prm, R.G, R.strand1(), R.st);
    const dim3 grid((unsigned)((p.nr * 16 + 255) / 256));
    if (R.G == 2)
        se_best_kernel<2><<<grid, dim3(256), 0, R.st>>>(p.view, R.out, 0);
    else
        se_best_kernel<1><<<grid, dim3(256), 0, R.st>>>(p.view, R.out, R.strand1());
    BG_HIP(hipGetLastError());
    return BG_OK;
}

// The rescue modes' reduction: R1-R4 of seed_rescue.hip.  With pairq, se_pairq_kernel writes every pair's records before R1,
// which rewrites the same hits, and se_rescue_mapq_kernel rewrites the records of the rescued pairs after R4.  A pass without
// a rescue alignment ends after R1's read-back, the one extra host round trip.
int se_rescue(SeedRun& R, SeedPassRun& p) {
    int rc;
    const SeedCall& c = R.call;
    const uint64_t np = p.view.n;
    const uint64_t rstride = c.ops ? (uint64_t)c.max_read_len + R.rwin_max + 4 : 0;
    if ((rc = R.need(kRescuePlan, bg_seed_rescue_plan_bytes(np)))) return rc;
    if ((rc = R.need(kPerPairCounts, np * 8 + 3 * np * 4))) return rc;
    if ((rc = R.need(kPerPairOffsets, 3 * (np + 1) * 8))) return rc;
    Carve counts{R.buf<uint8_t>(kPerPairCounts)}, offsets{R.buf<uint8_t>(kPerPairOffsets)};
    SeedRescuePlan plan;
    plan.plan = R.buf<void>(kRescuePlan);
    plan.own_sum = counts.take<int64_t>(np);
    plan.n_res = counts.take<uint32_t>(np), plan.x_bytes = counts.take<uint32_t>(np), plan.y_bytes = counts.take<uint32_t>(np);
    uint64_t *d_roff = offsets.take<uint64_t>(np + 1), *d_rxoff = offsets.take<uint64_t>(np + 1), *d_ryoff = offsets.take<uint64_t>(np + 1);
    uint64_t* d_sums = R.buf<uint64_t>(kScanPartials);
    if (c.pairq && (rc = bg_seed_pairq_launch(p.view, R.out, c.pair, c.pairq, R.st))) return rc;
    // ---- R1: the paired call's answer for every pair + the rescue plan of those without a proper combination
    if ((rc = bg_seed_rescue_plan_launch(p.view, R.out, c.pair, c.rescue, R.prm.n_text, plan, R.st))) return rc;
    if ((rc = bg_scan_u32(plan.n_res, np, d_roff, d_sums, R.st))) return rc;
    if ((rc = bg_scan_u32(plan.x_bytes, np, d_rxoff, d_sums, R.st))) return rc;
    if ((rc = bg_scan_u32(plan.y_bytes, np, d_ryoff, d_sums, R.st))) return rc;
    BG_HIP(hipMemcpyAsync(&R.W.h_tot[5], d_roff + np, 8, hipMemcpyDeviceToHost, R.st));
    BG_HIP(hipMemcpyAsync(&R.W.h_tot[6], d_rxoff + np, 8, hipMemcpyDeviceToHost, R.st));
    BG_HIP(hipMemcpyAsync(&R.W.h_tot[7], d_ryoff + np, 8, hipMemcpyDeviceToHost, R.st));
    BG_HIP(hipStreamSynchronize(R.st));  // sizes the rescue pairs
    const uint64_t RC = R.W.h_tot[5], RX = R.W.h_tot[6], RY = R.W.h_tot[7];
    p.n_rescue = RC;
    if (!RC) return BG_OK;
    // ---- R2: the (other mate, insert window) pairs
    if ((rc = R.need(kRescueX, RX))) return rc;
    if ((rc = R.need(kRescueY, RY))) return rc;
    if ((rc = R.need(kRescueOff, 2 * (RC + 1) * 8))) return rc;
    if ((rc = R.need(kRescueAln, RC * sizeof(bg_alignment_t)))) return rc;
    if ((rc = R.need(kRescueOps, RC * rstride))) return rc;
    Carve o{R.buf<uint8_t>(kRescueOff)};
    const SeedPairsXY xy{R.buf<uint8_t>(kRescueX), o.take<uint64_t>(RC + 1), R.buf<uint8_t>(kRescueY), o.take<uint64_t>(RC + 1)};
    bg_alignment_t* d_raln = R.buf<bg_alignment_t>(kRescueAln);
    uint8_t* d_rops = c.ops ? R.buf<uint8_t>(kRescueOps) : nullptr;
    if ((rc = bg_seed_rescue_gather_launch(p.view, p.vreads, (const uint8_t*)c.fm->d_text, plan.plan, SeedXYOff{d_roff, d_rxoff, d_ryoff}, xy,
                                           R.st)))
        return rc;
    // ---- R3: Aligner::semiglobal on every rescue pair
    if ((rc = bg_align_batch_dev_hint(R.ctx, c.sc, BG_MODE_SEMIGLOBAL, RC, xy.x, xy.x_off, xy.y, xy.y_off, c.max_read_len, R.rwin_max, d_raln,
                                      d_rops, rstride, R.st, -1)))
        return rc;
    const SeedRescueAln res{d_roff, d_raln, d_rops};
    // ---- R4: the rescued pairs
    if ((rc = bg_seed_rescue_pick_launch(p.view, R.out, c.pair, c.rescue, plan, res, R.st))) return rc;
    // ---- the records of the rescued pairs (the plan and the rescue alignments are still live)
    if (c.pairq && (rc = bg_seed_rescueq_launch(p.view, R.out, c.pair, c.rescue, c.pairq, plan.plan, res, R.st))) return rc;
    return BG_OK;
}

// The seeds of a call in its mode: the slots of a read (prm.S) and what the candidate stages need to know about them.
int se_seed_params(const SeedCall& c, uint64_t n_index, SeedPrm* prm_out, SeedSmemPrm* smem_out) {
    SeedPrm prm = {};
    SeedSmemPrm smem = {};
    if (c.smem) {  // the slots of a read are its max_smems records; the text the windows are cut from is T, the first half
        smem = SeedSmemPrm{c.smem->max_smems, c.smem->max_occ, c.smem->pad, c.strands, (n_index - 2) / 2};
        prm.S = smem.M, prm.max_occ = smem.max_occ, prm.pad = smem.pad, prm.n_text = smem.n_t;
    } else {
        const bg_seed_params_t& w = c.tiered ? c.tiered->window : *c.prm;
        prm.S = c.max_read_len >= w.seed_len ? (c.max_read_len - w.seed_len) / w.stride + 1 : 0;
        prm.stride = w.stride;
        prm.seed_len = w.seed_len;
        prm.max_occ = w.max_occ;
        prm.pad = w.pad;
        prm.n_text = c.fm->n_text;
        if (prm.S > 64 || (uint64_t)prm.S * prm.max_occ > kMaxProposals) return BG_ERR_UNSUPPORTED;
        if (c.tiered) {  // tier 1: the slots of a read are its windows as records, on T$R$ as in SMEM mode
            smem = SeedSmemPrm{prm.S, w.max_occ, w.pad, c.strands, (n_index - 2) / 2};
            prm.n_text = smem.n_t;
        }
    }
    *prm_out = prm, *smem_out = smem;
    return BG_OK;
}

// one pass of a call: its candidates, their alignments, the answers
int se_pass(SeedRun& R, SeedPassRun& p, bool* any_panic, bool* any_truncated) {
    int rc;
    if ((rc = se_candidates(R, p, any_panic, any_truncated))) return rc;
    if ((rc = se_align(R, p))) return rc;
    return R.call.rescue ? se_rescue(R, p) : se_reduce(R, p);
}

// Tiered mode, after tier 1's pass has answered reads r0 .. r0 + nr: T1 select, the re-seeded count and bytes (one host round
// trip; count 0 ends here), T2 gather, tier 2 — an SMEM-mode pass of its own over the compact reads, into scratch slots —, T3 merge.
// strand1: tier 1's strand per read of the call.  Adds tier 2's rows, candidates and reads to the three counters.
int se_reseed(SeedRun& R, const SeedPassRun& p, uint8_t* strand1, uint64_t n_index, uint64_t* rows, uint64_t* cand, uint64_t* reseeded,
              bool* any_panic, bool* any_truncated) {
    int rc;
    const SeedCall& c = R.call;
    const uint64_t nr = p.nr;
    if ((rc = R.need(kReseedCounts, 2 * nr * 4))) return rc;
    if ((rc = R.need(kReseedOffsets, 2 * (nr + 1) * 8))) return rc;
    if ((rc = R.need(kScanPartials, bg_scan_sums_words(nr) * 8))) return rc;
    Carve counts{R.buf<uint8_t>(kReseedCounts)}, offsets{R.buf<uint8_t>(kReseedOffsets)};
    uint32_t *d_flag = counts.take<uint32_t>(nr), *d_bytes = counts.take<uint32_t>(nr);
    uint64_t *d_idx = offsets.take<uint64_t>(nr + 1), *d_boff = offsets.take<uint64_t>(nr + 1);
    uint64_t* d_sums = R.buf<uint64_t>(kScanPartials);
    if ((rc = bg_seed_tiered_select_launch(nr, p.r0, c.hits, c.read_off, c.tiered->reseed_below, d_flag, d_bytes, c.tier, R.st))) return rc;
    if ((rc = bg_scan_u32(d_flag, nr, d_idx, d_sums, R.st))) return rc;
    if ((rc = bg_scan_u32(d_bytes, nr, d_boff, d_sums, R.st))) return rc;
    BG_HIP(hipMemcpyAsync(&R.W.h_tot[5], d_idx + nr, 8, hipMemcpyDeviceToHost, R.st));
    BG_HIP(hipMemcpyAsync(&R.W.h_tot[6], d_boff + nr, 8, hipMemcpyDeviceToHost, R.st));
    BG_HIP(hipStreamSynchronize(R.st));  // sizes tier 2
    const uint64_t n2 = R.W.h_tot[5], n_bytes = R.W.h_tot[6];
    if (!n2) return BG_OK;
    // ---- T2: the re-seeded reads, back to back
    if ((rc = R.need(kReseedReads, n_bytes))) return rc;
    if ((rc = R.need(kReseedReadOff, (n2 + 1) * 8))) return rc;
    if ((rc = R.need(kReseedMap, n2 * 4))) return rc;
    if ((rc = R.need(kTier2Hits, n2 * sizeof(bg_seed_hit_t)))) return rc;
    if ((rc = R.need(kTier2Strand, n2))) return rc;
    if ((rc = R.need(kTier2Ops, c.ops ? n2 * c.ops_stride : 0))) return rc;
    uint32_t* d_map = R.buf<uint32_t>(kReseedMap);
    if ((rc = bg_seed_tiered_gather_launch(nr, p.r0, c.reads, c.read_off, d_flag, d_idx, d_boff, R.buf<uint8_t>(kReseedReads),
                                           R.buf<uint64_t>(kReseedReadOff), d_map, R.st)))
        return rc;
    // ---- tier 2: the SMEM call's pass on them
    SeedCall c2 = c;
    c2.tiered = nullptr, c2.smem = &c.tiered->smem, c2.tier = nullptr, c2.totals = nullptr;
    c2.n_reads = n2, c2.reads = R.buf<uint8_t>(kReseedReads), c2.read_off = R.buf<uint64_t>(kReseedReadOff);
    c2.hits = R.buf<bg_seed_hit_t>(kTier2Hits), c2.strand = R.buf<uint8_t>(kTier2Strand), c2.ops = c.ops ? R.buf<uint8_t>(kTier2Ops) : nullptr;
    SeedRun R2{c2, R.W};
    R2.ctx = R.ctx, R2.st = R.st, R2.G = R.G, R2.virt = R.virt, R2.win_max = R.win_max;
    if ((rc = se_seed_params(c2, n_index, &R2.prm, &R2.smem))) return rc;
    R2.out.hits = c2.hits, R2.out.ops = c2.ops, R2.out.ops_stride = c2.ops_stride, R2.out.strand = c2.strand;
    SeedPassRun p2{};
    p2.nr = n2;
    p2.nv = R.G * n2;
    p2.nq = n2 * R2.prm.S;
    if ((rc = se_pass(R2, p2, any_panic, any_truncated))) return rc;
    // ---- T3: the better of the two tier winners into the caller's slots
    if ((rc = bg_seed_tiered_merge_launch(n2, p.r0, d_map, R.out, strand1, c2.hits, c2.strand, c2.ops, c.tier, R.st))) return rc;
    *rows += p2.n_sa_rows;
    *cand += p2.C;
    *reseeded += n2;
    return BG_OK;
}

// The call's checks, its passes, its totals.
int se_run(const SeedCall& c) {
    if (!c.fm || !c.sc || (!c.prm && !c.smem && !c.tiered) || (c.n_reads && (!c.read_off || !c.hits))) return BG_ERR_INVALID_ARG;
    const uint64_t n_index = fm_len(c.fm);
    const bg_smem_seed_params_t* sp = c.tiered ? &c.tiered->smem : c.smem;  // the SMEM seeds of the call, if it has any
    const bg_seed_params_t* wp = c.tiered ? &c.tiered->window : c.prm;      // its window seeds, if it has any
    if (sp) {  // an FMD index over T$R$ (FMDIndex::from's assert, as K7 checks it)
        if (!c.fm->fmd_ok) return BG_ERR_UNSUPPORTED;
        if (n_index < 2 || n_index % 2) return BG_ERR_INVALID_ARG;
    }
    if (!c.fm->d_text || c.fm->sa_kind == 0) return BG_ERR_INVALID_ARG;  // needs bg_fm_set_text + a suffix array
    if (sp && (sp->min_seed_len == 0 || sp->max_smems == 0 || sp->max_occ == 0)) return BG_ERR_INVALID_ARG;
    if (wp && (wp->seed_len == 0 || wp->stride == 0 || wp->max_occ == 0)) return BG_ERR_INVALID_ARG;
    if (c.tiered && c.tiered->window.pad != c.tiered->smem.pad) return BG_ERR_INVALID_ARG;  // one ops_stride, one merge distance
    if (sp && (uint64_t)sp->max_smems * sp->max_occ > kMaxProposals) return BG_ERR_UNSUPPORTED;
    if (c.max_read_len > 65535 || c.pad() > 65535) return BG_ERR_TOO_LARGE;
    if (sp && c.max_read_len > 65534) return BG_ERR_TOO_LARGE;  // K7's own limit
    if (c.rescue && c.pair->max_span > 65535) return BG_ERR_TOO_LARGE;
    const uint32_t win_max = c.max_read_len + 2 * c.pad();
    const uint32_t rwin_max = c.rescue ? c.pair->max_span : 0;
    if (c.ops && c.ops_stride < (uint64_t)c.max_read_len + std::max(win_max, rwin_max) + 4) return BG_ERR_OPS_CAP;
    int rc;
    SeedPrm prm = {};
    SeedSmemPrm smem = {};
    if (c.tiered && (rc = se_seed_params(c, n_index, &prm, &smem))) return rc;  // (its limits refuse before any output is touched)
    if (c.totals) c.totals[0] = c.totals[1] = 0;
    if (c.totals && c.rescue) c.totals[2] = c.totals[3] = 0;
    if (c.totals && c.tiered) c.totals[2] = 0;
    if (c.n_reads == 0) return BG_OK;
    bg_ctx* ctx = c.fm->ctx;
    hipStream_t st = (hipStream_t)c.stream;
    BG_HIP(hipSetDevice(ctx->device));
    bg_scratch_guard guard(ctx, st);  // ctx->seed is one scratch set: calls on other streams wait for this one's last kernel
    if ((rc = se_seed_params(c, n_index, &prm, &smem))) return rc;
    if (!ctx->seed) ctx->seed = new bg_seed_scratch();
    bg_seed_scratch& W = *ctx->seed;
    if (!W.h_tot) BG_HIP(hipHostMalloc((void**)&W.h_tot, 64, hipHostMallocDefault));
    const uint32_t G = c.strands == BG_STRAND_BOTH ? 2 : 1;
    SeedRun R{c, W};
    R.ctx = ctx, R.st = st, R.prm = prm, R.smem = smem, R.G = G, R.win_max = win_max, R.rwin_max = rwin_max;
    R.virt = c.strands == BG_STRAND_REVERSE || c.strands == BG_STRAND_BOTH;
    R.out.hits = c.hits, R.out.ops = c.ops, R.out.ops_stride = c.ops_stride, R.out.strand = c.strand;
    R.out.pairs = c.pairs, R.out.multi = c.multi, R.out.rescued = c.rescued;
    if (c.tiered && !c.strand) {  // T3 chooses by the tier winners' strands: tier 1's go to scratch where the caller keeps none
        if ((rc = R.need(kTier1Strand, c.n_reads))) return rc;
        R.out.strand = R.buf<uint8_t>(kTier1Strand);
    }
    uint64_t done_hits = 0, done_cand = 0, done_rescue = 0, done_reseed = 0;
    bool any_panic = false, any_truncated = false;
    // reads per pass: bounds the scratch (seed slots, proposals, candidate pairs); bg_set_option("seed_chunk_reads") for tests
    // (default: up to 2^21 virtual reads per pass, the passes of a call of equal size).  The option counts the caller's reads;
    // in pair mode it is rounded down to whole pairs (at least one), and so are the equal passes.
    const uint64_t unit = c.pair ? 2 : 1, n_units = c.n_reads / unit;
    const uint64_t chunk_cap = std::max<uint64_t>(ctx->seed_chunk_reads > 0 ? (uint64_t)ctx->seed_chunk_reads / unit : (1u << 21) / G / unit, 1);
    const uint64_t n_pass = (n_units + chunk_cap - 1) / chunk_cap;
    const uint64_t chunk = unit * (ctx->seed_chunk_reads > 0 ? chunk_cap : (n_units + n_pass - 1) / n_pass);
    for (uint64_t r0 = 0; r0 < c.n_reads; r0 += chunk) {
        SeedPassRun p{};
        p.r0 = r0;
        p.nr = std::min(chunk, c.n_reads - r0);
        p.nv = G * p.nr;
        p.nq = (c.smem || c.tiered ? p.nr : p.nv) * std::max<uint32_t>(prm.S, 1);
        if ((rc = se_pass(R, p, &any_panic, &any_truncated))) return rc;
        if (c.tiered && (rc = se_reseed(R, p, R.out.strand, n_index, &done_hits, &done_cand, &done_reseed, &any_panic, &any_truncated)))
            return rc;
        done_hits += p.n_sa_rows;
        done_cand += p.C;
        done_rescue += p.n_rescue;
    }
    if (c.totals) {
        c.totals[0] = done_hits;
        c.totals[1] = done_cand;
    }
    if (c.totals && c.tiered) c.totals[2] = done_reseed;
    if (c.totals && c.rescue) {
        // pairs rescued: counted on the device from the bytes R1 / R4 wrote (the call's last wait, outside the passes)
        c.totals[2] = done_rescue;
        if ((rc = R.need(kRescuedCount, 64))) return rc;
        uint64_t* d_count = R.buf<uint64_t>(kRescuedCount);
        BG_HIP(hipMemsetAsync(d_count, 0, 8, st));
        if ((rc = bg_seed_rescue_count_launch(c.n_reads / 2, c.rescued, d_count, st))) return rc;
        BG_HIP(hipMemcpyAsync(&W.h_tot[5], d_count, 8, hipMemcpyDeviceToHost, st));
        BG_HIP(hipStreamSynchronize(st));
        c.totals[3] = W.h_tot[5];
    }
    // a seed that reaches a byte outside the alphabet makes the reference's backward_search panic; here it does not
    // vote, every read is still answered, and the call says so
    // (SMEM mode: a read the reference's all_smems panics on does not vote either; a read with more than max_smems records was
    // answered from the first max_smems, K7's convention for its cap)
    return any_panic ? BG_ERR_OUT_OF_ALPHABET : any_truncated ? BG_ERR_OPS_CAP : BG_OK;
}

// the mode calls' own argument checks; every other one is se_run's
int pair_args(const bg_pair_params_t* pp, const void* pairs, uint64_t n_pairs, const void* hits) {
    if (!pp || !pairs || pp->min_span > pp->max_span || pp->pen_unpaired < 0 || (n_pairs && !hits) || n_pairs > (UINT64_MAX >> 2))
        return BG_ERR_INVALID_ARG;
    return BG_OK;
}
int pairq_args(const bg_pairq_params_t* qp, const void* multi) {
    if (!qp || !multi || qp->mapq_cap > 254) return BG_ERR_INVALID_ARG;
    return BG_OK;
}
int rescue_args(const bg_rescue_params_t* rp, const void* rescued) {
    if (!rp || !rescued || rp->max_anchors == 0 || rp->max_anchors > BG_RESCUE_MAX_ANCHORS) return BG_ERR_INVALID_ARG;
    return BG_OK;
}
int multi_args(const bg_multi_params_t* mp, const void* multi, uint32_t strands, uint64_t n_reads) {
    if (!mp || !multi || mp->max_hits == 0 || mp->max_hits > BG_SEED_MAX_HITS || mp->mapq_cap > 254 || strands < BG_STRAND_FORWARD ||
        strands > BG_STRAND_BOTH || n_reads > (UINT64_MAX >> 8))
        return BG_ERR_INVALID_ARG;
    return BG_OK;
}

}  // namespace

extern "C" int bg_seed_extend_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, uint64_t n_reads,
                                        const uint8_t* d_reads, const uint64_t* d_read_off, uint32_t max_read_len,
                                        bg_seed_hit_t* d_hits, uint8_t* d_ops, uint64_t ops_stride, uint64_t* totals,
                                        void* stream) {
    SeedCall c;
    c.fm = fm, c.sc = sc, c.prm = prm, c.n_reads = n_reads, c.reads = d_reads, c.read_off = d_read_off;
    c.max_read_len = max_read_len, c.hits = d_hits, c.ops = d_ops, c.ops_stride = ops_stride, c.totals = totals, c.stream = stream;
    return se_run(c);
}

extern "C" int bg_seed_extend_strands_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, uint32_t strands,
                                                uint64_t n_reads, const uint8_t* d_reads, const uint64_t* d_read_off,
                                                uint32_t max_read_len, bg_seed_hit_t* d_hits, uint8_t* d_strand, uint8_t* d_ops,
                                                uint64_t ops_stride, uint64_t* totals, void* stream) {
    if (strands < BG_STRAND_FORWARD || strands > BG_STRAND_BOTH) return BG_ERR_INVALID_ARG;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.prm = prm, c.strands = strands, c.n_reads = n_reads, c.reads = d_reads, c.read_off = d_read_off;
    c.max_read_len = max_read_len, c.hits = d_hits, c.ops = d_ops, c.ops_stride = ops_stride, c.totals = totals, c.stream = stream;
    c.strand = d_strand;
    return se_run(c);
}

extern "C" int bg_seed_extend_smem_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_smem_seed_params_t* prm, uint32_t strands,
                                             uint64_t n_reads, const uint8_t* d_reads, const uint64_t* d_read_off, uint32_t max_read_len,
                                             bg_seed_hit_t* d_hits, uint8_t* d_strand, uint8_t* d_ops, uint64_t ops_stride,
                                             uint64_t* totals, void* stream) {
    if (!prm || strands < BG_STRAND_FORWARD || strands > BG_STRAND_BOTH) return BG_ERR_INVALID_ARG;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.smem = prm, c.strands = strands, c.n_reads = n_reads, c.reads = d_reads, c.read_off = d_read_off;
    c.max_read_len = max_read_len, c.hits = d_hits, c.ops = d_ops, c.ops_stride = ops_stride, c.totals = totals, c.stream = stream;
    c.strand = d_strand;
    return se_run(c);
}

extern "C" int bg_seed_extend_tiered_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_tiered_seed_params_t* prm, uint32_t strands,
                                               uint64_t n_reads, const uint8_t* d_reads, const uint64_t* d_read_off, uint32_t max_read_len,
                                               bg_seed_hit_t* d_hits, uint8_t* d_strand, uint8_t* d_tier, uint8_t* d_ops,
                                               uint64_t ops_stride, uint64_t* totals, void* stream) {
    if (!prm || strands < BG_STRAND_FORWARD || strands > BG_STRAND_BOTH) return BG_ERR_INVALID_ARG;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.tiered = prm, c.strands = strands, c.n_reads = n_reads, c.reads = d_reads, c.read_off = d_read_off;
    c.max_read_len = max_read_len, c.hits = d_hits, c.ops = d_ops, c.ops_stride = ops_stride, c.totals = totals, c.stream = stream;
    c.strand = d_strand, c.tier = d_tier;
    return se_run(c);
}

extern "C" int bg_seed_extend_pairs_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                                              uint64_t n_pairs, const uint8_t* d_reads, const uint64_t* d_read_off, uint32_t max_read_len,
                                              bg_seed_hit_t* d_hits, uint8_t* d_strand, bg_pair_hit_t* d_pairs, uint8_t* d_ops,
                                              uint64_t ops_stride, uint64_t* totals, void* stream) {
    if (int rc = pair_args(pp, d_pairs, n_pairs, d_hits)) return rc;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.prm = prm, c.strands = BG_STRAND_BOTH, c.n_reads = 2 * n_pairs, c.reads = d_reads, c.read_off = d_read_off;
    c.max_read_len = max_read_len, c.hits = d_hits, c.ops = d_ops, c.ops_stride = ops_stride, c.totals = totals, c.stream = stream;
    c.strand = d_strand, c.pair = pp, c.pairs = d_pairs;
    return se_run(c);
}

extern "C" int bg_seed_extend_pairs_mapq_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                                                   const bg_pairq_params_t* qp, uint64_t n_pairs, const uint8_t* d_reads,
                                                   const uint64_t* d_read_off, uint32_t max_read_len, bg_seed_hit_t* d_hits,
                                                   uint8_t* d_strand, bg_pair_hit_t* d_pairs, bg_multi_hit_t* d_multi, uint8_t* d_ops,
                                                   uint64_t ops_stride, uint64_t* totals, void* stream) {
    if (int rc = pair_args(pp, d_pairs, n_pairs, d_hits)) return rc;
    if (int rc = pairq_args(qp, d_multi)) return rc;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.prm = prm, c.strands = BG_STRAND_BOTH, c.n_reads = 2 * n_pairs, c.reads = d_reads, c.read_off = d_read_off;
    c.max_read_len = max_read_len, c.hits = d_hits, c.ops = d_ops, c.ops_stride = ops_stride, c.totals = totals, c.stream = stream;
    c.strand = d_strand, c.pair = pp, c.pairs = d_pairs, c.pairq = qp, c.multi = d_multi;
    return se_run(c);
}

extern "C" int bg_seed_extend_pairs_rescue_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                                                     const bg_rescue_params_t* rp, uint64_t n_pairs, const uint8_t* d_reads,
                                                     const uint64_t* d_read_off, uint32_t max_read_len, bg_seed_hit_t* d_hits,
                                                     uint8_t* d_strand, bg_pair_hit_t* d_pairs, uint8_t* d_rescued, uint8_t* d_ops,
                                                     uint64_t ops_stride, uint64_t* totals, void* stream) {
    if (int rc = pair_args(pp, d_pairs, n_pairs, d_hits)) return rc;
    if (int rc = rescue_args(rp, d_rescued)) return rc;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.prm = prm, c.strands = BG_STRAND_BOTH, c.n_reads = 2 * n_pairs, c.reads = d_reads, c.read_off = d_read_off;
    c.max_read_len = max_read_len, c.hits = d_hits, c.ops = d_ops, c.ops_stride = ops_stride, c.totals = totals, c.stream = stream;
    c.strand = d_strand, c.pair = pp, c.pairs = d_pairs, c.rescue = rp, c.rescued = d_rescued;
    return se_run(c);
}

extern "C" int bg_seed_extend_pairs_rescue_mapq_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm,
                                                          const bg_pair_params_t* pp, const bg_rescue_params_t* rp, const bg_pairq_params_t* qp,
                                                          uint64_t n_pairs, const uint8_t* d_reads, const uint64_t* d_read_off,
                                                          uint32_t max_read_len, bg_seed_hit_t* d_hits, uint8_t* d_strand, bg_pair_hit_t* d_pairs,
                                                          uint8_t* d_rescued, bg_multi_hit_t* d_multi, uint8_t* d_ops, uint64_t ops_stride,
                                                          uint64_t* totals, void* stream) {
    if (int rc = pair_args(pp, d_pairs, n_pairs, d_hits)) return rc;
    if (int rc = rescue_args(rp, d_rescued)) return rc;
    if (int rc = pairq_args(qp, d_multi)) return rc;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.prm = prm, c.strands = BG_STRAND_BOTH, c.n_reads = 2 * n_pairs, c.reads = d_reads, c.read_off = d_read_off;
    c.max_read_len = max_read_len, c.hits = d_hits, c.ops = d_ops, c.ops_stride = ops_stride, c.totals = totals, c.stream = stream;
    c.strand = d_strand, c.pair = pp, c.pairs = d_pairs, c.rescue = rp, c.rescued = d_rescued, c.pairq = qp, c.multi = d_multi;
    return se_run(c);
}

extern "C" int bg_seed_extend_multi_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_multi_params_t* mp,
                                              uint32_t strands, uint64_t n_reads, const uint8_t* d_reads, const uint64_t* d_read_off,
                                              uint32_t max_read_len, bg_seed_hit_t* d_hits, uint8_t* d_strand, bg_multi_hit_t* d_multi,
                                              uint8_t* d_ops, uint64_t ops_stride, uint64_t* totals, void* stream) {
    if (int rc = multi_args(mp, d_multi, strands, n_reads)) return rc;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.prm = prm, c.strands = strands, c.n_reads = n_reads, c.reads = d_reads, c.read_off = d_read_off;
    c.max_read_len = max_read_len, c.hits = d_hits, c.ops = d_ops, c.ops_stride = ops_stride, c.totals = totals, c.stream = stream;
    c.strand = d_strand, c.multi_prm = mp, c.multi = d_multi;
    return se_run(c);
}

extern "C" int bg_revcomp_batch_dev(bg_ctx* ctx, uint64_t n, const uint8_t* d_in, const uint64_t* d_off, uint8_t* d_out, void* stream) {
    if (!ctx || (n && (!d_in || !d_off || !d_out))) return BG_ERR_INVALID_ARG;
    if (n == 0) return BG_OK;
    BG_HIP(hipSetDevice(ctx->device));
    se_revcomp_kernel<<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(n, d_in, d_off, d_out);
    BG_HIP(hipGetLastError());
    return BG_OK;
}

namespace {

// The host-buffer flavours: `h` describes the call on the caller's host arrays (its max_read_len, ops, ops_stride, totals and
// stream are not set).  The same call runs on device copies; then the reported hits' operations are compacted into ops_buf in
// slot order (multi mode: max_hits slots per read).
int se_run_host(const SeedCall& h, uint8_t* ops_buf, uint64_t ops_cap, uint64_t* ops_used) {
    if (!h.fm || !h.sc || (!h.prm && !h.smem && !h.tiered) || (h.n_reads && (!h.read_off || !h.hits))) return BG_ERR_INVALID_ARG;
    if (ops_used) *ops_used = 0;
    if (h.n_reads == 0) return BG_OK;
    bg_ctx* ctx = h.fm->ctx;
    BG_HIP(hipSetDevice(ctx->device));
    const uint64_t n_reads = h.n_reads;
    uint64_t max_len = 0;
    for (uint64_t r = 0; r < n_reads; r++) max_len = std::max(max_len, h.read_off[r + 1] - h.read_off[r]);
    if (max_len > 65535) return BG_ERR_TOO_LARGE;
    if (h.rescue && h.pair->max_span > 65535) return BG_ERR_TOO_LARGE;
    // (rescue call: a slot also holds the operations of a read against a rescue window of max_span bytes)
    const uint64_t stride = ops_buf ? max_len + std::max<uint64_t>(max_len + 2 * (uint64_t)h.pad(), h.rescue ? h.pair->max_span : 0) + 4 : 0;
    const uint64_t n_slots = n_reads * (h.multi_prm ? h.multi_prm->max_hits : 1);
    const uint64_t bytes = h.read_off[n_reads], n_pairs = n_reads / 2;
    std::vector<uint8_t> h_ops;
    SeedCall d = h;  // the same call on device copies; an output the call does not have stays null
    uint8_t* d_reads = nullptr;
    uint64_t* d_off = nullptr;
    d.hits = nullptr, d.strand = nullptr, d.pairs = nullptr, d.rescued = nullptr, d.multi = nullptr, d.tier = nullptr;
    d.max_read_len = (uint32_t)max_len, d.ops_stride = stride, d.stream = ctx->stream;
    int panic_rc = BG_OK;
    auto run = [&]() -> int {
        hipStream_t st = ctx->stream;
        BG_HIP(hipMalloc((void**)&d_reads, std::max<uint64_t>(bytes, 16)));
        BG_HIP(hipMalloc((void**)&d_off, (n_reads + 1) * 8));
        BG_HIP(hipMalloc((void**)&d.hits, n_slots * sizeof(bg_seed_hit_t)));
        if (stride) BG_HIP(hipMalloc((void**)&d.ops, n_slots * stride));
        if (h.strand) BG_HIP(hipMalloc((void**)&d.strand, n_slots));
        if (h.pairs) BG_HIP(hipMalloc((void**)&d.pairs, n_pairs * sizeof(bg_pair_hit_t)));
        if (h.rescued) BG_HIP(hipMalloc((void**)&d.rescued, std::max<uint64_t>(n_pairs, 16)));
        if (h.multi) BG_HIP(hipMalloc((void**)&d.multi, n_reads * sizeof(bg_multi_hit_t)));
        if (h.tier) BG_HIP(hipMalloc((void**)&d.tier, std::max<uint64_t>(n_reads, 16)));
        if (bytes) BG_HIP(hipMemcpyAsync(d_reads, h.reads, bytes, hipMemcpyHostToDevice, st));
        BG_HIP(hipMemcpyAsync(d_off, h.read_off, (n_reads + 1) * 8, hipMemcpyHostToDevice, st));
        d.reads = d_reads, d.read_off = d_off;
        int rc = se_run(d);
        // (every read is answered under these two; the stride above is the call's own, so BG_ERR_OPS_CAP is the SMEM cap's)
        if (rc && rc != BG_ERR_OUT_OF_ALPHABET && !(rc == BG_ERR_OPS_CAP && (h.smem || h.tiered))) return rc;
        panic_rc = rc;
        BG_HIP(hipMemcpyAsync(h.hits, d.hits, n_slots * sizeof(bg_seed_hit_t), hipMemcpyDeviceToHost, st));
        if (h.strand) BG_HIP(hipMemcpyAsync(h.strand, d.strand, n_slots, hipMemcpyDeviceToHost, st));
        if (h.pairs) BG_HIP(hipMemcpyAsync(h.pairs, d.pairs, n_pairs * sizeof(bg_pair_hit_t), hipMemcpyDeviceToHost, st));
        if (h.rescued) BG_HIP(hipMemcpyAsync(h.rescued, d.rescued, n_pairs, hipMemcpyDeviceToHost, st));
        if (h.multi) BG_HIP(hipMemcpyAsync(h.multi, d.multi, n_reads * sizeof(bg_multi_hit_t), hipMemcpyDeviceToHost, st));
        if (h.tier) BG_HIP(hipMemcpyAsync(h.tier, d.tier, n_reads, hipMemcpyDeviceToHost, st));
        if (stride) {
            h_ops.resize(n_slots * stride);
            BG_HIP(hipMemcpyAsync(h_ops.data(), d.ops, n_slots * stride, hipMemcpyDeviceToHost, st));
        }
        BG_HIP(hipStreamSynchronize(st));
        return BG_OK;
    };
    int rc = run();
    for (void* q : {(void*)d_reads, (void*)d_off, (void*)d.hits, (void*)d.ops, (void*)d.strand, (void*)d.pairs, (void*)d.rescued, (void*)d.multi, (void*)d.tier})
        hipFree(q);
    if (rc) return rc;
    // compact the winners' operations into the caller's buffer, in read order
    bg_seed_hit_t* hits = h.hits;
    uint64_t used = 0;
    int status = BG_OK;
    for (uint64_t r = 0; r < n_slots; r++) {
        bg_alignment_t& a = hits[r].aln;
        if (a.status) status = a.status;
        if (ops_buf) {
            if (used + a.n_ops <= ops_cap)
                memcpy(ops_buf + used, h_ops.data() + a.ops_off, a.n_ops);
            else if (status == BG_OK)
                status = BG_ERR_OPS_CAP;
        }
        a.ops_off = used;
        used += ops_buf ? a.n_ops : 0;
    }
    if (ops_used) *ops_used = used;
    return status ? status : panic_rc;
}

}  // namespace

extern "C" int bg_seed_extend_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, uint64_t n_reads,
                                    const uint8_t* reads, const uint64_t* read_off, bg_seed_hit_t* hits, uint8_t* ops_buf,
                                    uint64_t ops_cap, uint64_t* ops_used) {
    SeedCall c;
    c.fm = fm, c.sc = sc, c.prm = prm, c.strands = 0, c.n_reads = n_reads, c.reads = reads, c.read_off = read_off;
    c.hits = hits;
    return se_run_host(c, ops_buf, ops_cap, ops_used);
}

extern "C" int bg_seed_extend_strands_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, uint32_t strands,
                                            uint64_t n_reads, const uint8_t* reads, const uint64_t* read_off, bg_seed_hit_t* hits,
                                            uint8_t* strand, uint8_t* ops_buf, uint64_t ops_cap, uint64_t* ops_used) {
    if (strands < BG_STRAND_FORWARD || strands > BG_STRAND_BOTH) return BG_ERR_INVALID_ARG;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.prm = prm, c.strands = strands, c.n_reads = n_reads, c.reads = reads, c.read_off = read_off;
    c.hits = hits, c.strand = strand;
    return se_run_host(c, ops_buf, ops_cap, ops_used);
}

extern "C" int bg_seed_extend_smem_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_smem_seed_params_t* prm, uint32_t strands,
                                         uint64_t n_reads, const uint8_t* reads, const uint64_t* read_off, bg_seed_hit_t* hits,
                                         uint8_t* strand, uint8_t* ops_buf, uint64_t ops_cap, uint64_t* ops_used) {
    if (!prm || strands < BG_STRAND_FORWARD || strands > BG_STRAND_BOTH) return BG_ERR_INVALID_ARG;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.smem = prm, c.strands = strands, c.n_reads = n_reads, c.reads = reads, c.read_off = read_off;
    c.hits = hits, c.strand = strand;
    return se_run_host(c, ops_buf, ops_cap, ops_used);
}

extern "C" int bg_seed_extend_tiered_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_tiered_seed_params_t* prm, uint32_t strands,
                                           uint64_t n_reads, const uint8_t* reads, const uint64_t* read_off, bg_seed_hit_t* hits,
                                           uint8_t* strand, uint8_t* tier, uint8_t* ops_buf, uint64_t ops_cap, uint64_t* ops_used) {
    if (!prm || strands < BG_STRAND_FORWARD || strands > BG_STRAND_BOTH) return BG_ERR_INVALID_ARG;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.tiered = prm, c.strands = strands, c.n_reads = n_reads, c.reads = reads, c.read_off = read_off;
    c.hits = hits, c.strand = strand, c.tier = tier;
    return se_run_host(c, ops_buf, ops_cap, ops_used);
}

extern "C" int bg_seed_extend_pairs_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                                          uint64_t n_pairs, const uint8_t* reads, const uint64_t* read_off, bg_seed_hit_t* hits,
                                          uint8_t* strand, bg_pair_hit_t* pairs, uint8_t* ops_buf, uint64_t ops_cap, uint64_t* ops_used) {
    if (int rc = pair_args(pp, pairs, n_pairs, hits)) return rc;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.prm = prm, c.strands = BG_STRAND_BOTH, c.n_reads = 2 * n_pairs, c.reads = reads, c.read_off = read_off;
    c.hits = hits, c.strand = strand, c.pair = pp, c.pairs = pairs;
    return se_run_host(c, ops_buf, ops_cap, ops_used);
}

extern "C" int bg_seed_extend_pairs_rescue_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                                                 const bg_rescue_params_t* rp, uint64_t n_pairs, const uint8_t* reads, const uint64_t* read_off,
                                                 bg_seed_hit_t* hits, uint8_t* strand, bg_pair_hit_t* pairs, uint8_t* rescued, uint8_t* ops_buf,
                                                 uint64_t ops_cap, uint64_t* ops_used) {
    if (int rc = pair_args(pp, pairs, n_pairs, hits)) return rc;
    if (int rc = rescue_args(rp, rescued)) return rc;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.prm = prm, c.strands = BG_STRAND_BOTH, c.n_reads = 2 * n_pairs, c.reads = reads, c.read_off = read_off;
    c.hits = hits, c.strand = strand, c.pair = pp, c.pairs = pairs, c.rescue = rp, c.rescued = rescued;
    return se_run_host(c, ops_buf, ops_cap, ops_used);
}

extern "C" int bg_seed_extend_multi_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_multi_params_t* mp,
                                          uint32_t strands, uint64_t n_reads, const uint8_t* reads, const uint64_t* read_off,
                                          bg_seed_hit_t* hits, uint8_t* strand, bg_multi_hit_t* multi, uint8_t* ops_buf, uint64_t ops_cap,
                                          uint64_t* ops_used) {
    if (int rc = multi_args(mp, multi, strands, n_reads)) return rc;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.prm = prm, c.strands = strands, c.n_reads = n_reads, c.reads = reads, c.read_off = read_off;
    c.hits = hits, c.strand = strand, c.multi_prm = mp, c.multi = multi;
    return se_run_host(c, ops_buf, ops_cap, ops_used);
}

extern "C" int bg_seed_extend_pairs_mapq_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                                               const bg_pairq_params_t* qp, uint64_t n_pairs, const uint8_t* reads, const uint64_t* read_off,
                                               bg_seed_hit_t* hits, uint8_t* strand, bg_pair_hit_t* pairs, bg_multi_hit_t* multi,
                                               uint8_t* ops_buf, uint64_t ops_cap, uint64_t* ops_used) {
    if (int rc = pair_args(pp, pairs, n_pairs, hits)) return rc;
    if (int rc = pairq_args(qp, multi)) return rc;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.prm = prm, c.strands = BG_STRAND_BOTH, c.n_reads = 2 * n_pairs, c.reads = reads, c.read_off = read_off;
    c.hits = hits, c.strand = strand, c.pair = pp, c.pairs = pairs, c.pairq = qp, c.multi = multi;
    return se_run_host(c, ops_buf, ops_cap, ops_used);
}

extern "C" int bg_seed_extend_pairs_rescue_mapq_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                                                      const bg_rescue_params_t* rp, const bg_pairq_params_t* qp, uint64_t n_pairs,
                                                      const uint8_t* reads, const uint64_t* read_off, bg_seed_hit_t* hits, uint8_t* strand,
                                                      bg_pair_hit_t* pairs, uint8_t* rescued, bg_multi_hit_t* multi, uint8_t* ops_buf,
                                                      uint64_t ops_cap, uint64_t* ops_used) {
    if (int rc = pair_args(pp, pairs, n_pairs, hits)) return rc;
    if (int rc = rescue_args(rp, rescued)) return rc;
    if (int rc = pairq_args(qp, multi)) return rc;
    SeedCall c;
    c.fm = fm, c.sc = sc, c.prm = prm, c.strands = BG_STRAND_BOTH, c.n_reads = 2 * n_pairs, c.reads = reads, c.read_off = read_off;
    c.hits = hits, c.strand = strand, c.pair = pp, c.pairs = pairs, c.rescue = rp, c.rescued = rescued, c.pairq = qp, c.multi = multi;
    return se_run_host(c, ops_buf, ops_cap, ops_used);
}
