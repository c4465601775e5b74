// One pass of seed-and-extend as its reduction stages see it (seed_pairs.hip, seed_pairq.hip, seed_multi.hip, seed_rescue.hip,
// seed_rescueq.hip, and se_best_kernel of seed_extend.hip): what stages S0-S6 of seed_extend.hip left in the pass scratch
// (SeedPass), where the answers go (SeedOut), and the launchers of the stages, which take these two plus what is their own.
// The SMEM-seeded call's candidate stages (seed_smem.hip) and the tiered call's own stages (seed_tiered.hip) are declared here as
// well.
#ifndef BG_SEED_PASS_H
#define BG_SEED_PASS_H
#include "fm_kernels.h"

namespace bgseed {

// Candidates of one virtual read are at most this (its proposals: seed slots x max_occ, sorted in LDS by one wavefront).
constexpr uint32_t kMaxCand = 1024;
constexpr uint32_t kMaskWords = 4;  // se_multi_kernel: one "out" bit per candidate in four dwords per lane
static_assert(kMaxCand <= 1u << 10, "a candidate index is a 10-bit field of the pair rule's key");
static_assert(4 * kMaxCand <= 1u << 13, "a candidate of a pair, relative to the pair's first, is a 13-bit field of a rescue plan entry");
static_assert(2 * kMaxCand <= 16 * 32 * kMaskWords, "the multi stage keeps one bit per candidate of both strands of a read");

// The pass: `n` units (reads; in the pair modes pairs of interleaved mates) from caller read r0 on.  A read has G virtual
// reads (itself, or itself and its revcomp), a pair the four m1, rc(m1), m2, rc(m2); virtual read v owns candidates
// coff[v] .. coff[v + 1) of aln / w_lo (the candidate's alignment with operations at c_ops + aln.ops_off, its window's
// first text offset) and resolved n_hits[v] suffix-array rows.  voff: the virtual reads' byte offsets (rescue stages).
struct SeedPass {
    uint64_t r0, n;
    const uint64_t* coff;
    const uint32_t* n_hits;
    const bg_alignment_t* aln;
    const uint8_t* c_ops;
    const uint64_t* w_lo;
    const uint64_t* voff;
};

// The caller's whole arrays (absent: null).  Slot s of hits / strand ends its operations at ops + (s + 1) * ops_stride.
struct SeedOut {
    bg_seed_hit_t* hits;
    uint8_t* ops;
    uint64_t ops_stride;
    uint8_t* strand;
    bg_pair_hit_t* pairs;
    bg_multi_hit_t* multi;
    uint8_t* rescued;
};

// What R1 leaves per pair of the pass: the plan entries (bg_seed_rescue_plan_bytes), the mates' own score sum, and the counts
// of rescue alignments / x bytes / y bytes.
struct SeedRescuePlan {
    void* plan;
    int64_t* own_sum;
    uint32_t *n_res, *x_bytes, *y_bytes;
};
// The scans of per-unit counts of alignments / x bytes / y bytes (n + 1 entries each): unit u's alignments are roff[u] ..
// roff[u + 1), their sequences start at x + xoff[u] and y + yoff[u].
struct SeedXYOff {
    const uint64_t *roff, *xoff, *yoff;
};
// the input of a batch of alignments: sequences back to back and their offsets
struct SeedPairsXY {
    uint8_t* x;
    uint64_t* x_off;
    uint8_t* y;
    uint64_t* y_off;
};
// R3's answer: rescue alignment j of pair p is aln[roff[p] + j], its operations at ops + aln.ops_off
struct SeedRescueAln {
    const uint64_t* roff;
    const bg_alignment_t* aln;
    const uint8_t* ops;
};

}  // namespace bgseed

// seed_smem.hip: the SMEM-seeded call's own stages (bg_seed_extend_smem_batch).  The pass has nr caller reads with M = max_smems
// record slots each; read r's records are rec[(r * M + t) * 6 ..], six uint64 as bg_fmd_smems_batch64_dev writes them.
namespace bgseed {
struct SeedSmemPrm {
    uint32_t M, max_occ, pad, strands;  // max_smems; BG_STRAND_*
    uint64_t n_t;                       // length of the forward text: the index is over T$R$, 2 n_t + 2 symbols
};
// bits of the pass's flag word
constexpr uint32_t kFlagPanic = 1, kFlagLongRead = 2, kFlagTruncated = 4;
}  // namespace bgseed
// a read longer than max_read_len sets kFlagLongRead (K7 sizes its interval lists by max_read_len: checked before it runs)
int bg_seed_smem_lengths_launch(uint64_t nr, const uint64_t* d_read_off, uint32_t max_read_len, uint32_t* d_flags, hipStream_t st);
// S1', S2': K7 (all_smems, uint64 records) over the reads, then per slot its votes and its interval's first row; a read K7
// marks as a panic sets kFlagPanic, one with more than M records kFlagTruncated
int bg_seed_smem_seeds_launch(bg_fm* fm, const bgseed::SeedSmemPrm& prm, uint32_t min_seed_len, uint64_t nr, const uint8_t* d_reads,
                              const uint64_t* d_read_off, uint32_t max_read_len, uint32_t* d_count, uint64_t* d_rec, uint32_t* d_votes,
                              uint64_t* d_lower, uint32_t* d_flags, hipStream_t st);
// S2' alone, over n_q = nr * M record slots that are already written (the tiered call's window records)
int bg_seed_smem_votes_launch(uint64_t n_q, const bgseed::SeedSmemPrm& prm, const uint32_t* d_count, const uint64_t* d_rec, uint32_t* d_votes,
                              uint64_t* d_lower, uint32_t* d_flags, hipStream_t st);
// S4': hits -> (strand, start) proposals, sorted and merged per strand; read r's kept starts go back over pos from hoff[r * M]
// on, the forward strand's first; per virtual read (G r + g): where its starts begin (soff), candidates, hits, x and y bytes
int bg_seed_smem_propose_launch(bool wide, const bgseed::SeedSmemPrm& prm, uint64_t nr, const uint64_t* d_read_off, const uint64_t* d_hoff,
                                const uint64_t* d_rec, uint64_t* d_pos, uint64_t* d_soff, uint32_t* d_n_cand, uint32_t* d_n_hits,
                                uint32_t* d_x_bytes, uint32_t* d_y_bytes, hipStream_t st);
// seed_tiered.hip: the tiered call's own stages (bg_seed_extend_tiered_batch).
// S1": K5's (tag, lower, upper) of the nr * S window slots of the caller's reads -> their records in K7's layout (six uint64 per
// slot: lower, lower_rev = 0, size, match_size, position, length; size 0 unless the search is Complete) and the reads' own window
// counts (<= S); a window that reached a byte outside the alphabet sets kFlagPanic
int bg_seed_tiered_records_launch(uint64_t nr, uint32_t S, uint32_t stride, uint32_t seed_len, const uint64_t* d_read_off,
                                  const uint8_t* d_tag, const uint64_t* d_lower, const uint64_t* d_upper, uint32_t* d_count,
                                  uint64_t* d_rec, uint32_t* d_flags, hipStream_t st);
// T1: per read r of the pass (caller read r0 + r; d_read_off: the caller's offsets): flag = its hit scores below reseed_below,
// bytes = its length if flagged; tier[r0 + r] = BG_TIER_NONE where the caller has a tier array
int bg_seed_tiered_select_launch(uint64_t nr, uint64_t r0, const bg_seed_hit_t* d_hits, const uint64_t* d_read_off, int32_t reseed_below,
                                 uint32_t* d_flag, uint32_t* d_bytes, uint8_t* d_tier, hipStream_t st);
// T2: the flagged reads back to back (d_idx, d_boff: the scans of T1's two arrays, nr + 1 entries): bytes, idx[nr] + 1 offsets,
// and map[j] = the read of the pass that compact read j is
int bg_seed_tiered_gather_launch(uint64_t nr, uint64_t r0, const uint8_t* d_reads, const uint64_t* d_read_off, const uint32_t* d_flag,
                                 const uint64_t* d_idx, const uint64_t* d_boff, uint8_t* d_out, uint64_t* d_out_off, uint32_t* d_map,
                                 hipStream_t st);
// T3: the answer of every re-seeded read (seed_tier_rule.h) into the caller's slot r0 + map[j]; d_strand1: tier 1's strand per
// caller read (O.strand or scratch), rewritten with the winner's; slot j of d_hits2 / d_strand2 / d_ops2 (stride O.ops_stride)
// is tier 2's answer
int bg_seed_tiered_merge_launch(uint64_t n2, uint64_t r0, const uint32_t* d_map, const bgseed::SeedOut& O, uint8_t* d_strand1,
                                const bg_seed_hit_t* d_hits2, const uint8_t* d_strand2, const uint8_t* d_ops2, uint8_t* d_tier,
                                hipStream_t st);
// seed_pairs.hip: S7 of the paired call: hits, strand and operations of reads r0 + 2p, r0 + 2p + 1 and pairs[r0 / 2 + p].
int bg_seed_pairs_launch(const bgseed::SeedPass& P, const bgseed::SeedOut& O, const bg_pair_params_t* pp, hipStream_t st);
// seed_pairq.hip: S7 of the pairs-mapq call: what bg_seed_pairs_launch writes, plus multi[r0 + 2p], multi[r0 + 2p + 1].
int bg_seed_pairq_launch(const bgseed::SeedPass& P, const bgseed::SeedOut& O, const bg_pair_params_t* pp, const bg_pairq_params_t* qp,
                         hipStream_t st);
// seed_multi.hip: S7 of the multi call (G virtual reads per read; strand1: the strand of every hit when G = 1).  Read r0 + r
// owns slots K (r0 + r) .. K (r0 + r) + K - 1 of hits / strand / ops and multi[r0 + r].
int bg_seed_multi_launch(const bgseed::SeedPass& P, const bgseed::SeedOut& O, const bg_multi_params_t* mp, uint32_t G, uint8_t strand1,
                         hipStream_t st);
// seed_rescue.hip: stages R1, R2, R4 of the rescue call.  R1 answers every pair as bg_seed_pairs_launch does and plans the rescue
// alignments; R2 gathers their (x, window) pairs at the scanned offsets; R4 rewrites the rescued pairs.
size_t bg_seed_rescue_plan_bytes(uint64_t n_pairs);
int bg_seed_rescue_plan_launch(const bgseed::SeedPass& P, const bgseed::SeedOut& O, const bg_pair_params_t* pp, const bg_rescue_params_t* rp,
                               uint64_t n_text, const bgseed::SeedRescuePlan& plan, hipStream_t st);
int bg_seed_rescue_gather_launch(const bgseed::SeedPass& P, const uint8_t* d_vreads, const uint8_t* d_text, const void* d_plan,
                                 const bgseed::SeedXYOff& off, const bgseed::SeedPairsXY& xy, hipStream_t st);
int bg_seed_rescue_pick_launch(const bgseed::SeedPass& P, const bgseed::SeedOut& O, const bg_pair_params_t* pp, const bg_rescue_params_t* rp,
                               const bgseed::SeedRescuePlan& plan, const bgseed::SeedRescueAln& res, hipStream_t st);
// *d_count += the pairs of the call with a non-zero rescued byte (totals[3])
int bg_seed_rescue_count_launch(uint64_t n_pairs, const uint8_t* d_rescued, uint64_t* d_count, hipStream_t st);
// seed_rescueq.hip: the stage after R4 of the rescue-mapq call: multi[r0 + 2p], multi[r0 + 2p + 1] of every pair p of the pass with
// a non-zero rescued byte.  The other pairs' records are written before R1 (bg_seed_pairq_launch) and stay.
int bg_seed_rescueq_launch(const bgseed::SeedPass& P, const bgseed::SeedOut& O, const bg_pair_params_t* pp, const bg_rescue_params_t* rp,
                           const bg_pairq_params_t* qp, const void* d_plan, const bgseed::SeedRescueAln& res, hipStream_t st);

#endif
