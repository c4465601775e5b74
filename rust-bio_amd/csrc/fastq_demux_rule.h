// The per-record bodies of fastq_demux.hip (bg_fastq_demux_assign[_dev], bg_fastq_demux_split[_dev]; both rules in
// include/biogpu.h) as __host__ __device__ functions: the kernels call them with the lanes of a group or of a wavefront,
// tests/fastq_demux_host_bodies.cpp calls them lane by lane on the CPU under AddressSanitizer.  What a shuffle or a ballot
// gives a kernel is an argument here, so that the host program can hand over the same value.
#ifndef BG_FASTQ_DEMUX_RULE_H
#define BG_FASTQ_DEMUX_RULE_H
#include "fastq_emit_rule.h"

// ---- bg_fastq_demux_assign ----------------------------------------------------------------------------------------------
// the sample of every pattern as the kernel takes it: 16 bits each (a sample is below BG_DMX_MAX_BINS), 2 KB by value
#define DMX_BIN_IGNORE 0xFFFFu
struct dmx_bins {
    uint16_t b[BG_MYERS_MAX_PATTERNS];
};

// What a set of counting hits comes to: the winner — the smallest (score, p) — with its bin, and the smallest score among
// the hits of every OTHER bin.  That is all the verdict needs, and two such states merge exactly (dmx_merge), so the lanes
// of a group, and the two mates of a pair, may each reduce a share and combine.  The runner-up's own bin is not kept: it is
// only ever compared with the winner's, and that comparison is made where a state loses its winner (dmx_merge).
struct dmx_state {
    int32_t s1;     // the winner's score
    uint32_t p1;    // ... its pattern; BG_DMX_IGNORE: no counting hit
    uint32_t bin1;  // ... its bin
    int32_t s2;     // the smallest score among counting hits whose bin is not bin1
    uint32_t has2;  // ... 0: there is none (`second` is infinite)
};
FQ_HD dmx_state dmx_empty() { return {0, BG_DMX_IGNORE, 0, 0, 0}; }
FQ_HD bool dmx_is_empty(const dmx_state& a) { return a.p1 == BG_DMX_IGNORE; }

// rule 1: does pattern p's record count?  bin: the pattern's entry of dmx_bins
FQ_HD bool dmx_counts(const bg_alignment_t& h, uint32_t bin, uint32_t flags, uint32_t max_offset) {
    if (h.score == BG_MIN_SCORE || bin == DMX_BIN_IGNORE) return false;
    if ((flags & BG_DMX_ANCHOR_5P) && h.ystart > max_offset) return false;
    if ((flags & BG_DMX_ANCHOR_3P) && h.ylen - h.yend > max_offset) return false;
    return true;
}
// a wins against b: it has a hit and b has none or no smaller (score, p) — equal ones go to a, the earlier mate
FQ_HD bool dmx_first_wins(const dmx_state& a, const dmx_state& b) {
    if (dmx_is_empty(a) || dmx_is_empty(b)) return !dmx_is_empty(a);
    return a.s1 < b.s1 || (a.s1 == b.s1 && a.p1 <= b.p1);
}
// a if c, b otherwise — field by field, so that a kernel keeps both states in registers
FQ_HD dmx_state dmx_pick(bool c, const dmx_state& a, const dmx_state& b) {
    return {c ? a.s1 : b.s1, c ? a.p1 : b.p1, c ? a.bin1 : b.bin1, c ? a.s2 : b.s2, c ? a.has2 : b.has2};
}
// The state of the union of two sets.  The loser's hits outside the winner's bin are: all of them if its own winner has
// another bin (the smallest is then its s1), otherwise exactly the ones its s2 is the smallest of.
FQ_HD dmx_state dmx_merge(const dmx_state& a, const dmx_state& b) {
    const bool aw = dmx_first_wins(a, b);  // an empty state loses; two empty ones give an empty one
    dmx_state o = dmx_pick(aw, a, b);
    const dmx_state l = dmx_pick(aw, b, a);
    const bool other_bin = l.bin1 != o.bin1;
    const uint32_t has = dmx_is_empty(l) ? 0u : other_bin ? 1u : l.has2;
    const int32_t cand = other_bin ? l.s1 : l.s2;
    if (has && (!o.has2 || cand < o.s2)) {
        o.has2 = 1;
        o.s2 = cand;
    }
    return o;
}
// this lane's share of a read's n_pat records: patterns lane, lane + G, ...
FQ_HD dmx_state dmx_lane_share(const bg_alignment_t* hits, uint32_t n_pat, const uint16_t* bins, uint32_t flags, uint32_t max_offset,
                               uint32_t lane, uint32_t G) {
    dmx_state s = dmx_empty();
    for (uint32_t p = lane; p < n_pat; p += G)
        if (dmx_counts(hits[p], bins[p], flags, max_offset)) s = dmx_merge(s, dmx_state{hits[p].score, p, bins[p], 0, 0});
    return s;
}
// rule 7: do the hits of mate `mate` (0 or 1) of a pair count?
FQ_HD bool dmx_mate_counts(uint32_t flags, uint32_t mate) {
    if (!(flags & BG_DMX_PAIRED) || !(flags & (BG_DMX_MATE1 | BG_DMX_MATE2))) return true;
    return (flags & (mate ? BG_DMX_MATE2 : BG_DMX_MATE1)) != 0;
}
// The pair rule.  own / other: the states of this read and of its mate, already emptied where dmx_mate_counts says no.
// Returns the pair's state; *holds: this read is the one the winner is on.
FQ_HD dmx_state dmx_pair(const dmx_state& own, const dmx_state& other, uint32_t mate, bool* holds) {
    const dmx_state first = dmx_pick(mate != 0, other, own), second = dmx_pick(mate != 0, own, other);
    const bool fw = dmx_first_wins(first, second);
    *holds = !dmx_is_empty(own) && (fw == (mate == 0));
    return dmx_merge(first, second);
}
// rule 4
FQ_HD uint32_t dmx_verdict(const dmx_state& s, uint32_t n_bins, uint32_t min_margin) {
    if (dmx_is_empty(s)) return n_bins;
    if (s.has2 && (int64_t)s.s2 - (int64_t)s.s1 < (int64_t)min_margin) return n_bins + 1;
    return s.bin1;
}
// rule 5: the 16 words of hit_out[r] by the G lanes of the group: the winning record (win != null) or the no-hit record,
// which has the score, and ylen and mode of the read's first record
FQ_HD void dmx_write_hit(bg_alignment_t* out, const bg_alignment_t* first, const bg_alignment_t* win, uint32_t lane, uint32_t G) {
    uint32_t* o = (uint32_t*)out;
    const uint32_t* f = (const uint32_t*)first;
    const uint32_t* w = (const uint32_t*)win;
    for (uint32_t i = lane; i < 16; i += G) {
        uint32_t v = 0;
        if (win)
            v = w[i];
        else if (i == 0)
            v = (uint32_t)BG_MIN_SCORE;
        else if (i == 6)
            v = f[6];  // ylen
        else if (i == 14)
            v = f[14] & 0x0000FF00u;  // n_clips, MODE, status, _pad
        o[i] = v;
    }
}

// ---- bg_fastq_demux_split -----------------------------------------------------------------------------------------------
// A tile is DMX_TILE records; wavefront w of the tile's block takes the DMX_TILE / DMX_WAVES records behind w * that many, 64
// a step, so that the input order inside a tile is (wavefront, step, lane).
#define DMX_TILE 2048u
#define DMX_WAVES 4u
#define DMX_STEPS (DMX_TILE / DMX_WAVES / 64u)
FQ_HD uint64_t dmx_item(uint64_t tile, uint32_t wave, uint32_t step, uint32_t lane) {
    return tile * DMX_TILE + wave * (DMX_TILE / DMX_WAVES) + step * 64u + lane;
}
// the group of a bin value: the samples, n_bins unassigned, n_bins + 1 ambiguous; anything above is unassigned
FQ_HD uint32_t dmx_group(uint32_t bin, uint32_t n_bins) { return bin > n_bins + 1 ? n_bins : bin; }
// bits a group number takes
FQ_HD uint32_t dmx_group_bits(uint32_t n_bins) {
    uint32_t b = 1;
    while (((n_bins + 1) >> b) != 0) b++;
    return b;
}
// The lanes of a wavefront with this lane's group, found bit by bit: `peers` starts as the live lanes and is narrowed once
// per bit by the ballot of that bit over the wavefront (dead lanes vote 0 and are not among the peers anyway).
FQ_HD uint64_t dmx_narrow(uint64_t peers, uint64_t ballot, uint32_t my_bit) { return peers & (my_bit ? ballot : ~ballot); }
// how many of them are earlier lanes: the record's stable rank among the wavefront's records of its group in this step
FQ_HD uint32_t dmx_rank_below(uint64_t peers, uint32_t lane) { return (uint32_t)__builtin_popcountll(peers & (((uint64_t)1 << lane) - 1)); }
FQ_HD uint32_t dmx_peer_count(uint64_t peers) { return (uint32_t)__builtin_popcountll(peers); }

#endif
