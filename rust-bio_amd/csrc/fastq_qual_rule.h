// The per-read and per-lane bodies of fastq_qual.hip (bg_fastq_qual_cut[_dev], bg_fastq_qual_select[_dev],
// bg_fastq_qc_tables[_dev]; the rules are in include/biogpu.h) as __host__ __device__ functions.  Two statements of every
// rule live here: the SERIAL one (ql_cut_serial, ql_stats_serial), which is the definition, and the LANE-PARALLEL one the
// kernels run — a group of G lanes per read, G symbols a step.  What a shuffle gives a kernel (a scan, a minimum, a maximum
// over the group) is an argument here, so that tests/fastq_qual_host_bodies.cpp can hand over the same values lane by lane
// on the CPU under AddressSanitizer.  Every load is a byte load at an index inside the read.
#ifndef BG_FASTQ_QUAL_RULE_H
#define BG_FASTQ_QUAL_RULE_H
#include "fastq_emit_rule.h"

#define QL_G 16u  // lanes per read in the kernels

// the quality of byte c
FQ_HD uint32_t ql_q(uint8_t c, uint32_t phred_offset) { return c > phred_offset ? c - phred_offset : 0u; }

// ---- bg_fastq_qual_cut: the serial statement ----------------------------------------------------------------------------
// RUNSUM from one end, in steps t = 0 .. L - 1 away from that end: the number of symbols cut
FQ_HD uint32_t ql_runsum_serial(const uint8_t* q, uint32_t L, uint32_t phred_offset, uint32_t cutoff, bool from_end) {
    int64_t s = 0, best = 0;
    uint32_t cnt = 0;
    for (uint32_t t = 0; t < L; t++) {
        s += (int64_t)cutoff - (int64_t)ql_q(q[from_end ? L - 1 - t : t], phred_offset);
        if (s < 0) break;
        if (s > best) {
            best = s;
            cnt = t + 1;
        }
    }
    return cnt;
}
FQ_HD uint32_t ql_window_serial(const uint8_t* q, uint32_t L, uint32_t phred_offset, uint32_t cutoff, uint32_t window) {
    const uint32_t W = window < L ? window : L;
    uint32_t e = L;
    for (uint64_t i = 0; i + W <= L; i++) {
        uint64_t sum = 0;
        for (uint32_t k = 0; k < W; k++) sum += ql_q(q[i + k], phred_offset);
        if (sum < (uint64_t)cutoff * W) {
            e = (uint32_t)i;
            while (e > 0 && ql_q(q[e - 1], phred_offset) < cutoff) e--;
            break;
        }
    }
    return e;
}
FQ_HD void ql_cut_serial(const uint8_t* q, uint32_t L, const bg_qual_cut_t& p, uint32_t* b_out, uint32_t* e_out) {
    uint32_t b = 0, e = L;
    if (p.method_5p == BG_QCUT_RUNSUM) b = ql_runsum_serial(q, L, p.phred_offset, p.cutoff_5p, false);
    if (p.method_3p == BG_QCUT_RUNSUM) e = L - ql_runsum_serial(q, L, p.phred_offset, p.cutoff_3p, true);
    if (p.method_3p == BG_QCUT_WINDOW) e = ql_window_serial(q, L, p.phred_offset, p.cutoff_3p, p.window);
    if (e < b) e = b;
    *b_out = b;
    *e_out = e;
}
// word i (0 .. 15) of the record of a read of L symbols that keeps [b, e)
FQ_HD uint32_t ql_cut_word(uint32_t L, uint32_t b, uint32_t e, uint32_t i) {
    const bool cut = L != 0 && !(b == 0 && e == L);
    if (i == 0) return cut ? L - (e - b) : (uint32_t)BG_MIN_SCORE;
    if (i == 3) return cut ? e : 0u;  // ystart
    if (i == 4) return cut ? b : 0u;  // yend
    if (i == 6) return L;             // ylen
    return 0u;
}

// ---- bg_fastq_qual_cut: G symbols a step ----------------------------------------------------------------------------------
// RUNSUM.  A cutoff above 256 gives what 256 gives: every term cutoff - q is then at least 1, so s grows with every symbol,
// never goes negative, and every step is a new maximum — the whole read is cut either way.  With the cutoff clamped a term
// lies in [-255, 256] and the prefix sums inside a step of at most 16 symbols in [-4080, 4096]: 32 bits hold them, and
// only the carried s and best are 64 bits wide.
FQ_HD int32_t ql_run_cutoff(uint32_t cutoff) { return cutoff > 256u ? 256 : (int32_t)cutoff; }
struct ql_run {
    int64_t s, best;   // s behind the steps taken so far; the largest s seen
    uint64_t cnt;      // symbols cut: the step behind which best was first reached
    uint32_t stopped;  // s went negative
};
FQ_HD ql_run ql_run_start() { return {0, 0, 0, 0}; }
// this lane's term of steps t0 .. t0 + G - 1 (lane: step t0 + lane); 0 behind the read's end
FQ_HD int32_t ql_run_term(const uint8_t* q, uint32_t L, uint32_t phred_offset, int32_t cutoff, bool from_end, uint64_t t0, uint32_t lane) {
    const uint64_t t = t0 + lane;
    if (t >= L) return 0;
    return cutoff - (int32_t)ql_q(q[from_end ? L - 1 - t : t], phred_offset);
}
// p: the inclusive scan of the terms over the group.  The lane if s goes negative behind its step, else G: the group's
// minimum is the step at which the rule stops.
FQ_HD uint32_t ql_run_neg(const ql_run& st, int32_t p, uint32_t L, uint64_t t0, uint32_t lane, uint32_t G) {
    return t0 + lane < L && st.s + p < 0 ? lane : G;
}
// first_neg: that minimum.  A key whose maximum over the group names the largest p in front of the stop, the first among
// equals: (p + 8192) * 32 + (31 - lane); 0 where the lane's step does not count.
FQ_HD uint32_t ql_run_key(int32_t p, uint32_t L, uint64_t t0, uint32_t lane, uint32_t first_neg) {
    if (t0 + lane >= L || lane >= first_neg) return 0;
    return ((uint32_t)(p + 8192) << 5) | (31u - lane);
}
// key: that maximum; total: p of the last lane.  The state behind the step.
FQ_HD void ql_run_carry(ql_run& st, uint64_t t0, uint32_t first_neg, uint32_t key, int32_t total, uint32_t G) {
    if (key) {
        const int64_t top = st.s + ((int32_t)(key >> 5) - 8192);
        if (top > st.best) {
            st.best = top;
            st.cnt = t0 + (31u - (key & 31u)) + 1;
        }
    }
    st.stopped = first_neg < G;
    st.s += total;
}

// WINDOW.  The window sum at start j is D + (exclusive scan over the group of q[j + W] - q[j]) with D the sum at the step's
// first start; D starts as the sum of q[0 .. W), of which this is a lane's share.
FQ_HD uint64_t ql_win_share(const uint8_t* q, uint32_t W, uint32_t phred_offset, uint32_t lane, uint32_t G) {
    uint64_t s = 0;
    for (uint64_t i = lane; i < W; i += G) s += ql_q(q[i], phred_offset);
    return s;
}
// this lane's term for starts j0 .. j0 + G - 1: q[j + W] - q[j], 0 where j is no start (j + W > L)
FQ_HD int32_t ql_win_term(const uint8_t* q, uint32_t L, uint32_t W, uint32_t phred_offset, uint64_t j0, uint32_t lane) {
    const uint64_t j = j0 + lane;
    if (j + W > L) return 0;
    const int32_t in = j + W < L ? (int32_t)ql_q(q[j + W], phred_offset) : 0;
    return in - (int32_t)ql_q(q[j], phred_offset);
}
// ex: the exclusive scan of the terms.  The lane if its window fails, else G.
FQ_HD uint32_t ql_win_fails(uint64_t D, int32_t ex, uint64_t threshold, uint32_t L, uint32_t W, uint64_t j0, uint32_t lane, uint32_t G) {
    return j0 + lane + W <= L && (uint64_t)((int64_t)D + ex) < threshold ? lane : G;
}
// the walk back from a failing window: the lane if symbol e - 1 - lane ends it (there is none, or it reaches the cutoff)
FQ_HD uint32_t ql_back_stops(const uint8_t* q, uint64_t e, uint32_t phred_offset, uint32_t cutoff, uint32_t lane, uint32_t G) {
    if (lane >= e) return lane;
    return ql_q(q[e - 1 - lane], phred_offset) >= cutoff ? lane : G;
}

// ---- bg_fastq_qual_select -----------------------------------------------------------------------------------------------
FQ_HD bg_qual_stats_t ql_stats_none() { return {0, 0, 0, 0, 0xFFFFFFFFu, 0}; }
FQ_HD void ql_stats_add(bg_qual_stats_t& s, uint8_t c, uint32_t phred_offset, uint32_t low_q, const uint32_t* weight) {
    const uint32_t v = ql_q(c, phred_offset);
    s.sum_q += v;
    s.n_low += v < low_q;
    s.min_q = v < s.min_q ? v : s.min_q;
    if (weight) s.weight_sum += weight[c];
}
// this lane's share: symbols lane, lane + G, ... (len stays 0: the read's length is set by ql_stats_close)
FQ_HD bg_qual_stats_t ql_stats_share(const uint8_t* q, uint32_t L, uint32_t phred_offset, uint32_t low_q, const uint32_t* weight, uint32_t lane,
                                     uint32_t G) {
    bg_qual_stats_t s = ql_stats_none();
    for (uint64_t i = lane; i < L; i += G) ql_stats_add(s, q[i], phred_offset, low_q, weight);
    return s;
}
FQ_HD bg_qual_stats_t ql_stats_merge(const bg_qual_stats_t& a, const bg_qual_stats_t& b) {
    return {a.sum_q + b.sum_q, a.weight_sum + b.weight_sum, 0, a.n_low + b.n_low, a.min_q < b.min_q ? a.min_q : b.min_q, 0};
}
FQ_HD bg_qual_stats_t ql_stats_close(bg_qual_stats_t s, uint32_t L) {
    s.len = L;
    if (L == 0) s.min_q = 0;
    return s;
}
// the serial statement
FQ_HD bg_qual_stats_t ql_stats_serial(const uint8_t* q, uint32_t L, uint32_t phred_offset, uint32_t low_q, const uint32_t* weight) {
    return ql_stats_close(ql_stats_share(q, L, phred_offset, low_q, weight, 0, 1), L);
}
FQ_HD bool ql_passes(const bg_qual_select_t& f, const bg_qual_stats_t& s, bool has_weight) {
    if (s.sum_q < (uint64_t)f.min_mean_q * s.len) return false;
    if (f.max_low_pct < 100u && (uint64_t)s.n_low * 100u > (uint64_t)f.max_low_pct * s.len) return false;
    if (has_weight && s.weight_sum > f.max_weight) return false;
    return true;
}
// the pair rule, the filter's: own / mate say whether the record and (BG_QSEL_PAIRED) its mate pass
FQ_HD bool ql_keeps(uint32_t flags, bool own, bool mate) {
    if (!(flags & BG_QSEL_PAIRED)) return own;
    return (flags & BG_QSEL_PAIR_BOTH) ? (own || mate) : (own && mate);
}
// word i (0 .. 7) of a bg_qual_stats_t
FQ_HD uint32_t ql_stats_word(const bg_qual_stats_t& s, uint32_t i) {
    const uint32_t w[8] = {(uint32_t)s.sum_q, (uint32_t)(s.sum_q >> 32), (uint32_t)s.weight_sum, (uint32_t)(s.weight_sum >> 32), s.len, s.n_low,
                           s.min_q, 0u};
    return w[i];
}

// ---- bg_fastq_qc_tables ---------------------------------------------------------------------------------------------------
// where the five tables start in the buffer, in words; R = max_cycles + 1
FQ_HD uint64_t ql_tab_base(uint32_t max_cycles) { return 0; }
FQ_HD uint64_t ql_tab_qhist(uint32_t max_cycles) { return (uint64_t)(max_cycles + 1) * 5; }
FQ_HD uint64_t ql_tab_len(uint32_t max_cycles) { return (uint64_t)(max_cycles + 1) * 69; }
FQ_HD uint64_t ql_tab_meanq(uint32_t max_cycles) { return ql_tab_len(max_cycles) + max_cycles + 2; }
FQ_HD uint64_t ql_tab_reads(uint32_t max_cycles) { return ql_tab_meanq(max_cycles) + 64; }
FQ_HD uint64_t ql_tab_words(uint32_t max_cycles) { return ql_tab_reads(max_cycles) + 1; }
// the column of `base` a sequence byte counts in
FQ_HD uint32_t ql_base_class(uint8_t c) {
    const uint8_t l = c | 0x20;
    return l == 'a' ? 0u : l == 'c' ? 1u : l == 'g' ? 2u : l == 't' ? 3u : 4u;
}
FQ_HD uint32_t ql_row(uint64_t pos, uint32_t max_cycles) { return pos < max_cycles ? (uint32_t)pos : max_cycles; }

#endif
