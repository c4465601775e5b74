// The five columns parsed FASTQ records travel in — recs, seq, seq_off, qual, qual_off — as one value on the host side of
// bg_fastq_trim, bg_fastq_filter and bg_fastq_demux_split, their passage through a bg_stage, and the two counts the FASTQ and
// SAM host entry points share.  Host code only.
#ifndef BG_FASTQ_COLS_H
#define BG_FASTQ_COLS_H
#include <algorithm>

#include "bg_common.h"

struct fq_cols_in {
    const bg_fastq_record_t* recs;  // [n]
    const uint8_t* seq;
    const uint64_t* seq_off;  // [n + 1]
    const uint8_t* qual;
    const uint64_t* qual_off;  // [n + 1]
    bool complete() const { return recs && seq && seq_off && qual && qual_off; }
};
struct fq_cols_out {
    bg_fastq_record_t* recs;
    uint8_t* seq;
    uint64_t* seq_off;
    uint8_t* qual;
    uint64_t* qual_off;
    bool offsets() const { return seq_off && qual_off; }
    bool data() const { return recs && seq && qual; }
};

// device copies of n records' columns; nothing of the caller's is read where n is 0
inline fq_cols_in fq_cols_upload(bg_stage& s, uint64_t n, const fq_cols_in& h) {
    const size_t off = n ? (size_t)n + 1 : 0;
    return {s.up(h.recs, n), s.up(h.seq, n ? h.seq_off[n] : 0), s.up(h.seq_off, off), s.up(h.qual, n ? h.qual_off[n] : 0), s.up(h.qual_off, off)};
}
// device columns for up to n records of seq_bytes and qual_bytes in all
inline fq_cols_out fq_cols_alloc(bg_stage& s, uint64_t n, uint64_t seq_bytes, uint64_t qual_bytes) {
    return {s.out<bg_fastq_record_t>(n), s.out<uint8_t>(seq_bytes), s.out<uint64_t>((size_t)n + 1), s.out<uint8_t>(qual_bytes),
            s.out<uint64_t>((size_t)n + 1)};
}
// the first n_recs records of d, their n_recs + 1 offsets and their bytes into the caller's columns h
inline void fq_cols_download(bg_stage& s, const fq_cols_out& h, const fq_cols_out& d, uint64_t n_recs, uint64_t seq_bytes, uint64_t qual_bytes) {
    s.down(h.recs, d.recs, n_recs);
    s.down(h.seq, d.seq, seq_bytes);
    s.down(h.qual, d.qual, qual_bytes);
    s.down(h.seq_off, d.seq_off, (size_t)n_recs + 1);
    s.down(h.qual_off, d.qual_off, (size_t)n_recs + 1);
}

// how many of the records first, first + step, ... are below n
inline uint64_t fq_strided_count(uint64_t n, uint64_t first, uint64_t step) { return first < n ? (n - first - 1) / step + 1 : 0; }

// Where the buffers that those records point into end: each where the last of them ends (ids and descriptions in the FASTQ
// text, a description only where the record has one).  The step is taken so that r + step never passes n or wraps.
struct fq_extents {
    uint64_t id = 0, desc = 0, seq = 0, qual = 0;
};
inline fq_extents fq_record_extents(const bg_fastq_record_t* recs, uint64_t n, uint64_t first = 0, uint64_t step = 1) {
    fq_extents e;
    for (uint64_t r = first; r < n; r += step) {
        e.id = std::max<uint64_t>(e.id, recs[r].id_off + recs[r].id_len);
        if (recs[r].has_desc) e.desc = std::max<uint64_t>(e.desc, recs[r].desc_off + recs[r].desc_len);
        e.seq = std::max<uint64_t>(e.seq, recs[r].seq_off + recs[r].seq_len);
        e.qual = std::max<uint64_t>(e.qual, recs[r].qual_off + recs[r].qual_len);
        if (n - r <= step) break;
    }
    return e;
}

#endif
