// The per-record bodies of fastq_emit.hip (bg_fastq_filter[_dev], bg_fastq_emit[_dev]; rules in include/biogpu.h) as
// __host__ __device__ functions of (record, lane within the group, group width): the kernels call them with the lanes of a
// group, tests/fastq_emit_host_bodies.cpp calls them lane by lane on the CPU under AddressSanitizer.  Every load is a byte
// load at an index inside the run it copies: no lane rounds a source address down to a word, so nothing before a run's first
// or behind its last byte is touched.  Only fq_line_flush accesses memory wide: the destination, whose alignment is known.
#ifndef BG_FASTQ_EMIT_RULE_H
#define BG_FASTQ_EMIT_RULE_H
#include <hip/hip_runtime.h>

#include <cstdint>

#include "biogpu.h"

#define FQ_HD __host__ __device__ inline

// ---- bg_fastq_filter ----------------------------------------------------------------------------------------------------
// "trimmed": some pattern of the read has a hit
FQ_HD bool fq_trimmed(const bg_alignment_t* hits, uint64_t r, uint32_t n_pat) {
    for (uint32_t p = 0; p < n_pat; p++)
        if (hits[r * n_pat + p].score != BG_MIN_SCORE) return true;
    return false;
}
// this lane's share of the 'N' / 'n' bytes of a sequence (the group sums the shares)
FQ_HD uint32_t fq_count_n(const uint8_t* s, uint32_t len, uint32_t lane, uint32_t G) {
    uint32_t c = 0;
    for (uint32_t i = lane; i < len; i += G) c += (s[i] | 0x20) == 'n';
    return c;
}
// every criterion that is switched on holds (n_count is not looked at where max_n is off)
FQ_HD bool fq_passes(const bg_fastq_filter_t& f, uint32_t seq_len, int32_t check, bool trimmed, uint32_t n_count) {
    if (seq_len < f.min_len || seq_len > f.max_len) return false;
    if ((f.flags & BG_FQF_CHECK_OK) && check != BG_FQCHECK_OK) return false;
    if ((f.flags & BG_FQF_DISCARD_UNTRIMMED) && !trimmed) return false;
    if ((f.flags & BG_FQF_DISCARD_TRIMMED) && trimmed) return false;
    if (f.max_n != 0xFFFFFFFFu && n_count > f.max_n) return false;
    return true;
}
// the pair rule: own / mate say whether the record and (BG_FQF_PAIRED) its mate pass
FQ_HD bool fq_keeps(uint32_t flags, bool own, bool mate) {
    if (!(flags & BG_FQF_PAIRED)) return own;
    return (flags & BG_FQF_PAIR_BOTH) ? (own || mate) : (own && mate);
}
// a kept record to its place k: sequence (s, sl bytes) to seq_out + so, qualities to qual_out + qo, lane 0 the record and
// the two offsets
FQ_HD void fq_copy_record(const bg_fastq_record_t& rec, const uint8_t* s, uint32_t sl, const uint8_t* q, uint32_t ql, uint64_t k, uint64_t so,
                          uint64_t qo, bg_fastq_record_t* recs_out, uint8_t* seq_out, uint64_t* seq_off_out, uint8_t* qual_out,
                          uint64_t* qual_off_out, uint32_t lane, uint32_t G) {
    for (uint32_t i = lane; i < sl; i += G) seq_out[so + i] = s[i];
    for (uint32_t i = lane; i < ql; i += G) qual_out[qo + i] = q[i];
    if (lane == 0) {
        bg_fastq_record_t o = rec;
        o.seq_off = so;
        o.qual_off = qo;
        recs_out[k] = o;
        seq_off_out[k] = so;
        qual_off_out[k] = qo;
    }
}

// ---- bg_fastq_emit ------------------------------------------------------------------------------------------------------
// "@id[ desc]\nseq\n+\nqual\n"
FQ_HD uint32_t fq_line_len(const bg_fastq_record_t& r) { return 6 + r.id_len + (r.has_desc ? 1 + r.desc_len : 0) + r.seq_len + r.qual_len; }

// len bytes from src to dst by the G lanes of a group
FQ_HD void fq_copy_run(char* dst, const uint8_t* src, uint32_t len, uint32_t lane, uint32_t G) {
    for (uint32_t i = lane; i < len; i += G) dst[i] = (char)src[i];
}

// One record's text by the G lanes of its group into dst (LDS, global or host memory): the four runs by fq_copy_run, lane 0
// the six bytes between them.
FQ_HD void fq_line_write(const uint8_t* text, const bg_fastq_record_t& r, const uint8_t* seq, const uint8_t* qual, char* dst, uint32_t lane,
                         uint32_t G) {
    const uint32_t desc_at = 1 + r.id_len + 1;                                       // behind '@', the id and the space
    const uint32_t nl_at = r.has_desc ? desc_at + r.desc_len : 1 + r.id_len;          // the header's newline
    const uint32_t seq_at = nl_at + 1, qual_at = seq_at + r.seq_len + 3;
    fq_copy_run(dst + 1, text + r.id_off, r.id_len, lane, G);
    if (r.has_desc) fq_copy_run(dst + desc_at, text + r.desc_off, r.desc_len, lane, G);
    fq_copy_run(dst + seq_at, seq + r.seq_off, r.seq_len, lane, G);
    fq_copy_run(dst + qual_at, qual + r.qual_off, r.qual_len, lane, G);
    if (lane == 0) {
        dst[0] = '@';
        if (r.has_desc) dst[desc_at - 1] = ' ';
        dst[nl_at] = '\n';
        dst[qual_at - 3] = '\n';
        dst[qual_at - 2] = '+';
        dst[qual_at - 1] = '\n';
        dst[qual_at + r.qual_len] = '\n';
    }
}

struct alignas(16) fq_b16 {
    uint32_t w[4];
};
// A staged line to its place: `stage` holds the line at the same offset inside a 16-byte granule that `line` has, so the
// bytes up to the first 16-byte boundary and behind the last one leave singly and everything between as 16-byte stores.
FQ_HD void fq_line_flush(const char* stage, char* line, uint32_t len, uint32_t lane, uint32_t G) {
    const uint32_t mis = (uint32_t)((uintptr_t)line & 15);
    const uint32_t to_boundary = (16 - mis) & 15;
    const uint32_t head = len < to_boundary ? len : to_boundary;
    const uint32_t body = (len - head) >> 4, tail = (len - head) & 15;
    for (uint32_t i = lane; i < head; i += G) line[i] = stage[i];
    for (uint32_t i = lane; i < body; i += G) *(fq_b16*)(line + head + 16 * i) = *(const fq_b16*)(stage + head + 16 * i);
    for (uint32_t i = lane; i < tail; i += G) line[head + 16 * body + i] = stage[head + 16 * body + i];
}

#endif
