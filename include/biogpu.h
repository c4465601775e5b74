/*
 * biogpu.h — C ABI of the MI355X-native engine that sits behind rust-bio's
 *   bio::alignment::pairwise::Aligner            (src/alignment/pairwise/mod.rs:472-1016)
 *   bio::alignment::pairwise::banded::Aligner    (src/alignment/pairwise/banded.rs:122-1004)
 *   bio::data_structures::fmindex::FMIndex       (src/data_structures/fmindex.rs:98-248)
 * and the host-side table builders they are fed from
 *   suffix_array / bwt / less / Occ::new         (suffix_array.rs:264, bwt.rs:39,186,94).
 *
 * rust-bio has no FFI of its own; these are the entry points a Rust shim
 * inside `bio` binds with `extern "C"` (INTEGRATION.md shows the binding).  Plain pointers
 * and sizes only.  Every function returns BG_OK (0) or a negative bg_status; nothing panics
 * or throws across the boundary.  Where the reference would `panic!` (assert on positive
 * penalties, index-out-of-bounds on a byte outside the alphabet, missing sentinel) the
 * matching error code is returned and documented at the function.
 *
 * Two flavours per batched op:
 *   bg_*_batch      caller passes HOST buffers (the drop-in boundary; includes PCIe copies)
 *   bg_*_batch_dev  caller passes DEVICE pointers + a hipStream_t (as void*): inputs already
 *                   resident in HBM, results left in HBM, asynchronous on that stream.
 *
 * Streams and threads.  A bg_ctx owns ONE set of device scratch (traceback words, aux records, scoring table).
 * *_dev calls that use it may be issued on different streams: a call arriving on another stream than the
 * previous one first waits, on the device, for that call's last kernel (an event per ctx), so two calls in
 * flight never share scratch — they serialise.  For real overlap use one bg_ctx per stream.  A bg_ctx must
 * not be used from two host threads at once (like `&mut Aligner`).  A bg_fm is immutable after bg_fm_build /
 * bg_fm_set_*; bg_fm_backward_search_batch_dev, bg_sa_get_batch_dev and bg_interval_occ_batch_dev use no ctx
 * scratch and may be called from several threads on their own streams (with bg_enable_timing off — the timing
 * events belong to the ctx); the host-buffer flavours and bg_fmd_smems_* go through the handle's ctx and share
 * its single-thread rule.
 *
 * Several GPUs.  One process (and one bg_ctx, one replica of a bg_fm) per device; pairs / queries / reads are split in
 * contiguous ranges and nothing is exchanged during a call.  What a caller gathers afterwards (one all-gather) are the
 * FIXED-SIZE results: bg_alignment_t headers (score + coordinates), search intervals + tags, bg_seed_hit_t headers.
 * Operation lists are variable-length and ops_off indexes the buffer of the process that made them: they stay where
 * they are unless the caller gathers byte counts (ops_used) and bytes itself and re-bases ops_off.
 *
 * Text positions are 64-bit at the boundary, like the reference's usize (fmindex.rs:70-71, bwt.rs:94, suffix_array.rs:
 * 264).  Inside, an index below 2^32 - 1 symbols keeps the uint32 layout of rounds 1-4 (and its speed); from 2^32 - 1
 * symbols on — T$R$ of a human genome for an FMD index is 6.2 G — bg_fm_build / bg_fm_build_dev lay the SAME rank blocks
 * out with superblock-relative counters and 64-bit bases (csrc/fm_kernels.h) and every entry point that takes a bg_fm works
 * on them: backward search with byte or 2-bit packed patterns (2-step blocks included), bg_fm_set_[sampled_]suffix_array,
 * bg_sa_get_batch[_dev], bg_interval_occ_batch[_dev], bg_fm_set_text + bg_seed_extend_batch[_dev], bg_fm_save / bg_fm_load,
 * and the FMD kernels through their *64 entry points (bg_fmd_smems_batch64[_dev], bg_fmd_interval_batch64: uint64 records;
 * the uint32-record flavours answer BG_ERR_UNSUPPORTED on such an index, the *64 flavours serve both layouts).
 * bg_suffix_array_dev64 / bg_bwt_dev64 / bg_sa_sample_dev64 build the 64-bit suffix array in HBM.  BG_ERR_TOO_LARGE only
 * beyond 2^40 symbols.  The one thing a 64-bit index does NOT offer (BG_ERR_UNSUPPORTED at build time): BWTs with more
 * than 1024 positions outside their four most frequent bytes (protein texts, genomes with long N runs: they would need
 * rank bit vectors with 64-bit bases); bg_fm_backward_search_count_lines_dev is a measurement aid of the 32-bit kernels.
 * A sequence of an aligner call may have up to 2^24 symbols.
 */
#ifndef BIOGPU_H
#define BIOGPU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    BG_OK = 0,
    BG_ERR_INVALID_ARG = -1,
    BG_ERR_NO_DEVICE = -2,       /* no usable HIP device / extension cannot run */
    BG_ERR_HIP = -3,             /* a HIP runtime call failed (see bg_last_error) */
    BG_ERR_OOM = -4,
    BG_ERR_SENTINEL = -5,        /* suffix_array.rs:431-437 assert: last byte must be the smallest */
    BG_ERR_POSITIVE_PENALTY = -6,/* pairwise/mod.rs:265-266,292-293,554-571 asserts */
    BG_ERR_OUT_OF_ALPHABET = -7, /* fmindex.rs:229 / bwt.rs:114,158 index-out-of-bounds panics */
    BG_ERR_TOO_LARGE = -8,       /* text > 2^40 symbols (>= 2^32 - 1 for the uint32 suffix-array flavours), or sequence too long for the engine */
    BG_ERR_OPS_CAP = -9,         /* caller's ops buffer too small (ops_used reports the need) */
    BG_ERR_TRACEBACK = -10,      /* traceback did not terminate (reference would loop forever) */
    BG_ERR_UNSUPPORTED = -11,    /* legal for rust-bio, not yet covered by the device layout */
    BG_ERR_IO = -12              /* bg_fm_save / bg_fm_load: the file cannot be opened, is truncated, or fails its checksum */
} bg_status;

#define BG_MIN_SCORE (-858993459) /* pairwise::MIN_SCORE, mod.rs:174 */

typedef struct bg_ctx bg_ctx; /* one per device; not thread-safe (like `&mut Aligner`) */
typedef struct bg_fm bg_fm;   /* device-resident FM index; immutable after construction (like Arc<FMIndex>): see "Streams and threads" */

int bg_device_count(void);
int bg_init(int device, bg_ctx** out);
int bg_free(bg_ctx* ctx);
const char* bg_strerror(int status);
const char* bg_last_error(void); /* text of the last HIP failure on this thread */
/* Tunables (0 keeps the default) and the switches the tests use to reach every kernel variant:
 *   chunk_pairs        pairs per sub-batch of bg_align_batch_dev (default 2^20) and of the banded pipeline (16384)
 *   host_chunk_pairs   pairs per stage of bg_align_batch's pipelined host path (122880)
 *   seed_chunk_reads   reads per pass of bg_seed_extend[_strands|_pairs|_multi]_batch[_dev] (0: equal passes of at most 2^21
 *                      reads, 2^20 with both strands and with pairs; pairs round it down to an even count, at least 2)
 *   force_wide = 1     scores kept as plain int32 even where they fit the 24-bit keys of the fast kernels
 *   no_pk16 = 1        no packed-int16 fill (K1p): the int32 kernel K1 runs for every batch
 *   no_couples = 1     K1p without the (m, n) slot order on ragged batches
 *   no_local_fast = 1  Aligner::local batches on the general K1p instead of its LF flavour (tests, A/B)
 *   fm_host_bytes = 1  bg_fm_backward_search_batch stages the pattern bytes as they are (default: packed to 2-bit codes by
 *                      the host threads where the index takes packed patterns; tests, A/B)
 *   band_on_host = 1   bands built by the host threads instead of the device builder
 *   band_fill_v1       1: banded fill with one pair per wavefront (K3) always; -1: eight pairs per wavefront (K3v2)
 *                      always; 0 (default): K3 for sub-batches of at most 2048 pairs (latency), K3v2 above (throughput)
 *   band_interior_off = 1  banded fill (K3v2) with its general step in every strip (tests, A/B: no reduced interior step)
 *   band_packed_off = 1    interior runs on the int32 kernel (K3i) only: no packed-int16 kernel (K3p) in front of it
 *   band_packed_thresh     K3p's detect-and-recompute threshold in key units (score * 16); 0 = derived from the scoring,
 *                          65535 = every pair is flagged and recomputed by the int32 kernels (tests)
 *   band_chain_global  chaining tree placement: 0 LDS, 1 global scratch, -1 by batch size (default)
 *   band_join_global = 1  k-mer join with its table in global memory even where the LDS flavour applies
 *   band_chain_rows    global-tree chaining with four pairs per wavefront (chain_rows_kernel; default 1) or one (0: A/B, tests)
 *   fm_wide_from       texts of this many symbols or more get the 64-bit index layout (default 2^32 - 1; tests lower it so
 *                      that small texts exercise that layout); 0 restores the default
 *   fm_wide_sb_shift   log2 of the rank blocks per superblock of the 64-bit layout (default 17; 0 .. 24; tests use small
 *                      values so that short texts span many superblocks)
 *   fq_no_fused = 1    bg_fastq_parse[_dev] through its general multi-pass kernels only, without the one-pass kernel that serves
 *                      four-line ASCII records in front (tests, A/B)
 *   sam_lanes          lanes that format one line in bg_sam_emit_batch_dev's write pass: 16 or 32 (0 = default; tests, A/B: the
 *                      text does not depend on it)
 *   fq_emit_mode       bg_fastq_emit_dev's text pass: 1 byte stores straight to the output, 2 lines staged in LDS and stored 16
 *                      bytes wide (0 = default, which is 1; tests, A/B: the text does not depend on it)
 *   indels_stop_after  bg_bam_indels_dev and bg_bam_indels_left_dev return BG_OK with no event after 1 the count pass, 2 the emit
 *                      pass, 3 the sort (0 = default: they run through; A/B only: timing tells the passes apart by differences
 *                      of whole calls)
 *   sa_chunk_symbols   suffixes sorted per pass of round 0 of bg_suffix_array_dev[64] (0 = derived from free device memory;
 *                      tests use small values so that short texts take several passes)
 *   band_budget_gb     traceback + aux bytes per scratch set of the banded pipeline, in GB (0 = default: 40, and never more
 *                      than a third of the device's free memory); a sub-batch that does not fit is cut
 *   myers_chunk_jobs   jobs per launch of bg_myers_*_batch[_dev] (0 = by a 256 MB budget for the traceback columns; tests use
 *                      small values so that small batches take several launches)
 *   myers_lds_bytes    LDS bytes the pattern tables of one group of bg_myers_*_batch[_dev] may take (0 = 48 KB; 4096 .. 65536;
 *                      tests lower it so that a few patterns need two groups)
 * Unknown keys return BG_ERR_INVALID_ARG. */
int bg_set_option(bg_ctx* ctx, const char* key, int64_t value);

/* ------------------------------------------------------------------ host table builders
 * Same contracts as the reference functions; pure host code (usable without a GPU). */

/* suffix_array(text) — suffix_array.rs:264-284.  text must end in a sentinel <= every other
 * byte, else BG_ERR_SENTINEL (the reference asserts).  Several sentinels are ordered by
 * position: the first occurrence sorts last among them (transform_text, 444-466). */
int bg_suffix_array(const uint8_t* text, uint64_t n, uint64_t* sa_out);
/* bwt(text, pos) — bwt.rs:39-49 */
int bg_bwt(const uint8_t* text, const uint64_t* sa, uint64_t n, uint8_t* bwt_out);
/* less(bwt, alphabet) — bwt.rs:186-199.  less_out must hold max_symbol+2 entries;
 * *less_len receives that length (call with less_out == NULL to query it). */
int bg_less(const uint8_t* bwt, uint64_t n, const uint8_t* alphabet, uint32_t n_sym,
            uint64_t* less_out, uint32_t* less_len);

/* Device flavours for a text that already lives in HBM (sa_build.hip): suffix array by prefix doubling (radix sorts
 * of (rank, rank) keys), n uint32 entries; BWT gather; RawSuffixArray::sample (suffix_array.rs:86-120) with the
 * samples and the sentinel rows returned to host arrays (what bg_fm_set_sampled_suffix_array takes: sample holds
 * ceil(n / rate) entries, extra rows come back sorted, *n_extra says how many; BG_ERR_OPS_CAP beyond extra_cap).
 * The results equal the host functions' (the suffix array of the transformed text is unique), also for texts whose
 * sentinel byte occurs several times — several sequences, or T$R$ for an FMD index (fmindex.rs:312-340): the sentinels
 * rank by position, the last occurrence smallest (transform_text, suffix_array.rs:444-466).  The uint32 flavours take
 * texts up to 2^32 - 2 symbols (BG_ERR_TOO_LARGE beyond) with about 29 bytes of device scratch per symbol; the *64
 * flavours are the same algorithm on uint64 positions (suffix_array.rs:264: usize) for texts up to 2^40 symbols, 49 bytes
 * of scratch per symbol (a 4.4 G-symbol text: 216 GB next to its 35 GB suffix array on the 288 GB part).  Synchronous. */
int bg_suffix_array_dev(bg_ctx* ctx, const uint8_t* d_text, uint64_t n, uint32_t* d_sa, void* stream);
int bg_bwt_dev(bg_ctx* ctx, const uint8_t* d_text, const uint32_t* d_sa, uint64_t n, uint8_t* d_bwt, void* stream);
int bg_sa_sample_dev(bg_ctx* ctx, const uint32_t* d_sa, const uint8_t* d_bwt, uint64_t n, uint32_t sampling_rate,
                     uint8_t sentinel, uint64_t* sample, uint64_t* extra_rows, uint64_t* extra_pos, uint64_t extra_cap,
                     uint64_t* n_extra, void* stream);
int bg_suffix_array_dev64(bg_ctx* ctx, const uint8_t* d_text, uint64_t n, uint64_t* d_sa, void* stream);
int bg_bwt_dev64(bg_ctx* ctx, const uint8_t* d_text, const uint64_t* d_sa, uint64_t n, uint8_t* d_bwt, void* stream);
int bg_sa_sample_dev64(bg_ctx* ctx, const uint64_t* d_sa, const uint8_t* d_bwt, uint64_t n, uint32_t sampling_rate,
                       uint8_t sentinel, uint64_t* sample, uint64_t* extra_rows, uint64_t* extra_pos, uint64_t extra_cap,
                       uint64_t* n_extra, void* stream);

/* ------------------------------------------------------------------ FM index
 * bg_fm_build replaces `Occ::new(&bwt, k, &alphabet)` + `FMIndex::new(bwt, less, occ)`
 * (bwt.rs:94-125, fmindex.rs:245-247): the sampled-Occ table layout on the device is the
 * engine's own, `occ_k` is accepted for API fidelity and only validated (>= 1):
 * Occ::get's result does not depend on k.  The reference's third argument, the host-built `Occ` table itself,
 * is deliberately NOT part of this signature: the engine ranks on its own packed blocks built from `bwt`, so a
 * Rust shim drops its `Occ` (or never builds it) and passes (bwt, less, k, alphabet) — INTEGRATION.md.  BG_ERR_OUT_OF_ALPHABET when a BWT byte exceeds
 * the alphabet's max symbol (Occ::new would panic, bwt.rs:114).  The BWT is uploaded and the index laid out on the device
 * (the builder of bg_fm_build_dev, with the caller's `less` kept): while the call runs it needs n bytes of device memory
 * for the uploaded BWT plus the builder's count and scan temporaries (about n / 6 bytes), on top of the index; both are
 * freed before it returns.  Synchronous. */
int bg_fm_build(bg_ctx* ctx, const uint8_t* bwt, uint64_t n, const uint64_t* less,
                uint32_t less_len, uint32_t occ_k, const uint8_t* alphabet, uint32_t n_sym,
                bg_fm** out);
/* The same index from a BWT that lives in HBM (with bg_suffix_array_dev / bg_bwt_dev: text to searchable index
 * without a host copy of anything text-sized).  `less(bwt, alphabet)` (bwt.rs:186-199) falls out of the byte
 * histogram the layout needs anyway: it is computed here and, if less_out is given (max_symbol + 2 entries),
 * returned.  Identical handle to bg_fm_build's on the same BWT.  Synchronous. */
int bg_fm_build_dev(bg_ctx* ctx, const uint8_t* d_bwt, uint64_t n, uint32_t occ_k, const uint8_t* alphabet,
                    uint32_t n_sym, uint64_t* less_out, bg_fm** out, void* stream);
int bg_fm_free(bg_fm* fm);
uint64_t bg_fm_device_bytes(const bg_fm* fm);
/* Index persistence.  The reference derives Serialize / Deserialize for Occ (bwt.rs:76), FMIndex (fmindex.rs:214) and
 * SampledSuffixArray (suffix_array.rs:124): an index is built once per genome and loaded afterwards.  bg_fm_save writes what
 * the reference's FMIndex holds — the BWT (read back out of the rank blocks), less, the alphabet and k — plus the suffix
 * array attached to the handle (raw, or sampled with its extra rows) and the text if the handle owns a copy
 * (bg_fm_set_text); bg_fm_load lays the index out again (the rank blocks are cheap: csrc/fm_persist.hip) and attaches
 * them: the loaded handle answers every call like the saved one.  The file is the engine's own format (little-endian,
 * checksummed), not serde's.  BG_ERR_IO: cannot open / truncated / altered. */
int bg_fm_save(const bg_fm* fm, const char* path);
int bg_fm_load(bg_ctx* ctx, const char* path, bg_fm** out);
/* What a handle says about itself — a loaded handle comes without the caller-side arrays it was built from, and the
 * reference's FMDIndex::from(fmindex) (fmindex.rs:311-329) reads the BWT of whatever FMIndex it is given, deserialized
 * or not.  bg_fm_len: the text length n (FMIndex's bwt.len()).  bg_fm_less: the `less` array the index answers with
 * (less_out may be NULL to query *less_len = max_symbol + 2).  bg_fm_bwt / bg_fm_bwt_dev: the n BWT bytes, read back
 * out of the rank blocks (2-bit codes -> bytes, listed exceptions put back) into host / device memory; the device
 * flavour is asynchronous on `stream`. */
int bg_fm_len(const bg_fm* fm, uint64_t* n);
int bg_fm_less(const bg_fm* fm, uint64_t* less_out, uint32_t* less_len);
int bg_fm_bwt(const bg_fm* fm, uint8_t* bwt);
int bg_fm_bwt_dev(const bg_fm* fm, uint8_t* d_bwt, void* stream);
/* Bytes of the index's 2-step rank blocks (128-byte lines: 16 pair counters + 128 four-bit pair codes per 128 BWT
 * positions; built behind DNA-like indexes whose `less` is the BWT's own, fm_step2.hip) that the searches take two
 * pattern symbols per block access from; 0: single steps (no such blocks, or bg_fm_set_option "no_step2" = 1). */
uint64_t bg_fm_step2_bytes(const bg_fm* fm);

/* Result tags of FMIndexable::backward_search (fmindex.rs:92-96). */
enum { BG_FM_COMPLETE = 0, BG_FM_PARTIAL = 1, BG_FM_ABSENT = 2,
       BG_FM_PANIC = 3 /* this query reached a byte outside the alphabet */ };

/* Options of an index handle (tests, A/B): "no_step2" = 1 — single LF steps even where the index has 2-step blocks;
 * "no_fast" = 1 — every search through the generic kernel alone.  Neither changes a result.  Any other key:
 * BG_ERR_INVALID_ARG. */
int bg_fm_set_option(bg_fm* fm, const char* key, int64_t value);

/* backward_search for n_q patterns (fmindex.rs:144-208).  Pattern q is
 * pat[pat_off[q] .. pat_off[q+1]).  Outputs per query: tag, Interval{lower,upper} (for
 * Partial: the interval of the maximal matching suffix), matched_len (Complete: |P|).
 * Returns BG_ERR_OUT_OF_ALPHABET if any query has tag BG_FM_PANIC (all other queries are
 * still valid). */
int bg_fm_backward_search_batch(bg_fm* fm, uint64_t n_q, const uint8_t* pat,
                                const uint64_t* pat_off, uint8_t* tag, uint64_t* lower,
                                uint64_t* upper, uint32_t* matched_len);
/* Same with device pointers; asynchronous on `stream`; no panic scan (tags tell). */
int bg_fm_backward_search_batch_dev(bg_fm* fm, uint64_t n_q, const uint8_t* d_pat,
                                    const uint64_t* d_pat_off, uint8_t* d_tag, uint64_t* d_lower,
                                    uint64_t* d_upper, uint32_t* d_matched_len, void* stream);

/* ---- 2-bit packed sequences (pack2.hip) ---------------------------------------------------------
 * rust-bio's Aligner and FMIndex take `&[u8]` (pairwise/mod.rs:591, fmindex.rs:144); the engine also accepts its own
 * 2-bit wire format, what BASELINE's north_star calls "packed 2-bit reads".  A byte buffer — any concatenation of
 * sequences, e.g. the `seq` buffer bg_fastq_parse_dev fills — is packed as ONE stream: symbol s sits in bits
 * 2 (s % 16) .. + 1 of little-endian dword s / 16, `codes[c]` is the byte value of code c (four distinct bytes).
 * Sequence boundaries do not matter to the packing: the offset arrays of the byte flavours (x_off / pat_off /
 * seq_off, in symbols) address the packed stream unchanged.  d_packed must hold (n + 15) / 16 + 1 dwords (consumers
 * may read one dword past the last symbol; its content is never interpreted).  A byte that is none of the four
 * codes is stored as code 0 and counted in *d_n_invalid (a device counter the caller zeroes; may be NULL): a buffer
 * with a non-zero count must take the byte entry points.  Asynchronous on `stream`. */
/* d_bytes (and bg_unpack2_dev's output) may be at any address: a whole word at a 16-byte aligned address is one vector load, any
 * other address byte by byte. */
int bg_pack2_dev(bg_ctx* ctx, const uint8_t* d_bytes, uint64_t n, const uint8_t* codes, uint32_t* d_packed,
                 uint64_t* d_n_invalid, void* stream);
int bg_unpack2_dev(bg_ctx* ctx, const uint32_t* d_packed, uint64_t n, const uint8_t* codes, uint8_t* d_bytes,
                   void* stream);
/* The same packing on the host (no GPU involved; AVX2 where the CPU has it): `packed` must hold (n + 15) / 16 dwords.
 * Returns 1 if every byte was one of the four codes, 0 if not (such bytes are stored as whatever their low bits say:
 * take the byte entry points), a negative BG_ERR_* for bad arguments.  bg_fm_backward_search_batch packs its stages
 * with it on the worker threads. */
int bg_pack2_host(const uint8_t* bytes, uint64_t n, const uint8_t* codes, uint32_t* packed);
/* The byte values of the index's four 2-bit codes — the `codes` to pack its patterns with.  BG_ERR_UNSUPPORTED when
 * the text has fewer than four frequent letters or symbols ranked by bit vectors: such an
 * index takes byte patterns only.  (Both position widths.) */
int bg_fm_pattern_codes(const bg_fm* fm, uint8_t* codes);
/* bg_fm_backward_search_batch_dev on patterns packed with bg_fm_pattern_codes' codes; d_sym_off[q] is the SYMBOL
 * offset of pattern q in the stream (n_q + 1 entries).  Same outputs.  (A dword load per 16 steps instead of a byte
 * load per step, no symbol-class lookups: measured against the byte flavour in bench.py's `fm.packed2`.) */
int bg_fm_backward_search_packed_dev(bg_fm* fm, uint64_t n_q, const uint32_t* d_packed, const uint64_t* d_sym_off,
                                     uint8_t* d_tag, uint64_t* d_lower, uint64_t* d_upper, uint32_t* d_matched_len,
                                     void* stream);
/* Measurement aid: bg_fm_backward_search_batch_dev with the 64-byte block loads it issues counted (*lines_out, host
 * memory; synchronous).  bench.py sets the count against the chip's measured ceiling for such gathers
 * (tools/microbench/ub_gather64.hip). */
int bg_fm_backward_search_count_lines_dev(bg_fm* fm, uint64_t n_q, const uint8_t* d_pat, const uint64_t* d_pat_off,
                                          uint8_t* d_tag, uint64_t* d_lower, uint64_t* d_upper, uint32_t* d_matched_len,
                                          uint64_t* lines_out, void* stream);

/* ---- suffix-array lookups for FM-index hits (kernel K6) ------------------------------------
 * Attach the suffix array the FM index was built from, then resolve rows to text positions.
 * The index handle must come from bg_fm_build over the same text (n rows). */
#define BG_SA_NONE 0xFFFFFFFFFFFFFFFFull  /* SuffixArray::get -> None (row >= len) */
#define BG_SA_PANIC 0xFFFFFFFFFFFFFFFEull /* the reference would panic (missing extra row / non-alphabet byte) */

/* RawSuffixArray (suffix_array.rs:25, get 134-141): the full SA, n entries */
int bg_fm_set_suffix_array(bg_fm* fm, const uint64_t* sa, uint64_t n);
/* SampledSuffixArray as RawSuffixArray::sample builds it (suffix_array.rs:86-120): sample[i] =
 * SA[i * sampling_rate], n_sample = ceil(n / rate); sentinel = last byte of the text; the rows
 * whose BWT byte is the sentinel and that are not sampled, sorted by row, with their positions
 * (`extra_rows`, a hash map in the reference). */
int bg_fm_set_sampled_suffix_array(bg_fm* fm, const uint64_t* sample, uint64_t n_sample,
                                   uint32_t sampling_rate, uint8_t sentinel,
                                   const uint64_t* extra_rows, const uint64_t* extra_pos,
                                   uint64_t n_extra);
/* SuffixArray::get for a batch of rows (suffix_array.rs:134-141 raw, 157-184 sampled):
 * pos[i] = SA[index[i]], BG_SA_NONE if index[i] >= n.  Returns BG_ERR_OUT_OF_ALPHABET if any
 * row hit BG_SA_PANIC. */
int bg_sa_get_batch(bg_fm* fm, uint64_t n_idx, const uint64_t* index, uint64_t* pos);
int bg_sa_get_batch_dev(bg_fm* fm, uint64_t n_idx, const uint64_t* d_index, uint64_t* d_pos,
                        void* stream);
/* Interval::occ for a batch (fmindex.rs:75-79): positions of interval v are written to
 * pos[out_off[v] .. out_off[v+1]) in row order; out_off (n_iv + 1 entries) is filled by the call.
 * BG_ERR_INVALID_ARG if an interval exceeds the suffix array (the reference's expect() panic),
 * BG_ERR_OPS_CAP if pos_cap is too small (out_off is still filled). */
int bg_interval_occ_batch(bg_fm* fm, uint64_t n_iv, const uint64_t* lower, const uint64_t* upper,
                          uint64_t* out_off, uint64_t* pos, uint64_t pos_cap);
/* Device flavour: the caller supplies the prefix offsets (exclusive scan of upper - lower) and
 * their total; asynchronous on `stream`. */
int bg_interval_occ_batch_dev(bg_fm* fm, uint64_t n_iv, const uint64_t* d_lower,
                              const uint64_t* d_out_off, uint64_t total, uint64_t* d_pos,
                              void* stream);

/* ---- FMD index: supermaximal exact matches (kernel K7) ---------------------------------------
 * FMDIndex::smems(pattern, i, l) (fmindex.rs:363-434; all == 0, i_pos[q] = i) or
 * FMDIndex::all_smems(pattern, l) (479-501; all != 0, i_pos may be NULL) for a batch of patterns.
 * The index must have been built (bg_fm_build) over T$R$-style text whose BWT is a word over
 * dna::n_alphabet() + '$' — FMDIndex::from's assert (323-327), else BG_ERR_UNSUPPORTED.
 * Pattern q's matches are the records out[(q*cap + t)*6 ..], t < min(count[q], cap), six uint32:
 * BiInterval {lower, lower_rev, size, match_size}, position on the pattern, SMEM length — in the
 * order the reference pushes them.  count[q] == 0xFFFFFFFF where the reference would panic
 * (BG_ERR_OUT_OF_ALPHABET); BG_ERR_OPS_CAP if some count exceeds cap. */
int bg_fmd_smems_batch(bg_fm* fm, int all, uint64_t n_p, const uint8_t* pat, const uint64_t* pat_off,
                       const uint32_t* i_pos, uint32_t min_len, uint32_t cap, uint32_t* count,
                       uint32_t* out);
/* Single bi-interval steps for a batch of requests: op[q] = 0 init_interval (fmindex.rs:517-524),
 * 1 init_interval_with(sym[q]) (504-514), 2 backward_ext(iv_in[q], sym[q]) (527-558), 3 forward_ext
 * (560-564).  Intervals are four uint32 {lower, lower_rev, size, match_size}. */
int bg_fmd_interval_batch(bg_fm* fm, uint64_t n_req, const uint8_t* op, const uint32_t* iv_in,
                          const uint8_t* sym, uint32_t* iv_out);
int bg_fmd_smems_batch_dev(bg_fm* fm, int all, uint64_t n_p, const uint8_t* d_pat,
                           const uint64_t* d_pat_off, const uint32_t* d_i_pos, uint32_t min_len,
                           uint32_t max_pattern_len, uint32_t cap, uint32_t* d_count, uint32_t* d_out,
                           void* stream);
/* The same three with uint64 records — the reference's BiInterval is usize throughout (fmindex.rs:254-259) — for any
 * index, and the only flavour an index with 64-bit positions answers (T$R$ of a human genome: 6.2 G symbols): six uint64
 * per match {lower, lower_rev, size, match_size, position, length}, four per interval. */
int bg_fmd_smems_batch64(bg_fm* fm, int all, uint64_t n_p, const uint8_t* pat, const uint64_t* pat_off,
                         const uint32_t* i_pos, uint32_t min_len, uint32_t cap, uint32_t* count,
                         uint64_t* out);
int bg_fmd_interval_batch64(bg_fm* fm, uint64_t n_req, const uint8_t* op, const uint64_t* iv_in,
                            const uint8_t* sym, uint64_t* iv_out);
int bg_fmd_smems_batch64_dev(bg_fm* fm, int all, uint64_t n_p, const uint8_t* d_pat,
                             const uint64_t* d_pat_off, const uint32_t* d_i_pos, uint32_t min_len,
                             uint32_t max_pattern_len, uint32_t cap, uint32_t* d_count, uint64_t* d_out,
                             void* stream);

/* ------------------------------------------------------------------ pairwise alignment */

/* Scoring<F> (pairwise/mod.rs:238-247) as the *effective* values `custom` sees.  match_fn is
 * MatchParams{match_score,mismatch_score} when matrix == NULL, else the closure tabulated by
 * the host: matrix[a*256+b] = F(a,b) (int32[65536]).  match_scores_some mirrors
 * `match_scores: Option<(i32,i32)>`, read only by the banded aligner (banded.rs:1315-1318). */
typedef struct {
    int32_t gap_open, gap_extend;
    int32_t xclip_prefix, xclip_suffix, yclip_prefix, yclip_suffix;
    int32_t match_score, mismatch_score;
    int32_t match_scores_some;
    const int32_t* matrix;
} bg_scoring_t;

/* AlignmentMode (bio-types) */
enum { BG_MODE_CUSTOM = 0, BG_MODE_GLOBAL = 1, BG_MODE_SEMIGLOBAL = 2, BG_MODE_LOCAL = 3 };
/* AlignmentOperation, one byte each in the ops buffer.  Xclip/Yclip lengths are the
 * entries of bg_alignment_t.clip_len, in the order the clip ops appear. */
enum { BG_OP_MATCH = 0, BG_OP_SUBST = 1, BG_OP_DEL = 2, BG_OP_INS = 3, BG_OP_XCLIP = 4,
       BG_OP_YCLIP = 5 };

/* bio_types::alignment::Alignment (fields as constructed at pairwise/mod.rs:911-921) */
typedef struct {
    int32_t score;
    uint32_t xstart, xend, ystart, yend, xlen, ylen;
    uint32_t n_ops;
    uint64_t ops_off;     /* offset of this alignment's first op in the ops buffer */
    uint32_t clip_len[4]; /* lengths of the Xclip/Yclip ops, in order of appearance */
    uint8_t n_clips;
    uint8_t mode;         /* BG_MODE_* */
    int8_t status;        /* BG_OK, BG_ERR_TRACEBACK, or BG_ERR_INVALID_ARG (longer than the stated bounds) for this pair */
    uint8_t _pad;
    uint32_t _reserved;   /* 0: the record is 64 bytes, every one of them defined */
} bg_alignment_t;

/* Aligner::{custom,global,semiglobal,local} for n_pairs independent pairs
 * (mod.rs:591,925,954,986).  `mode` selects the wrapper: GLOBAL/SEMIGLOBAL/LOCAL overwrite
 * the four clip penalties exactly as the reference does (and SEMIGLOBAL/LOCAL drop the clip
 * ops, mod.rs:974,1006); CUSTOM uses sc as given.  x/y are concatenated sequences with
 * n_pairs+1 offsets each.  Returns BG_ERR_POSITIVE_PENALTY when a penalty is > 0.
 * ops_buf may be NULL (scores/coordinates only). */
int bg_align_batch(bg_ctx* ctx, const bg_scoring_t* sc, int mode, uint64_t n_pairs,
                   const uint8_t* x, const uint64_t* x_off, const uint8_t* y,
                   const uint64_t* y_off, bg_alignment_t* out, uint8_t* ops_buf,
                   uint64_t ops_cap, uint64_t* ops_used);
/* Device-resident flavour.  d_ops must hold n_pairs * ops_stride bytes where
 * ops_stride >= max(xlen+ylen)+4 over the batch; alignment p's ops end at
 * d_ops + (p+1)*ops_stride and ops_off points at its first op.  sc->matrix (if any) is a
 * HOST pointer (it is compacted and uploaded by the call, which then synchronises `stream` once).
 * max_xlen/max_ylen are upper bounds on the sequence lengths in the batch: a pair that exceeds them is not
 * aligned and gets status BG_ERR_INVALID_ARG in its record (xlen/ylen filled in, no operations). */
/* d_x, d_y and d_ops may be at any address (a pair whose slot ends 4-byte aligned stores four operations at a time, any other
 * byte by byte). */
int bg_align_batch_dev(bg_ctx* ctx, const bg_scoring_t* sc, int mode, uint64_t n_pairs,
                       const uint8_t* d_x, const uint64_t* d_x_off, const uint8_t* d_y,
                       const uint64_t* d_y_off, uint32_t max_xlen, uint32_t max_ylen,
                       bg_alignment_t* d_out, uint8_t* d_ops, uint64_t ops_stride, void* stream);
/* The same on 2-bit streams (bg_pack2_dev above): d_x / d_y hold 16 symbols per dword, the offsets count symbols,
 * `codes` are the bytes the four codes stand for.  Short reads under MatchParams scoring (the packed-int16 kernel) read
 * the codes as they are and the call stays asynchronous like bg_align_batch_dev.  Every other case (long reads, wide
 * scores, a matrix) is a FALLBACK that is not: it reads the two stream lengths d_x_off[n_pairs] / d_y_off[n_pairs] back
 * (two blocking copies + one synchronisation of `stream`), may grow the ctx's unpack scratch (hipMalloc), unpacks both
 * streams there and runs the byte kernels — same results either way.  That scratch belongs to the ctx: calls on one ctx
 * are serialised by the ctx's scratch guard (an event), so use one ctx per stream for concurrent batches. */
int bg_align_batch_packed_dev(bg_ctx* ctx, const bg_scoring_t* sc, int mode, uint64_t n_pairs, const uint32_t* d_x,
                              const uint64_t* d_x_off, const uint32_t* d_y, const uint64_t* d_y_off,
                              const uint8_t* codes, uint32_t max_xlen, uint32_t max_ylen, bg_alignment_t* d_out,
                              uint8_t* d_ops, uint64_t ops_stride, void* stream);

/* banded::Aligner::{custom,global,semiglobal,local} (banded.rs:282,872,901,972) with k-mer
 * length k and window w.  The band (k-mer matching, sparse DP chaining, Band construction,
 * banded.rs:1278-1367) is built on the device by this call (band_device.hip; the few pairs its fixed-size
 * tables cannot hold — > 4095 matches, > 32 occurrences of one k-mer — are rebuilt by the host builder,
 * band_host.cpp, with identical results); pairs whose band exceeds MAX_CELLS
 * (banded.rs:104) get the reference's sentinel alignment {score: MIN_SCORE, all zero, no ops,
 * mode Custom} (banded.rs:407-420).  band_cells (optional) receives Band::num_cells. */
int bg_align_banded_batch(bg_ctx* ctx, const bg_scoring_t* sc, int mode, uint32_t k, uint32_t w,
                          uint64_t n_pairs, const uint8_t* x, const uint64_t* x_off,
                          const uint8_t* y, const uint64_t* y_off, bg_alignment_t* out,
                          uint8_t* ops_buf, uint64_t ops_cap, uint64_t* ops_used,
                          uint64_t* band_cells);

/* Same with device pointers for the sequences, offsets, records and operation slots (bg_align_batch_dev
 * conventions: record p keeps ops_off = (p + 1) * ops_stride - n_ops, its operations right-aligned in
 * slot p; ops_stride >= longest x + longest y + 4).  The call is synchronous (it drives the engine's own
 * streams); work queued on `stream` before it is waited for.  band_cells is a host array (optional). */
/* d_x, d_y and d_ops may be at any address (the band builder loads 16 bytes at a time from the first 16-byte boundary of a
 * sequence on, the bytes around byte by byte). */
int bg_align_banded_batch_dev(bg_ctx* ctx, const bg_scoring_t* sc, int mode, uint32_t k, uint32_t w,
                              uint64_t n_pairs, const uint8_t* d_x, const uint64_t* d_x_off,
                              const uint8_t* d_y, const uint64_t* d_y_off, bg_alignment_t* d_out,
                              uint8_t* d_ops, uint64_t ops_stride, uint64_t* band_cells, void* stream);

/* Band::create (banded.rs:1278-1367) for a batch, on host threads: k-mer matching, sparse DP
 * chaining (sparse.rs:188-295) and band rasterisation under the clip penalties `mode` implies.
 * Pair p's n_p+1 half-open row ranges [start, end) are written at band_off[p]; band_cells
 * (optional) receives Band::num_cells.  Pure host code. */
int bg_band_create_batch(const bg_scoring_t* sc, int mode, uint32_t k, uint32_t w, uint64_t n_pairs,
                         const uint8_t* x, const uint64_t* x_off, const uint8_t* y, const uint64_t* y_off,
                         const uint64_t* band_off, uint32_t* start, uint32_t* end, uint64_t* band_cells);

/* compute_alignment (banded.rs:406-869) over caller-supplied bands — the common tail of
 * custom_with_prehash / custom_with_matches / custom_with_expanded_matches / custom_with_match_path
 * / semiglobal_with_prehash (banded.rs:294-401, 938-970) once their band exists.  Pair p's band is
 * the n_p + 1 half-open row ranges band_start/band_end[band_off[p] ..]; `mode` applies the same
 * clip overrides as bg_align_banded_batch.  A band whose column ranges are not monotone gets
 * status BG_ERR_UNSUPPORTED for that pair. */
int bg_align_banded_bands_batch(bg_ctx* ctx, const bg_scoring_t* sc, int mode, uint64_t n_pairs,
                                const uint8_t* x, const uint64_t* x_off, const uint8_t* y,
                                const uint64_t* y_off, const uint64_t* band_off,
                                const uint32_t* band_start, const uint32_t* band_end,
                                bg_alignment_t* out, uint8_t* ops_buf, uint64_t ops_cap,
                                uint64_t* ops_used, uint64_t* band_cells);

/* Band::create_with_matches (banded.rs:1301-1328; path == NULL) or Band::create_from_match_path
 * (banded.rs:1330-1367) for a batch, on host threads.  Matches are (x, y) uint32 pairs, sorted;
 * pair p owns matches_xy[2*match_off[p] .. 2*match_off[p+1]) and, if given, path[path_off[p] ..
 * path_off[p+1]) (indices into its matches).  BG_ERR_INVALID_ARG where the reference asserts
 * (unsorted matches) or indexes out of bounds. */
int bg_band_from_matches_batch(const bg_scoring_t* sc, int mode, uint32_t k, uint32_t w,
                               uint64_t n_pairs, const uint64_t* x_off, const uint64_t* y_off,
                               const uint32_t* matches_xy, const uint64_t* match_off,
                               const uint32_t* path, const uint64_t* path_off,
                               const uint64_t* band_off, uint32_t* start, uint32_t* end,
                               uint64_t* band_cells);

/* sparse.rs on the host: find_kmer_matches (337-348), sdpkpp path (188-295), lcskpp path + score
 * (67-143), sdpkpp_union_lcskpp_path (297-329), expand_kmer_matches (404-500).  Each returns the
 * length of its result (call again with a larger buffer if it exceeds `cap`), or UINT64_MAX where
 * the reference asserts ("incoming matches must be sorted"). */
uint64_t bg_sparse_find_kmer_matches(const uint8_t* x, uint64_t m, const uint8_t* y, uint64_t n,
                                     uint32_t k, uint32_t* out_xy, uint64_t cap);
uint64_t bg_sparse_sdpkpp(const uint32_t* matches_xy, uint64_t n_matches, uint32_t k,
                          uint32_t match_score, int32_t gap_open, int32_t gap_extend,
                          uint32_t* path, uint64_t cap);
uint64_t bg_sparse_lcskpp(const uint32_t* matches_xy, uint64_t n_matches, uint32_t k, uint32_t* path,
                          uint64_t cap, uint32_t* score);
uint64_t bg_sparse_sdpkpp_union_lcskpp_path(const uint32_t* matches_xy, uint64_t n_matches, uint32_t k,
                                            uint32_t match_score, int32_t gap_open,
                                            int32_t gap_extend, uint32_t* path, uint64_t cap);
uint64_t bg_sparse_expand_kmer_matches(const uint8_t* x, uint64_t m, const uint8_t* y, uint64_t n,
                                       uint32_t k, const uint32_t* matches_xy, uint64_t n_matches,
                                       uint32_t allowed_mismatches, uint32_t* out_xy, uint64_t cap);

/* ---- seed-and-extend read mapping (BASELINE configs[4]) ----------------------------------------------------
 * rust-bio has no read mapper; its callers compose one from FMIndex::backward_search (fmindex.rs:144-208),
 * Interval::occ (fmindex.rs:75-79) and Aligner::semiglobal (pairwise/mod.rs:954) — the pattern of src/lib.rs:129-165
 * and benches/fmindex.rs:20-38.  bg_seed_extend_batch is that composition for a batch of reads with every
 * intermediate in HBM; its definition (stated on the CPU by oracle/pipeline.cpp out of the oracle's three calls):
 *   seeds        read[o .. o + seed_len) for o = 0, stride, 2 stride, ... while the window fits in the read;
 *   votes        a seed votes when its search is Complete and its interval holds 1 ..= max_occ rows;
 *   proposals    hit position p of the seed at offset o proposes the read start s = p - o; s < 0 or s >= n_text
 *                (the text without its final sentinel) is dropped, equal (read, s) proposals are merged; of the sorted starts
 *                of a read, one within pad / 2 of the last start kept is merged into it as well (the seeds either side of an
 *                indel propose the same locus a few bases apart, and the +- pad window of the first holds both alignments;
 *                pad / 2 = 0: only equal starts merge — the definition of rounds 3-5);
 *   extension    Aligner::semiglobal(x = read, y = text[max(0, s - pad) .. min(n_text, s + read_len + pad)));
 *   best hit     per read the highest score, the smallest s among equal scores; a read without candidates
 *                reports score BG_MIN_SCORE, ref positions UINT64_MAX and no operations.
 * A seed that reaches a byte outside the index's alphabet (where the reference's backward_search panics, fmindex.rs:229)
 * does not vote; the call then returns BG_ERR_OUT_OF_ALPHABET with every read still answered.
 * The index handle needs the text (bg_fm_set_text[_dev]: all n bytes the index was built from, final sentinel
 * included) and a suffix array (bg_fm_set_suffix_array / bg_fm_set_sampled_suffix_array). */
int bg_fm_set_text(bg_fm* fm, const uint8_t* text, uint64_t n);         /* host text, copied to the device */
/* (d_text of bg_fm_set_text_dev may be at any address) */
int bg_fm_set_text_dev(bg_fm* fm, const uint8_t* d_text, uint64_t n);   /* device text, borrowed: must outlive the handle's use */
typedef struct {
    uint32_t seed_len, stride; /* benches/fmindex.rs:21-25 searches 20-mers */
    uint32_t max_occ;          /* a seed with more occurrences does not vote */
    uint32_t pad;              /* text taken on both sides of the proposed placement */
} bg_seed_params_t;
typedef struct {
    bg_alignment_t aln;          /* Aligner::semiglobal(read, window) of the best candidate (y coordinates inside the window) */
    uint64_t window_start;       /* text offset of that window */
    uint64_t ref_start, ref_end; /* window_start + ystart / yend */
    uint32_t n_candidates;       /* distinct proposed starts of this read (all were aligned) */
    uint32_t n_seed_hits;        /* suffix-array rows its voting seeds resolved */
} bg_seed_hit_t;
/* reads: concatenated, n_reads + 1 offsets (reads up to 65535 bases; (seed slots) x max_occ <= 1024 per read).
 * ops_buf (optional) receives the winners' operations back to back in read order, hits[r].aln.ops_off points there. */
int bg_seed_extend_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, uint64_t n_reads,
                         const uint8_t* reads, const uint64_t* read_off, bg_seed_hit_t* hits, uint8_t* ops_buf,
                         uint64_t ops_cap, uint64_t* ops_used);
/* Device flavour: reads, offsets, hits and (optional) operation slots in HBM; read r's operations end at
 * d_ops + (r + 1) * ops_stride (ops_stride >= 2 * max_read_len + 2 * pad + 4), hits[r].aln.ops_off points at the
 * first.  totals (optional, host, 2 entries): suffix-array rows resolved, candidates aligned.  The call waits twice
 * per 2^20 reads for a few counters that size the next stage; everything else is asynchronous on `stream`.
 * It goes through the handle's ctx (scratch, aligner): the ctx's single-thread rule applies. */
int bg_seed_extend_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, uint64_t n_reads,
                             const uint8_t* d_reads, const uint64_t* d_read_off, uint32_t max_read_len,
                             bg_seed_hit_t* d_hits, uint8_t* d_ops, uint64_t ops_stride, uint64_t* totals,
                             void* stream);
/* Both strands.  Sequencers read both strands of the DNA: against an index of the forward text, a read from the other
 * strand maps as its reverse complement.  revcomp(read) is rust-bio's dna::revcomp (alphabets/dna.rs): the bytes
 * reversed, AGCTYRWSKMDVHBN -> TCGARYWSMKHBDVN and the same in lower case, every other byte (N, $, ...) itself.
 *   forward strand   the composition above on `read`;
 *   reverse strand   the composition above on revcomp(read) — seeds, votes, proposals, merge, windows and extension apply
 *                    to each strand on its own;
 *   best hit         with both strands the highest score wins, the forward strand on an equal score, the smallest s
 *                    within one strand.
 * A reverse-strand winner's aln (x coordinates, xlen, operations) refers to revcomp(read) against the forward text (the
 * SAM convention: bg_cigar_batch gives the SAM CIGAR directly); window_start / ref_start / ref_end are forward-text
 * coordinates.  n_candidates, n_seed_hits and totals are sums over the strands that ran.  strand[r] (optional): BG_HIT_*
 * of read r's winner.  `strands` outside BG_STRAND_FORWARD ..= BG_STRAND_BOTH: BG_ERR_INVALID_ARG; every other limit,
 * argument check and the out-of-alphabet rule are those of bg_seed_extend_batch[_dev], per strand.  strands =
 * BG_STRAND_FORWARD computes exactly what bg_seed_extend_batch[_dev] computes. */
enum { BG_STRAND_FORWARD = 1, BG_STRAND_REVERSE = 2, BG_STRAND_BOTH = 3 };   /* which strands to map */
enum { BG_HIT_FORWARD = 0, BG_HIT_REVERSE = 1, BG_HIT_NONE = 255 };          /* strand[r] of the winner */
int bg_seed_extend_strands_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, uint32_t strands,
                                 uint64_t n_reads, const uint8_t* reads, const uint64_t* read_off, bg_seed_hit_t* hits,
                                 uint8_t* strand, uint8_t* ops_buf, uint64_t ops_cap, uint64_t* ops_used);
/* Device flavour (operation slots, totals and passes as bg_seed_extend_batch_dev; seed_chunk_reads counts the caller's
 * reads, and with both strands a pass takes at most 2^20 of them). */
/* d_reads, d_strand and d_ops may be at any address. */
int bg_seed_extend_strands_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, uint32_t strands,
                                     uint64_t n_reads, const uint8_t* d_reads, const uint64_t* d_read_off,
                                     uint32_t max_read_len, bg_seed_hit_t* d_hits, uint8_t* d_strand, uint8_t* d_ops,
                                     uint64_t ops_stride, uint64_t* totals, void* stream);
/* Seeds from the SMEMs of an FMD index, both strands in one seeding pass.  The handle is an FMD index over T$R$ (T: the
 * forward text of n_t = (n - 2) / 2 symbols, which may itself hold '$' between sequences; R = revcomp(T); the check K7 makes,
 * else BG_ERR_UNSUPPORTED) with its text attached, all n bytes of T$R$ (n odd or n < 2: BG_ERR_INVALID_ARG), and a raw or
 * sampled suffix array.  Fixed seed windows miss a read that has an error in every window; its exact stretches between the
 * errors are SMEMs, and over T$R$ the rows of an SMEM's interval in the T half place the read, those in the R half its
 * revcomp.  The definition (stated on the CPU by tests/smem_seed_oracle.py):
 *   seeds        the records of FMDIndex::all_smems(read, min_seed_len) (fmindex.rs:479-501) on the caller's read, once per
 *                read (not again on its revcomp), in the reference's push order: a BiInterval {lower, lower_rev, size,
 *                match_size}, a position a on the read and a length len.  Only the first max_smems records are used; if a read
 *                has more, the call still answers every read from those and returns BG_ERR_OPS_CAP (bg_fmd_smems_batch's
 *                convention for its cap).  A read on which the reference would panic (K7's count 0xFFFFFFFF) does not vote:
 *                the call returns BG_ERR_OUT_OF_ALPHABET with every read answered; this error takes precedence over
 *                BG_ERR_OPS_CAP;
 *   votes        a record votes when 1 <= size <= max_occ;
 *   locate       Interval::occ of [lower, lower + size) (BiInterval::forward()), through K6 unchanged;
 *   proposals    text position p of a voting record, L the read's length:
 *                  forward half   p + len <= n_t: the read starts at s = p - a (dropped if p < a);
 *                  reverse half   p >= n_t + 1 and p + len <= 2 n_t + 1, q = p - n_t - 1: revcomp(read) starts on the forward
 *                                 text at s = n_t + a - q - L (dropped if q + L > n_t + a);
 *                anything else is dropped (a hit across a sentinel, which only a read that holds '$' can have, BG_SA_NONE,
 *                BG_SA_PANIC), and so are s >= n_t and a proposal of a strand that `strands` excludes;
 *   after that   the strands call word for word with n_text = n_t: per (read, strand) the starts are sorted, equal ones and
 *                those within pad / 2 of the last start kept are merged; windows [max(0, s - pad), min(n_t, s + L + pad));
 *                Aligner::semiglobal; best hit (highest score, forward on a tie between strands, smallest s within one).
 * n_seed_hits: the suffix-array rows of the read's voting records that fall in the half (as the two conditions above define
 * it) of a strand that ran; totals[0]: every row K6 resolved; totals[1]: candidates aligned.  Limits: max_smems * max_occ <=
 * 1024 (else BG_ERR_UNSUPPORTED), a zero min_seed_len / max_smems / max_occ is BG_ERR_INVALID_ARG, pad <= 65535, reads of up to
 * 65534 bases (K7's limit; longer: BG_ERR_TOO_LARGE); indexes with 32-bit and with 64-bit positions.  Arguments, slots, the
 * ops_stride rule, passes (seed_chunk_reads) and the two totals are those of bg_seed_extend_strands_batch[_dev]; the device
 * flavour waits once more per pass, for the check of the reads' lengths against max_read_len that K7's scratch depends on. */
typedef struct {
    uint32_t min_seed_len;  /* l of FMDIndex::all_smems(read, l), fmindex.rs:479-501; >= 1 */
    uint32_t max_smems;     /* records used per read, in the reference's push order; >= 1 */
    uint32_t max_occ;       /* an SMEM whose BiInterval.size exceeds this does not vote; >= 1 */
    uint32_t pad;           /* as bg_seed_params_t.pad */
} bg_smem_seed_params_t;
int bg_seed_extend_smem_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_smem_seed_params_t* prm, uint32_t strands,
                              uint64_t n_reads, const uint8_t* reads, const uint64_t* read_off, bg_seed_hit_t* hits,
                              uint8_t* strand, uint8_t* ops_buf, uint64_t ops_cap, uint64_t* ops_used);
int bg_seed_extend_smem_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_smem_seed_params_t* prm, uint32_t strands,
                                  uint64_t n_reads, const uint8_t* d_reads, const uint64_t* d_read_off, uint32_t max_read_len,
                                  bg_seed_hit_t* d_hits, uint8_t* d_strand, uint8_t* d_ops, uint64_t ops_stride,
                                  uint64_t* totals, void* stream);
/* Tiered seeds: one call on one FMD index, fixed windows for every read and SMEMs only for the reads the windows leave weak.
 * The handle is what bg_seed_extend_smem_batch takes: an FMD index over T$R$ (else BG_ERR_UNSUPPORTED; n odd or n < 2:
 * BG_ERR_INVALID_ARG) with all of T$R$ attached and a raw or sampled suffix array, on 32- or 64-bit positions.  The definition
 * (stated on the CPU by tests/tiered_seed_oracle.py):
 *   tier 1       the SMEM call above word for word, with its `seeds` line replaced:
 *     seeds        the records of a read of length L are its windows read[o .. o + seed_len) for o = 0, stride, 2 stride, ...
 *                  while the window fits in the read, each searched once with FMIndex::backward_search (fmindex.rs:144-208) on
 *                  the FMD index — on the caller's read only, never on its revcomp.  A Complete search gives the record {lower,
 *                  size = upper - lower, a = o, len = seed_len}; a Partial or Absent one a record of size 0.  A window that
 *                  reaches a byte outside the alphabet does not vote (the read's other windows do), and the call returns
 *                  BG_ERR_OUT_OF_ALPHABET with every read answered.  There is no truncation: a read's records are all its
 *                  windows;
 *     votes        a record votes when 1 <= size <= window.max_occ, size being the whole interval over T$R$, both halves together;
 *     after that   locate, the two half formulas and their dropped cases, `strands`, the merge within a strand with window.pad,
 *                  windows, Aligner::semiglobal, best hit, n_seed_hits and n_candidates are the SMEM call's, with n_text = n_t.
 *                This is NOT bg_seed_extend_strands_batch on a forward index of T$: a window whose rows lie in the R half proposes
 *                revcomp(read) from a window that is not on revcomp(read)'s own stride grid (its offset on revcomp(read) is L - o -
 *                seed_len), and max_occ counts the occurrences on both strands together.
 *   selection    read r is re-seeded when its tier-1 winner's score is below reseed_below.  A read without candidates has
 *                BG_MIN_SCORE, so reseed_below = BG_MIN_SCORE re-seeds no read and INT32_MAX every read.
 *   tier 2       bg_seed_extend_smem_batch with `smem` and the same `strands` on exactly the re-seeded reads.
 *   answer       a read that is not re-seeded reports tier 1 alone.  A re-seeded read reports the better of its two tier winners
 *                (a tier without a hit loses to one with a hit): the higher score, then the forward strand, then the smaller
 *                window_start, then tier 1.  Strand and operations are the winner's; n_candidates and n_seed_hits are the sums
 *                of both tiers.
 * tier[r] (optional): BG_TIER_NONE — not re-seeded; BG_TIER_FIRST — re-seeded, tier 1's hit (or no hit) kept; BG_TIER_SECOND —
 * tier 2's hit.  totals (optional, host, 3 entries): suffix-array rows resolved and candidates aligned, each over both tiers,
 * then reads re-seeded.  Status: BG_ERR_OUT_OF_ALPHABET from either tier comes before BG_ERR_OPS_CAP, which says that a
 * re-seeded read has more than smem.max_smems SMEMs (answered from the first max_smems, as in the SMEM call); every read is
 * answered under both.  Refused before any work, outputs untouched: window.pad != smem.pad (one ops_stride and one merge distance
 * serve both tiers), a zero seed_len / stride / window.max_occ / min_seed_len / max_smems / smem.max_occ (BG_ERR_INVALID_ARG);
 * more than 64 window slots at max_read_len ((max_read_len - seed_len) / stride + 1), slots * window.max_occ > 1024, max_smems *
 * smem.max_occ > 1024 (BG_ERR_UNSUPPORTED); max_read_len > 65534 (BG_ERR_TOO_LARGE).  Arguments, slots, the ops_stride rule and
 * passes (seed_chunk_reads) are those of bg_seed_extend_strands_batch[_dev]; the hits are ordinary bg_seed_hit_t slots
 * (bg_sam_emit_batch[_dev] takes them as they are).  The device flavour waits once more per pass for the number of re-seeded
 * reads and their bytes; a pass that re-seeds no read launches nothing of tier 2. */
typedef struct {
    bg_seed_params_t window;      /* tier 1: seed_len, stride, max_occ, pad */
    bg_smem_seed_params_t smem;   /* tier 2: min_seed_len, max_smems, max_occ, pad (== window.pad) */
    int32_t reseed_below;         /* a read whose tier-1 winner scores less is re-seeded */
} bg_tiered_seed_params_t;
enum { BG_TIER_NONE = 0, BG_TIER_FIRST = 1, BG_TIER_SECOND = 2 };   /* tier[r] */
int bg_seed_extend_tiered_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_tiered_seed_params_t* prm, uint32_t strands,
                                uint64_t n_reads, const uint8_t* reads, const uint64_t* read_off, bg_seed_hit_t* hits,
                                uint8_t* strand, uint8_t* tier, uint8_t* ops_buf, uint64_t ops_cap, uint64_t* ops_used);
/* Device flavour: d_reads, d_strand, d_tier and d_ops may be at any address (a re-seeded read's operations move into the
 * caller's slot 16 bytes at a time where the two addresses agree mod 16, else byte by byte). */
int bg_seed_extend_tiered_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_tiered_seed_params_t* prm, uint32_t strands,
                                    uint64_t n_reads, const uint8_t* d_reads, const uint64_t* d_read_off, uint32_t max_read_len,
                                    bg_seed_hit_t* d_hits, uint8_t* d_strand, uint8_t* d_tier, uint8_t* d_ops, uint64_t ops_stride,
                                    uint64_t* totals, void* stream);
/* Read pairs.  Paired-end reads come as two mates per DNA fragment, read towards each other from opposite strands.  The
 * reads are interleaved mates: read 2p is mate 1 of pair p, read 2p + 1 its mate 2 (2 n_pairs + 1 offsets; an interleaved
 * FASTQ parsed by bg_fastq_parse[_dev] gives this layout).
 *   candidates       each mate is mapped on both strands exactly as bg_seed_extend_strands_batch with BG_STRAND_BOTH maps a
 *                    read; a candidate's ref_start / ref_end are forward-text coordinates; the candidates of one (mate,
 *                    strand) are numbered in ascending proposed start;
 *   proper           a candidate a of one mate on the forward strand with a candidate b of the other mate on the reverse
 *                    strand — orientation A: m1 forward, m2 reverse; orientation B: m2 forward, m1 reverse — with
 *                    a.ref_start <= b.ref_start and min_span <= span <= max_span, span = max(a.ref_end, b.ref_end) -
 *                    a.ref_start (FR only: RF, FF and RR are never proper);
 *   best proper      the highest a.score + b.score (64-bit); on a tie orientation A, then the smaller candidate index of the
 *                    forward mate, then that of the reverse mate;
 *   paired or not    best1, best2: each mate's own best under the strands rule.  If a proper combination exists and
 *                    pair_sum + pen_unpaired >= best1 + best2, the pair is proper: hits[2p], hits[2p + 1] are that
 *                    combination's two candidates (operations and strands with them).  Otherwise each mate reports exactly
 *                    what bg_seed_extend_strands_batch reports for it (BG_HIT_NONE included) and the pair is not proper.
 * n_candidates, n_seed_hits and totals mean what they mean in the strands call, per mate.  strand[r] (optional): BG_HIT_*
 * of each reported hit.  Operation slots, ops_stride, host compaction, the out-of-alphabet rule and every limit are those of
 * the strands call.  BG_ERR_INVALID_ARG: min_span > max_span, pen_unpaired < 0, a null pairs, a null hits with n_pairs > 0.
 * A pass never splits a pair: seed_chunk_reads counts the caller's reads, rounded down to an even count (at least 2). */
typedef struct {
    uint32_t min_span, max_span; /* a proper pair's span (SAM |TLEN|), both inclusive */
    int32_t  pen_unpaired;       /* >= 0; the score a proper pair may give up against the two mates' own bests */
} bg_pair_params_t;
typedef struct {
    uint64_t span;      /* of the reported proper pair; 0 when not proper */
    uint32_t n_proper;  /* proper combinations among the pair's candidates, both orientations */
    uint8_t  proper;    /* 1: hits[2p], hits[2p + 1] are the chosen proper pair */
    uint8_t  reserved[3];
} bg_pair_hit_t;        /* 16 bytes */
int bg_seed_extend_pairs_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                               uint64_t n_pairs, const uint8_t* reads, const uint64_t* read_off, bg_seed_hit_t* hits,
                               uint8_t* strand, bg_pair_hit_t* pairs, uint8_t* ops_buf, uint64_t ops_cap, uint64_t* ops_used);
/* Device flavour (operation slots of the 2 n_pairs reads, totals and passes as bg_seed_extend_strands_batch_dev). */
int bg_seed_extend_pairs_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                                   uint64_t n_pairs, const uint8_t* d_reads, const uint64_t* d_read_off, uint32_t max_read_len,
                                   bg_seed_hit_t* d_hits, uint8_t* d_strand, bg_pair_hit_t* d_pairs, uint8_t* d_ops,
                                   uint64_t ops_stride, uint64_t* totals, void* stream);
/* Mate rescue.  The paired call makes a pair proper only if BOTH mates produced a seeded candidate at the right locus.  A mate
 * whose every seed window holds a mismatch, or whose seeds all fall in intervals above max_occ (a mate inside a repeat), has no
 * candidate there.  Its partner already says where it must lie: within max_span, on the opposite strand.  The rescue call is
 * the paired call plus one more batch of semiglobal alignments in those insert windows.  Per pair p (m1 = read 2p, m2 = read
 * 2p + 1):
 *   candidates, pair rule   exactly those of bg_seed_extend_pairs_batch.  If the pair rule finds a proper combination
 *                    (n_proper > 0, whatever "paired or not" then decides), or neither mate has a candidate, the pair's outputs
 *                    are exactly the paired call's and rescued[p] = 0;
 *   anchors          otherwise, for each mate that has candidates: its candidates over both strands in the multi call's rank order
 *                    (score descending, then candidate number: forward strand first, ascending proposed start); the first A =
 *                    max_anchors of them are its anchors, of anchor rank 0 .. A - 1.  An anchor with ref_end - ref_start >
 *                    max_span is skipped (it keeps its rank and gives no rescue alignment);
 *   rescue window    of anchor c (text = the indexed text without its final sentinel, n_text bytes):
 *                    forward anchor: [c.ref_start, min(n_text, c.ref_start + max_span)), the other mate is sought on the reverse
 *                    strand; reverse anchor: [c.ref_end - max_span (0 if that is negative), c.ref_end), the other mate is sought
 *                    on the forward strand;
 *   rescue alignment Aligner::semiglobal(x, y = text[window)), x = the other mate as read (forward strand sought) or revcomp of
 *                    it (reverse strand sought).  An empty window or an x of length 0 gives no alignment.  Its hit is a complete
 *                    bg_seed_hit_t: aln the aligner's record (operations with it), window_start the window's first text offset,
 *                    ref_start / ref_end = window_start + ystart / yend, n_candidates / n_seed_hits the mate's own seeded counts
 *                    (possibly 0);
 *   accepted         if its score >= min_score and (anchor, rescued) passes the pair rule's own "proper" test (the forward one is
 *                    a, the reverse one b: a.ref_start <= b.ref_start, min_span <= span <= max_span);
 *   choice           among a pair's accepted rescues the highest anchor.score + rescued.score (64-bit); on a tie orientation A (m1
 *                    forward), then the rescue anchored on m1, then the smaller anchor rank;
 *   paired or not    own(m) = mate m's own best score under the strands rule, 0 for a mate without candidates.  If sum +
 *                    pen_unpaired >= own(m1) + own(m2): the anchor's mate reports the anchor candidate exactly as the paired call
 *                    writes a candidate, the other mate reports the rescued hit with its strand, pairs[p].proper = 1,
 *                    pairs[p].span the span, pairs[p].n_proper stays the seeded count (0), rescued[p] = 1 or 2: which mate was
 *                    rescued.  Otherwise the paired call's output and rescued[p] = 0.
 * A rescued hit is an ordinary hit to every consumer (bg_sam_emit_batch[_dev] writes it as it writes a seeded one).
 * Limits and errors of the rescue calls (everything else is the paired call's): max_span > 65535: BG_ERR_TOO_LARGE; max_anchors 0
 * or above BG_RESCUE_MAX_ANCHORS, a null rp or rescued: BG_ERR_INVALID_ARG; device operation slots need ops_stride >=
 * max_read_len + max(max_read_len + 2 pad, max_span) + 4, else BG_ERR_OPS_CAP.  totals (optional, host) has 4 entries:
 * suffix-array rows resolved, seeded candidates aligned, rescue alignments run, pairs rescued.  A pass waits once more than
 * a pass of the paired call, for the counters that size the rescue batch; a call given totals waits once more at its end, for
 * the fourth.  Passes never split a pair and the result does not depend on seed_chunk_reads.  The out-of-alphabet rule is
 * unchanged (the rescue alignment itself needs no alphabet).
 * max_span also sizes the window: with max_span one below a fragment's length the mate is still found, aligned without its last
 * base, and the accepted span is then at most max_span.
 * Known limits: a forward mate that ends beyond its reverse partner's end is outside the window (dovetailed mates); a better
 * rescued pair is not sought when a proper seeded combination exists; a rescue window may cross a contig boundary.  (A MAPQ for
 * the mates of a rescued pair: bg_seed_extend_pairs_rescue_mapq_batch[_dev] below.) */
enum { BG_RESCUE_MAX_ANCHORS = 4 };
typedef struct {
    uint32_t max_anchors;  /* A: anchors tried per mate, 1 ..= BG_RESCUE_MAX_ANCHORS */
    int32_t  min_score;    /* a rescued alignment scoring below this is discarded */
} bg_rescue_params_t;
int bg_seed_extend_pairs_rescue_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                                      const bg_rescue_params_t* rp, uint64_t n_pairs, const uint8_t* reads, const uint64_t* read_off,
                                      bg_seed_hit_t* hits, uint8_t* strand, bg_pair_hit_t* pairs, uint8_t* rescued, uint8_t* ops_buf,
                                      uint64_t ops_cap, uint64_t* ops_used);
/* Device flavour (operation slots of the 2 n_pairs reads and passes as bg_seed_extend_pairs_batch_dev). */
int bg_seed_extend_pairs_rescue_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                                          const bg_rescue_params_t* rp, uint64_t n_pairs, const uint8_t* d_reads,
                                          const uint64_t* d_read_off, uint32_t max_read_len, bg_seed_hit_t* d_hits, uint8_t* d_strand,
                                          bg_pair_hit_t* d_pairs, uint8_t* d_rescued, uint8_t* d_ops, uint64_t ops_stride,
                                          uint64_t* totals, void* stream);
/* Runner-up loci and a mapping quality.  The strands call reports one alignment per read, so a read inside a two-copy repeat and
 * a read that maps uniquely look the same.  The multi call reports up to K = max_hits loci per read and a MAPQ: hits / strand
 * have K slots per read (hits[K r + k]), multi one record per read.
 *   candidates       those of bg_seed_extend_strands_batch with the same `strands`, numbered with the forward strand first and
 *                    in ascending proposed start within a strand; ref_start / ref_end are forward-text coordinates;
 *   rank             by score, the highest first; among equal scores the smaller candidate number (the strands call's best
 *                    hit is rank 0);
 *   loci             walk the candidates in rank order.  A candidate is kept as the next locus unless its text interval
 *                    touches or overlaps that of a locus already kept: a.ref_start <= b.ref_end && b.ref_start <= a.ref_end,
 *                    whatever the two strands (candidates that were not kept suppress nothing).  A candidate that scores below
 *                    min_score is never kept.  The walk stops after max(K, 2) loci;
 *   reported         loci 0 .. min(n_loci, K) - 1 fill the read's slots in that order, each a complete bg_seed_hit_t with its
 *                    strand and operations exactly as the strands call would write that candidate.  An unused slot is written
 *                    like an unmapped read (score BG_MIN_SCORE, positions UINT64_MAX, n_ops 0, strand BG_HIT_NONE).
 *                    n_candidates / n_seed_hits are the read's, repeated in every slot;
 *   MAPQ             in integers: s1 = the score of locus 0, s2 = the score of locus 1, or 0 if there is none.  mapq = 0 if there
 *                    is no locus, s1 <= 0 or s2 >= s1; otherwise min(mapq_cap, mapq_cap * (s1 - max(s2, 0)) / s1), 64-bit, the
 *                    division truncating.  The runner-up is found even when K = 1.
 * With min_score = INT32_MIN, slot 0 of every read is what bg_seed_extend_strands_batch[_dev] reports for it with the same
 * `strands`, field by field and operation by operation.  Device operation slots: slot K r + k ends at d_ops + (K r + k + 1) *
 * ops_stride (the same minimum stride); the host flavour compacts operations in slot order.  BG_ERR_INVALID_ARG: max_hits 0 or
 * above BG_SEED_MAX_HITS, mapq_cap above 254, a null mp or multi; every other check, limit, the out-of-alphabet rule, totals,
 * passes and seed_chunk_reads are the strands call's.
 * Known limit: inside a tandem repeat whose period is shorter than the read, the shifted copies overlap and count as one
 * locus, so MAPQ there is optimistic. */
enum { BG_SEED_MAX_HITS = 8 };
typedef struct {
    uint32_t max_hits;   /* K: hits reported per read, 1 ..= BG_SEED_MAX_HITS */
    int32_t  min_score;  /* a candidate scoring below this is neither reported nor counted as a runner-up */
    uint32_t mapq_cap;   /* MAPQ of a read without a runner-up; 0 ..= 254 (255 means "unavailable" in SAM) */
} bg_multi_params_t;
typedef struct {
    int32_t  sub_score;  /* score of the runner-up locus (locus 1), BG_MIN_SCORE if there is none */
    uint32_t n_loci;     /* loci found by the rule above, counted up to max(K, 2) */
    uint8_t  n_reported; /* min(n_loci, K): how many of the read's K slots are filled */
    uint8_t  mapq;
    uint8_t  reserved[6];
} bg_multi_hit_t;        /* 16 bytes */
int bg_seed_extend_multi_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_multi_params_t* mp,
                               uint32_t strands, uint64_t n_reads, const uint8_t* reads, const uint64_t* read_off,
                               bg_seed_hit_t* hits, uint8_t* strand, bg_multi_hit_t* multi, uint8_t* ops_buf, uint64_t ops_cap,
                               uint64_t* ops_used);
/* Device flavour (totals and passes as bg_seed_extend_strands_batch_dev). */
int bg_seed_extend_multi_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_multi_params_t* mp,
                                   uint32_t strands, uint64_t n_reads, const uint8_t* d_reads, const uint64_t* d_read_off,
                                   uint32_t max_read_len, bg_seed_hit_t* d_hits, uint8_t* d_strand, bg_multi_hit_t* d_multi,
                                   uint8_t* d_ops, uint64_t ops_stride, uint64_t* totals, void* stream);
/* Mapping quality of read pairs.  The paired call reports one placement per mate and does not say how unique it is; the multi
 * call scores single reads and knows nothing of the partner.  The pairs-mapq call is the paired call plus one bg_multi_hit_t
 * per read: multi[2p], multi[2p + 1] belong to the mates of pair p.  A mate inside a repeat whose partner is unique gets a high
 * MAPQ when the partner settles which copy it is, and 0 when it does not.  Like the pair and multi rules this is this library's
 * own definition (rust-bio has no mapper).
 *   outputs          candidates, the pair rule, "paired or not", hits, strand, pairs, operation slots, totals, passes and limits
 *                    are exactly those of bg_seed_extend_pairs_batch[_dev]: those outputs are written byte for byte as the
 *                    paired call writes them;
 *   touches(a, b)    the multi rule's test in forward-text coordinates, whatever the strands: a.ref_start <= b.ref_end &&
 *                    b.ref_start <= a.ref_end;
 *   not proper       (pairs[p].proper == 0) each mate's record is exactly what bg_seed_extend_multi_batch with BG_STRAND_BOTH,
 *                    max_hits = 1 and the same min_score / mapq_cap writes for that read: sub_score, n_loci (counted up to 2),
 *                    n_reported and mapq.  hits stay the paired call's even where the mate's best scores below min_score; the
 *                    record then says n_reported = 0, mapq = 0;
 *   proper           with the chosen combination (c1, c2), S1 = c1.score + c2.score (64-bit).  For mate i with partner j:
 *                    alternatives of mate i: every candidate x of mate i, on either strand, with x.score >= min_score and
 *                    !touches(x, c_i).  sub_score = the highest x.score among them, or BG_MIN_SCORE if there are none; n_loci =
 *                    2 or 1 accordingly; n_reported = 1.
 *                    S2_i = the maximum over (a) every proper combination (the pair rule's test, both orientations) whose
 *                    mate-i member is an alternative of mate i: the sum of its two scores; (b) every alternative x: x.score +
 *                    c_j.score - pen_unpaired, the mate placed elsewhere and unpaired.
 *                    mapq = 0 if c_i.score <= 0; mapq_cap if mate i has no alternative; otherwise min(mapq_cap, mapq_cap *
 *                    min(S1 - S2_i, c_i.score) / c_i.score), 64-bit, the division truncating.
 * S1 >= S2_i always holds: S1 is the maximum over all proper combinations, which covers (a); and "paired or not" made the pair
 * proper because S1 + pen_unpaired >= best1 + best2 >= x.score + c_j.score, which covers (b).  When the partner is the same in
 * both sums (S2_i = x.score + c_j.score through a proper combination) the formula is the multi rule's on mate i's scores, so a
 * pair and a single read agree where they should.
 * BG_ERR_INVALID_ARG: a null qp or multi, mapq_cap above 254; everything else is the paired call's.
 * Known limit: inside a tandem repeat whose period is shorter than the read the shifted copies touch and are no alternatives (the
 * multi rule's limit).  (This call never rescues; bg_seed_extend_pairs_rescue_mapq_batch[_dev] below rescues and judges.) */
typedef struct {
    int32_t  min_score;  /* a candidate scoring below this is no alternative and no runner-up */
    uint32_t mapq_cap;   /* MAPQ of a mate without an alternative; 0 ..= 254 */
} bg_pairq_params_t;
int bg_seed_extend_pairs_mapq_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                                    const bg_pairq_params_t* qp, uint64_t n_pairs, const uint8_t* reads, const uint64_t* read_off,
                                    bg_seed_hit_t* hits, uint8_t* strand, bg_pair_hit_t* pairs, bg_multi_hit_t* multi,
                                    uint8_t* ops_buf, uint64_t ops_cap, uint64_t* ops_used);
/* Device flavour (operation slots, totals and passes as bg_seed_extend_pairs_batch_dev; d_multi: 2 n_pairs records). */
int bg_seed_extend_pairs_mapq_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                                        const bg_pairq_params_t* qp, uint64_t n_pairs, const uint8_t* d_reads,
                                        const uint64_t* d_read_off, uint32_t max_read_len, bg_seed_hit_t* d_hits, uint8_t* d_strand,
                                        bg_pair_hit_t* d_pairs, bg_multi_hit_t* d_multi, uint8_t* d_ops, uint64_t ops_stride,
                                        uint64_t* totals, void* stream);
/* Mapping quality of rescued read pairs.  The rescue call places a mate inside its partner's insert window and says nothing of
 * how unique either placement is; the pairs-mapq call judges every mate and never rescues.  The rescue-mapq call is the rescue
 * call plus one bg_multi_hit_t per read (multi[2p], multi[2p + 1]: the mates of pair p).  rp is the rescue call's, qp the
 * pairs-mapq call's.  This is this library's own definition (rust-bio has no mapper).
 *   outputs          hits, strand, pairs, rescued, operation slots and totals (4 entries) are byte for byte what
 *                    bg_seed_extend_pairs_rescue_batch[_dev] writes for the same arguments;
 *   rescued[p] == 0  multi[2p] and multi[2p + 1] are exactly what bg_seed_extend_pairs_mapq_batch[_dev] writes for that pair: the
 *                    pairs-mapq rule with a proper seeded combination, the multi rule at K = 1 otherwise, also where rescue
 *                    alignments were run and none was accepted or "paired or not" turned the choice down;
 *   rescued[p] != 0  the chosen rescue is (anchor candidate c_a of mate a, rescued hit h of mate r); c_i is mate i's reported hit
 *                    (c_a or h); S1 = c_a.score + h.score (64-bit); touches is the multi rule's test.  An accepted rescue is any
 *                    planned rescue alignment of the pair that passes the rescue rule's acceptance, chosen or not; its two
 *                    members are its anchor (a seeded candidate of the anchoring mate) and its hit (a placement of the other
 *                    mate).  For mate i with partner j:
 *                    alternatives of mate i: every seeded candidate x of mate i, on either strand, with x.score >= qp.min_score
 *                    and !touches(x, c_i); and the mate-i member y of every accepted rescue with y.score >= qp.min_score and
 *                    !touches(y, c_i).  sub_score = the highest score among the alternatives, or BG_MIN_SCORE if there are none;
 *                    n_loci = 2 or 1 accordingly; n_reported = 1.
 *                    S2_i = the maximum over (a) every accepted rescue whose mate-i member is an alternative: its anchor's score
 *                    plus its hit's score; (b) every seeded alternative x: x.score + c_j.score - pen_unpaired.
 *                    mapq = 0 if c_i.score <= 0; mapq_cap if mate i has no alternative; otherwise min(mapq_cap, mapq_cap *
 *                    clamp(S1 - S2_i, 0, c_i.score) / c_i.score), in 64-bit signed integers, the division truncating.
 * Unlike the seeded rule, S1 >= S2_i does not always hold here: the chosen anchor is one of its mate's first A candidates by rank
 * and need not be that mate's best (the best one's own rescue may have failed), and the rescued hit may score above own(j); a
 * better-scoring seeded candidate of the anchor's mate then gives S2_i > S1 through (b).  Hence the clamp at 0: such a mate gets
 * mapq 0.
 * What the rule gives: an anchor inside a far two-copy repeat costs the anchor's mate pen_unpaired (mapq = mapq_cap *
 * pen_unpaired / score) and the rescued mate gets mapq_cap; two anchors that rescue the same placement give the anchor's mate 0
 * and the rescued mate mapq_cap (the two hits touch); a fragment wholly inside a two-copy repeat gives both mates 0; a rescued
 * mate with an exact seeded copy elsewhere is judged through (b).
 * Argument checks, limits, the ops_stride minimum, totals, passes and the extra waits are the rescue call's; in addition a null
 * qp or multi, or mapq_cap above 254: BG_ERR_INVALID_ARG.  An error writes nothing.
 * Known limits: those of the rescue rule (dovetailed mates, no rescue where a proper seeded combination exists, windows that
 * cross a contig boundary) and the multi rule's tandem-repeat limit. */
int bg_seed_extend_pairs_rescue_mapq_batch(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                                           const bg_rescue_params_t* rp, const bg_pairq_params_t* qp, uint64_t n_pairs,
                                           const uint8_t* reads, const uint64_t* read_off, bg_seed_hit_t* hits, uint8_t* strand,
                                           bg_pair_hit_t* pairs, uint8_t* rescued, bg_multi_hit_t* multi, uint8_t* ops_buf,
                                           uint64_t ops_cap, uint64_t* ops_used);
/* Device flavour (operation slots, totals and passes as bg_seed_extend_pairs_rescue_batch_dev; d_multi: 2 n_pairs records). */
int bg_seed_extend_pairs_rescue_mapq_batch_dev(bg_fm* fm, const bg_scoring_t* sc, const bg_seed_params_t* prm, const bg_pair_params_t* pp,
                                               const bg_rescue_params_t* rp, const bg_pairq_params_t* qp, uint64_t n_pairs,
                                               const uint8_t* d_reads, const uint64_t* d_read_off, uint32_t max_read_len,
                                               bg_seed_hit_t* d_hits, uint8_t* d_strand, bg_pair_hit_t* d_pairs, uint8_t* d_rescued,
                                               bg_multi_hit_t* d_multi, uint8_t* d_ops, uint64_t ops_stride, uint64_t* totals,
                                               void* stream);
/* d_out[d_off[i] .. d_off[i + 1]) = revcomp(d_in[d_off[i] .. d_off[i + 1])) for i < n (the FMD / SMEM callers need the
 * same operation); asynchronous on `stream`.  d_in and d_out must not overlap. */
/* (d_in and d_out may be at any address: read and written byte by byte) */
int bg_revcomp_batch_dev(bg_ctx* ctx, uint64_t n, const uint8_t* d_in, const uint64_t* d_off, uint8_t* d_out, void* stream);

/* ---- FASTQ ingest and CIGAR emission --------------------------------------
 * bio::io::fastq::Reader::read / Records on a text that is in memory (io/fastq.rs:266-303, 508-527: header
 * line '@id desc', sequence lines up to a line that starts with '+', then as many quality lines as there were
 * sequence lines; every line trimmed with str::trim_end) and Record::check (fastq.rs:388-410).  Records are
 * read until the end of the text or the first ReadError: *status is that error (BG_FASTQ_*), *err_pos the byte
 * offset of the line that raised it (the header line for IncompleteRecord), *n_records the records before it.
 * seq/qual are the concatenated trimmed lines; seq_off/qual_off have n_records+1 entries (seq_off is directly
 * the x_off of bg_align_batch_dev); capacity of seq/qual: `len` bytes, of the offsets: rec_cap+1.
 * Returns BG_ERR_TOO_LARGE if there are more than rec_cap records (n_records says how many). */
enum { BG_FASTQ_OK = 0, BG_FASTQ_MISSING_AT = 1, BG_FASTQ_INCOMPLETE = 2, BG_FASTQ_IO = 3 };   /* ReadError, fastq.rs:113-126 */
enum { BG_FQCHECK_OK = 0, BG_FQCHECK_EMPTY_ID = 1, BG_FQCHECK_NONASCII_SEQ = 2, BG_FQCHECK_INVALID_SEQ = 3,
       BG_FQCHECK_NONASCII_QUAL = 4, BG_FQCHECK_UNEQUAL = 5 };                                   /* CheckError, fastq.rs:129-150 */
typedef struct {
    uint64_t id_off, desc_off;   /* into the text */
    uint64_t seq_off, qual_off;  /* into seq / qual */
    uint32_t id_len, desc_len, seq_len, qual_len;
    int32_t has_desc;            /* 0: Record::desc() is None */
    int32_t check;               /* Record::check(): BG_FQCHECK_* (first failing rule) */
} bg_fastq_record_t;
int bg_fastq_parse(bg_ctx* ctx, const uint8_t* text, uint64_t len, bg_fastq_record_t* recs, uint64_t rec_cap,
                   uint8_t* seq, uint64_t* seq_off, uint8_t* qual, uint64_t* qual_off, uint64_t* n_records,
                   int32_t* status, uint64_t* err_pos);
/* the same with text, records, sequences, qualities and offsets in device memory (n_records/status/err_pos are
 * host pointers; the call synchronises `stream`) */
/* d_text, d_seq and d_qual may be at any address: a text at a 16-byte aligned address is loaded with vector loads, any other
 * address byte by byte; the outputs are written 16 bytes at a time between their own 16-byte boundaries. */
int bg_fastq_parse_dev(bg_ctx* ctx, const uint8_t* d_text, uint64_t len, bg_fastq_record_t* d_recs,
                       uint64_t rec_cap, uint8_t* d_seq, uint64_t* d_seq_off, uint8_t* d_qual,
                       uint64_t* d_qual_off, uint64_t* n_records, int32_t* status, uint64_t* err_pos,
                       void* stream);
/* bio_types::alignment::Alignment::cigar(hard_clip) (bio-types 1.0, a dependency that is not in the reference
 * tree: restated from its documentation, parity unpinned) for n alignments as returned by bg_align_batch
 * (ops_off into `ops`): xstart as a leading soft/hard clip, runs of '=' 'X' 'D' 'I', xlen - xend as the
 * trailing clip, "" without operations.  out_off has n+1 entries.  BG_ERR_UNSUPPORTED if some alignment has
 * AlignmentMode::Custom (the crate panics; its string is empty), BG_ERR_OPS_CAP if out_cap is too small. */
int bg_cigar_batch(bg_ctx* ctx, uint64_t n, const bg_alignment_t* aln, const uint8_t* ops, uint64_t ops_bytes,
                   int hard_clip, char* out, uint64_t out_cap, uint64_t* out_off);
/* device flavour: one slot of `stride` chars (>= 2 * max n_ops + 24) per alignment, d_len[p] = chars written
 * or a negative bg_status */
/* (d_ops and d_out may be at any address: read and written byte by byte) */
int bg_cigar_batch_dev(bg_ctx* ctx, uint64_t n, const bg_alignment_t* d_aln, const uint8_t* d_ops, int hard_clip,
                       char* d_out, uint64_t stride, int32_t* d_len, void* stream);

/* bio_types::alignment::Alignment::pretty(x, y, ncol) (bio-types, not in the reference tree: restated from the crate's
 * source as documented — parity unpinned; rust-bio's tests only print it, e.g. pairwise/banded.rs:1805) for n
 * alignments and the sequences they were computed from: rows x / marks / y ('|' match, '\\' mismatch, '+' insertion,
 * 'x' deletion, ' ' clipped, '-' gap), cut into blocks of ncol columns, each block "x\nmarks\ny\n\n\n".
 * out_off has n + 1 entries.  BG_ERR_UNSUPPORTED where the crate panics (a non-ASCII byte breaks its row-length
 * assert) or the sequences do not have the alignment's xlen / ylen; BG_ERR_OPS_CAP if out_cap is too small. */
int bg_pretty_batch(bg_ctx* ctx, uint64_t n, const bg_alignment_t* aln, const uint8_t* ops, uint64_t ops_bytes,
                    const uint8_t* x, const uint64_t* x_off, const uint8_t* y, const uint64_t* y_off, uint32_t ncol,
                    char* out, uint64_t out_cap, uint64_t* out_off);

/* ---- FASTA ingest and the reference text (fasta_ingest.hip) ----------------------------------------------
 * bio::io::fasta::Reader::read / Records on a text that is in memory (io/fasta.rs:334-359, 1090-1111) and Record::check
 * (fasta.rs:982-1009); conventions as for bg_fastq_parse[_dev] above.
 * Lines.  A line is the bytes up to and including '\n', or to the end of the text.  A line that is not valid UTF-8 makes
 * read_line fail (the validity rule of the FASTQ reader).  str::trim_end strips trailing Unicode White_Space: the line's
 * own '\n', '\r', and the multi-byte members U+0085, U+00A0, U+1680, U+2000-200A, U+2028, U+2029, U+202F, U+205F, U+3000.
 * First line and headers.  The first line must start with '>': otherwise *status = BG_FASTA_MISSING_GT with no records and
 * *err_pos = 0 (a leading blank line is that error).  An empty text is BG_FASTA_OK with 0 records.  After the first header
 * every line whose first byte is '>' is a header; every other line is a sequence line, whose trimmed bytes are appended to
 * the record's sequence (interior white space stays; check rejects it).
 * Header fields.  line[1..].trim_end() is split once at its first char::is_whitespace: the id is the part in front of that
 * character (it may be empty), the description everything behind that one character (it may begin with more white space);
 * without white space has_desc = 0.
 * Errors.  A read_line failure anywhere inside `read` of record k loses record k — also a failure on the header line of
 * record k + 1, which record k's loop reads: *status = BG_FASTA_IO, *err_pos = that line's offset, *n_records = k.
 * Early end.  Records ends at the first record that is_empty() (empty id, no description, empty sequence):
 * ">\n\n>x\nAC\n" yields 0 records with BG_FASTA_OK.
 * check: first failing rule of BG_FACHECK_EMPTY_ID, _NONASCII_SEQ, _INVALID_SEQ (a byte is valid if it is an ASCII letter
 * or one of - . *).
 * seq holds `len` bytes, seq_off rec_cap + 1 entries; BG_ERR_TOO_LARGE if there are more than rec_cap records (*n_records
 * says how many).  The device kernels work on tiles of BG_FASTA_TILE bytes of the text; a text at a 16-byte aligned address
 * is loaded with vector loads, any other address byte by byte (coalesced, but slower).  bg_fasta_parse, like bg_fastq_parse,
 * copies the text to the device and runs the same kernels: it needs a ctx and a GPU (bg_fasta_reference below does not).
 * recs, seq and seq_off must not be NULL for a text that is not empty, also with rec_cap == 0 (a call that only counts). */
#define BG_FASTA_TILE 8192
enum { BG_FASTA_OK = 0, BG_FASTA_MISSING_GT = 1, BG_FASTA_IO = 2 };
enum { BG_FACHECK_OK = 0, BG_FACHECK_EMPTY_ID = 1, BG_FACHECK_NONASCII_SEQ = 2, BG_FACHECK_INVALID_SEQ = 3 };  /* CheckError */
typedef struct {
    uint64_t id_off, desc_off;   /* into the text */
    uint64_t seq_off, seq_len;   /* into seq; 64-bit: a chromosome may exceed 2^32 */
    uint32_t id_len, desc_len;
    int32_t has_desc;            /* 0: Record::desc() is None */
    int32_t check;               /* Record::check(): BG_FACHECK_* (first failing rule) */
} bg_fasta_record_t;             /* 48 bytes */
int bg_fasta_parse(bg_ctx* ctx, const uint8_t* text, uint64_t len, bg_fasta_record_t* recs, uint64_t rec_cap,
                   uint8_t* seq, uint64_t* seq_off, uint64_t* n_records, int32_t* status, uint64_t* err_pos);
/* the same with text, records, sequences and offsets in device memory (n_records/status/err_pos are host pointers; the
 * call synchronises `stream`) */
int bg_fasta_parse_dev(bg_ctx* ctx, const uint8_t* d_text, uint64_t len, bg_fasta_record_t* d_recs, uint64_t rec_cap,
                       uint8_t* d_seq, uint64_t* d_seq_off, uint64_t* n_records, int32_t* status, uint64_t* err_pos,
                       void* stream);

/* ---- SAM records from seed-and-extend hits (sam_emit.hip) -----------------------------------------------
 * The output half of "wire format in, format out": one SAM line (SAM v1.6, section 1.4) per hit slot, formatted in HBM
 * from exactly what bg_fastq_parse_dev and bg_seed_extend_strands / _pairs / _pairs_mapq / _multi_batch_dev leave there; nothing is
 * repacked in between.  rust-bio has no SAM writer: the record is defined here from the SAM specification, the way the
 * pair and multi rules are defined above.  fm supplies the ctx and the attached text (bg_fm_set_text[_dev]), which MD needs.
 * Read r is FASTQ record r (recs[r]; its sequence and qualities at seq + seq_off, qual + qual_off, its id in the FASTQ
 * text), slot K r + k is hits / strand [K r + k] with K = max_hits (1 after the strands and pairs calls), operations at
 * ops + aln.ops_off.  multi (optional): one record per read; pairs (with BG_SAM_PAIRED): one per pair, reads 2p, 2p + 1.
 *
 * Output is one contiguous buffer: slot K r + k occupies out[out_off[K r + k] .. out_off[K r + k + 1]); a slot that writes
 * no line has length 0; the lines are in slot order, so the buffer is a valid SAM body as it stands.  The call computes every
 * length and the offsets first, reads the total back with one stream synchronisation (like the counters of the seed-extend
 * calls) and stores it in *out_bytes whatever happens next.  out == NULL with out_cap == 0 is a sizing call (out_off is
 * filled) and returns BG_OK; a total above out_cap returns BG_ERR_OPS_CAP before one byte of text is written.
 * BG_ERR_INVALID_ARG: max_hits 0 or above BG_SEED_MAX_HITS; n_contigs 0; BG_SAM_PAIRED with an odd n_reads, with
 * max_hits != 1 or without pairs; BG_SAM_TAG_MD on an index without text; unknown flag bits; a null fm, sp, out_off or
 * out_bytes, or (n_reads > 0) a null contigs, names, fastq text, recs, seq, qual, hits, strand or ops.
 *
 * The record.  A slot is PLACED if its hit has a score (score != BG_MIN_SCORE and strand != BG_HIT_NONE) and
 * [ref_start, ref_end) lies inside one contig, found by binary search of ref_start in `start`: a hit that falls between
 * contigs or runs over a contig's end is not placed and is treated as unmapped everywhere below.  pos = ref_start -
 * contig.start + 1.  Slot k = 0 always writes a line; a slot k > 0 writes a line only with BG_SAM_SECONDARY, and only if
 * it is placed and slot 0 is placed.  The line has eleven TAB-separated fields, then tags, then '\n':
 *    1 QNAME   the FASTQ id bytes, or "*" if id_len == 0.  With BG_SAM_PAIRED a trailing "/1" on mate 1 or "/2" on mate 2
 *              is dropped when id_len > 2.
 *    2 FLAG    in decimal.  0x4 not placed; 0x10 reverse strand and placed; 0x100 for k > 0.  With BG_SAM_PAIRED: 0x1; 0x40
 *              for even r, 0x80 for odd r; 0x8 mate not placed; 0x20 mate placed on the reverse strand; 0x2 when
 *              pairs[p].proper and both mates are placed on one contig.
 *    3 RNAME   the contig's name, or "*".
 *    4 POS     pos, or 0.  A mate that is not placed takes RNAME and POS from a placed mate (SAM 1.4).
 *    5 MAPQ    0 if not placed or k > 0; otherwise multi[r].mapq if multi is given, else 255.  With BG_SAM_PAIRED the records
 *              of bg_seed_extend_pairs_mapq_batch[_dev] go in as multi: each mate's MAPQ, judged against the pair.
 *    6 CIGAR   byte for byte what bg_cigar_batch_dev(hard_clip = 0) writes for hits[slot].aln, or "*" if not placed (or
 *              without operations).
 *    7 RNEXT   "*" when not paired or neither mate is placed; "=" when this line's RNAME is the mate's contig; otherwise
 *              the mate's contig name.
 *    8 PNEXT   the mate's POS field, or 0.
 *    9 TLEN    0 unless both mates are placed on one contig; otherwise max(ref_end) - min(ref_start), positive for the
 *              mate with the smaller ref_start (mate 1 on a tie) and negative for the other.  For a proper pair |TLEN| is
 *              pairs[p].span.
 *   10 SEQ     the read for a forward or unplaced slot, dna::revcomp(read) for a reverse one (the bytes of
 *              bg_revcomp_batch_dev); "*" if the read is empty or k > 0.
 *   11 QUAL    the quality bytes, reversed on the reverse strand; "*" if qual_len != seq_len, if empty, or if k > 0.
 * Tags, on placed lines only, in this order: AS:i:<score>; XS:i:<multi[r].sub_score> with multi, k == 0 and a runner-up
 * (sub_score != BG_MIN_SCORE; with the pairs-mapq records: the mate's best alternative); NM:i:<number of SUBST + INS + DEL operations> with BG_SAM_TAG_NM; MD:Z:<md> with
 * BG_SAM_TAG_MD.  The MD string is built by walking the operations from ref_start with a counter c = 0.  MATCH: c += 1
 * and the text advances.  SUBST: write c, write the text byte, set c = 0; the text advances.  A run of consecutive DEL:
 * write c, '^' and the run's text bytes, set c = 0.  INS: nothing.  At the end write c.  (This yields the specification's
 * 10A5^AC0T3 forms without special cases.)
 * bg_sam_header (host only, no GPU) writes "@HD\tVN:1.6\tSO:unsorted\n", one "@SQ\tSN:<name>\tLN:<len>\n" per contig and
 * "@PG\tID:biogpu\tPN:biogpu\n"; *out_bytes receives the length, out == NULL with out_cap == 0 sizes, BG_ERR_OPS_CAP if
 * out_cap is too small (nothing written).
 * Not covered: supplementary (chimeric) records, read groups.  (Coordinate order and duplicate flags: the section below; BAM
 * records and BGZF framing: the one after it.)  (Mate rescue happens before this call:
 * bg_seed_extend_pairs_rescue_batch[_dev]; a rescued hit is written like any other.)  Known limit: the
 * seed-and-extend windows know nothing of contig boundaries, so a read whose best alignment crosses one is reported
 * unmapped here (not clipped to the contig) even where a slightly worse alignment inside one contig exists. */
typedef struct {            /* one reference sequence inside the indexed text; 32 bytes */
    uint64_t start, len;    /* text[start .. start + len): contigs ascending in start, not overlapping, inside the text without its final sentinel */
    uint64_t name_off;      /* into `names` */
    uint32_t name_len, reserved;
} bg_sam_contig_t;
enum { BG_SAM_PAIRED = 1, BG_SAM_SECONDARY = 2, BG_SAM_TAG_NM = 4, BG_SAM_TAG_MD = 8 };
typedef struct {
    uint32_t flags;         /* BG_SAM_* */
    uint32_t max_hits;      /* K: slots per read in hits / strand (1 after the strands and pairs calls) */
} bg_sam_params_t;
int bg_sam_header(const bg_sam_contig_t* contigs, uint64_t n_contigs, const char* names, char* out, uint64_t out_cap,
                  uint64_t* out_bytes);
/* Device flavour: every d_* pointer in HBM, d_out_off n_reads * K + 1 entries, out_bytes a host pointer; the text pass is
 * asynchronous on `stream`.  Goes through the handle's ctx (scratch): the ctx's single-thread rule applies. */
/* The byte pointers (d_names, d_fastq_text, d_seq, d_qual, d_strand, d_ops, d_out) may be at any address: a line is written 16
 * bytes at a time between its first and last 16-byte boundary in d_out, the columns are read byte by byte. */
int bg_sam_emit_batch_dev(bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* d_contigs,
                          uint64_t n_contigs, const char* d_names, const uint8_t* d_fastq_text, const bg_fastq_record_t* d_recs,
                          const uint8_t* d_seq, const uint8_t* d_qual, const bg_seed_hit_t* d_hits, const uint8_t* d_strand,
                          const uint8_t* d_ops, const bg_multi_hit_t* d_multi, const bg_pair_hit_t* d_pairs, char* d_out,
                          uint64_t out_cap, uint64_t* d_out_off, uint64_t* out_bytes, void* stream);
/* The same with host pointers; ops as the host seed-extend calls return them (aln.ops_off into ops).  The sizes of the
 * FASTQ text, seq, qual, ops and names are taken from the records that point into them. */
int bg_sam_emit_batch(bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* contigs,
                      uint64_t n_contigs, const char* names, const uint8_t* fastq_text, const bg_fastq_record_t* recs,
                      const uint8_t* seq, const uint8_t* qual, const bg_seed_hit_t* hits, const uint8_t* strand,
                      const uint8_t* ops, const bg_multi_hit_t* multi, const bg_pair_hit_t* pairs, char* out, uint64_t out_cap,
                      uint64_t* out_off, uint64_t* out_bytes);

/* ---- coordinate-sorted SAM and duplicate marking (sam_sort.hip; the bodies in csrc/sam_rule.h) ------------------------
 * What the next tool takes: records in coordinate order, PCR duplicates flagged 0x400.  The order of use is
 *   bg_sam_markdup[_dev]         one duplicate byte per read, from the hits and the qualities
 *   bg_sam_emit_dup_batch[_dev]  the writer above with `dup`: SAM text that carries the flags
 *   bg_sam_sort_keys[_dev]       a 64-bit key per slot
 *   bg_sam_sort[_dev]            the lines permuted into key order
 *   bg_sam_header_so             a header that says SO:coordinate
 * rust-bio has none of this; as with the pair and multi rules the definitions are this header's.  PLACED and "writes a line"
 * are the writer's (one definition: csrc/sam_rule.h).
 *
 * bg_sam_markdup.  Only slot K r of read r takes part (K = max_hits); secondary slots never do.
 *   score(r)   the sum of q - phred_offset over the quality bytes q of read r (qual[recs[r].qual_off .. + qual_len)) with
 *              q >= phred_offset + min_qual; a 32-bit integer.
 *   end(r)     exists only if slot K r is placed: the triple (contig, u5, rev) with rev = (strand == BG_HIT_REVERSE) and u5
 *              the unclipped 5' coordinate in the index text: forward u5 = ref_start - aln.xstart, saturating at 0; reverse
 *              u5 = ref_end - 1 + (aln.xlen - aln.xend).  (After the semiglobal extension the clip terms are 0; the rule
 *              holds for any hit record.)  Coordinates are 64-bit throughout.
 *   Without BG_SAM_PAIRED: reads with an end are grouped by end.  In each group the read with the highest score stays, on a
 *              tie the smallest r; every other read of the group gets dup[r] = 1.
 *   With BG_SAM_PAIRED (n_reads even, K = 1, reads 2p and 2p + 1 the mates of pair p):
 *     both mates have an end: order the two ends by (contig, u5, rev, mate number) into lo and hi.  The pair's key is
 *              (lo, hi, whether lo is mate 2), its score the sum of the mates' scores.  Pairs are grouped by key; the
 *              highest score stays, then the smallest p; both mates of every other pair of the group get 1.
 *     exactly one mate has an end (a fragment): if any both-ended pair, kept or not, has lo or hi equal to the fragment's
 *              end, the placed mate gets 1.  Otherwise the fragments are grouped by end among themselves; the highest score
 *              of the placed mate stays, then the smallest r; the placed mates of the rest get 1.  The mate without an end
 *              gets 0.
 *     neither mate has an end: both get 0.
 *   counts (host, 4 entries, read back with one stream synchronisation like the other calls' totals): [0] reads with an
 *              end, [1] reads flagged, [2] pairs flagged, [3] fragments flagged because of a pair's end.
 *   The result does not depend on how a sort breaks ties: every tie of the rule is stated by index and is part of the order
 *   that is sorted by.  BG_ERR_INVALID_ARG: unknown flag bits (anything but BG_SAM_PAIRED); max_hits 0 or above
 *   BG_SEED_MAX_HITS; n_contigs 0; paired with an odd n_reads or max_hits != 1; a null ctx, mp or counts, or (n_reads > 0) a
 *   null contigs, hits, strand, recs, qual or dup.  n_reads == 0 is BG_OK with the counts zero.
 *
 * bg_sam_emit_dup_batch[_dev]: bg_sam_emit_batch[_dev] with `dup` (n_reads entries, optional) behind `pairs`.  Every placed
 *   line of read r (slot 0 and secondary slots) carries 0x400 in FLAG when dup[r] != 0; nothing else in the line changes
 *   (the length of FLAG's decimal text may).  With dup == NULL the output is byte for byte bg_sam_emit_batch[_dev]'s, which
 *   pass a null dup through.
 *
 * bg_sam_sort_keys[_dev]: key[K r + k], n_reads * K entries.  A slot that writes a line and is placed gets ref_start
 *   (contigs ascend in `start`, so this orders by (RNAME's index, POS)); a paired, unplaced slot whose mate is placed gets
 *   the mate's ref_start (its line carries the mate's RNAME and POS); every other slot — unmapped lines with "*", slots that
 *   write no line — gets UINT64_MAX.  BG_ERR_INVALID_ARG as for the writer where it applies: unknown flag bits, max_hits 0
 *   or above BG_SEED_MAX_HITS, n_contigs 0, paired with an odd n_reads or max_hits != 1, a null ctx or sp, or (n_reads > 0)
 *   a null contigs, hits, strand or key.  The device flavour is asynchronous on `stream`.
 *
 * bg_sam_sort[_dev] knows nothing of SAM: it sorts ANY buffer of variable-length records by a 64-bit key.  Record i is
 *   in[in_off[i] .. in_off[i + 1]), in_off ascending with in_off[n_slots] <= in_bytes.  perm is the stable ascending sort of
 *   0 .. n_slots - 1 by key; output record j is input record perm[j]; out_off is the running sum of the permuted lengths
 *   (n_slots + 1 entries).  Records of length 0 stay in the permutation and add no bytes.  out_cap < in_bytes returns
 *   BG_ERR_OPS_CAP with nothing written.  d_out must not overlap d_in.  BG_ERR_INVALID_ARG: a null ctx, out_off or perm, or
 *   (n_slots > 0) a null key, in_off, or (in_bytes > 0) in or out.  The device flavour is asynchronous on `stream`, with no
 *   read-back; with bg_enable_timing on it waits and reports its stable radix sort (rocPRIM) in bg_timing_t.fm_ms and its
 *   permuted copy in bg_timing_t.fill_ms.
 *
 * bg_sam_header_so: bg_sam_header with the sort order named: BG_SAM_SO_UNSORTED gives exactly bg_sam_header's bytes,
 *   BG_SAM_SO_COORDINATE the same with SO:coordinate; anything else is BG_ERR_INVALID_ARG.
 * Not covered: queryname order, optical duplicates, duplicate sets across calls, UMIs. */
enum { BG_SAM_SO_UNSORTED = 0, BG_SAM_SO_COORDINATE = 1 };
typedef struct {
    uint32_t flags;         /* BG_SAM_PAIRED or 0; anything else BG_ERR_INVALID_ARG */
    uint32_t max_hits;      /* K, as in bg_sam_params_t; only slot K r of read r takes part */
    uint32_t phred_offset;  /* 33 for Sanger qualities */
    uint32_t min_qual;      /* quality symbols below it do not count towards a read's score (Picard: 15) */
} bg_markdup_params_t;
int bg_sam_markdup_dev(bg_ctx* ctx, const bg_markdup_params_t* mp, uint64_t n_reads, const bg_sam_contig_t* d_contigs,
                       uint64_t n_contigs, const bg_seed_hit_t* d_hits, const uint8_t* d_strand, const bg_fastq_record_t* d_recs,
                       const uint8_t* d_qual, uint8_t* d_dup, uint64_t* counts, void* stream);
int bg_sam_markdup(bg_ctx* ctx, const bg_markdup_params_t* mp, uint64_t n_reads, const bg_sam_contig_t* contigs,
                   uint64_t n_contigs, const bg_seed_hit_t* hits, const uint8_t* strand, const bg_fastq_record_t* recs,
                   const uint8_t* qual, uint8_t* dup, uint64_t* counts);
int bg_sam_emit_dup_batch_dev(bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* d_contigs,
                              uint64_t n_contigs, const char* d_names, const uint8_t* d_fastq_text, const bg_fastq_record_t* d_recs,
                              const uint8_t* d_seq, const uint8_t* d_qual, const bg_seed_hit_t* d_hits, const uint8_t* d_strand,
                              const uint8_t* d_ops, const bg_multi_hit_t* d_multi, const bg_pair_hit_t* d_pairs, const uint8_t* d_dup,
                              char* d_out, uint64_t out_cap, uint64_t* d_out_off, uint64_t* out_bytes, void* stream);
int bg_sam_emit_dup_batch(bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* contigs,
                          uint64_t n_contigs, const char* names, const uint8_t* fastq_text, const bg_fastq_record_t* recs,
                          const uint8_t* seq, const uint8_t* qual, const bg_seed_hit_t* hits, const uint8_t* strand,
                          const uint8_t* ops, const bg_multi_hit_t* multi, const bg_pair_hit_t* pairs, const uint8_t* dup, char* out,
                          uint64_t out_cap, uint64_t* out_off, uint64_t* out_bytes);
int bg_sam_sort_keys_dev(bg_ctx* ctx, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* d_contigs,
                         uint64_t n_contigs, const bg_seed_hit_t* d_hits, const uint8_t* d_strand, uint64_t* d_key, void* stream);
int bg_sam_sort_keys(bg_ctx* ctx, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* contigs, uint64_t n_contigs,
                     const bg_seed_hit_t* hits, const uint8_t* strand, uint64_t* key);
/* d_in and d_out may be at any address: a record is copied 16 bytes at a time on the alignment of its place in d_out, from
 * whole aligned loads where they lie inside the record and byte by byte at its ends. */
int bg_sam_sort_dev(bg_ctx* ctx, uint64_t n_slots, const uint64_t* d_key, const char* d_in, const uint64_t* d_in_off,
                    uint64_t in_bytes, char* d_out, uint64_t out_cap, uint64_t* d_out_off, uint64_t* d_perm, void* stream);
int bg_sam_sort(bg_ctx* ctx, uint64_t n_slots, const uint64_t* key, const char* in, const uint64_t* in_off, uint64_t in_bytes,
                char* out, uint64_t out_cap, uint64_t* out_off, uint64_t* perm);
int bg_sam_header_so(const bg_sam_contig_t* contigs, uint64_t n_contigs, const char* names, int sort_order, char* out,
                     uint64_t out_cap, uint64_t* out_bytes);

/* ---- BAM records and BGZF framing (bam_emit.hip, bgzf.hip, bgzf_deflate.hip; the bodies in csrc/bam_rule.h) ----------------
 * What every tool behind a mapper reads, from the same hits, without the text in between:
 *   bg_bam_header            "BAM\1", the SAM header text, the reference table (host only, no GPU)
 *   bg_bam_emit_batch[_dev]  one BAM record per hit slot
 *   bg_bgzf_frame[_dev]      any byte stream cut into BGZF blocks
 *   bg_bgzf_deflate[_dev]    ... with deflate-compressed payloads
 * BAM records are variable-length records like SAM lines: bg_sam_sort[_dev] sorts them with bg_sam_sort_keys[_dev]'s keys as
 * they are.  A file is the framed header followed by the framed records with BG_BGZF_EOF (blocks are independent).
 *
 * bg_bam_header: arguments as bg_sam_header_so.  Writes "BAM\1", l_text, the bytes of bg_sam_header_so for the same
 *   arguments (no NUL added), n_ref, and per contig l_name = name_len + 1, the name, a NUL and l_ref; every integer a
 *   little-endian int32.  Sizing call and BG_ERR_OPS_CAP as bg_sam_header.  A contig with len > 2^31 - 1 is legal SAM but has
 *   no l_ref: BG_ERR_UNSUPPORTED.
 *
 * bg_bam_emit_batch[_dev]: the arguments, the conventions and the BG_ERR_INVALID_ARG list of bg_sam_emit_dup_batch[_dev]
 *   (dup optional); out is bytes: one contiguous buffer, out_off with n_reads * K + 1 entries, a slot that writes no line has
 *   length 0; a length pass, a scan, one read-back of the total with one stream synchronisation; out == NULL with
 *   out_cap == 0 sizes; BG_ERR_OPS_CAP before a byte is written; byte pointers at any address.
 *   THE RULE: the record of a slot is the BAM encoding (SAM v1.6, section 4.2) of the SAM line bg_sam_emit_dup_batch writes
 *   for that slot.
 *     block_size           the record's length minus 4
 *     refID / next_refID   the contig index of RNAME / RNEXT; "=" resolved to the index, "*" gives -1
 *     pos / next_pos       POS - 1 / PNEXT - 1 (-1 for 0)
 *     tlen, mapq, flag     the line's
 *     bin                  the specification's reg2bin(pos, end), end = pos + the reference bases the CIGAR consumes, or
 *                          pos + 1 where that is 0 or the line has no CIGAR; pos = -1 gives 4680
 *     read_name            QNAME and a NUL; "*" stays "*"
 *     cigar                len << 4 | op with MIDNSHP=X -> 0 .. 8, on the letters bg_cigar_batch_dev(hard_clip = 0) writes;
 *                          "*" gives n_cigar_op = 0.  More than 65 535 operations: n_cigar_op = 2 holds <l_seq>S<reference
 *                          length>N and the operations go into a CG:B:I tag behind the other tags (section 4.2.2)
 *     seq                  4 bits a base, high nibble first, codes from "=ACMGRSVTWYHKDBN", lower case as upper case, every
 *                          other byte 15, an odd length padded with 0; "*" gives l_seq = 0
 *     qual                 q - 33 modulo 256 per byte; "*" with l_seq > 0 gives l_seq bytes 0xFF
 *     tags                 in the line's order.  AS, XS, NM: the smallest integer type that holds the value (htslib's parse
 *                          rule): c, s, i for a negative one, C, S, I otherwise.  MD: Z with a NUL.
 *   Not representable: a slot whose QNAME exceeds 254 bytes; a slot that writes a line on, or borrows RNAME from, or names as
 *   RNEXT a contig with len > 2^31 - 1.  The length pass counts such slots (they count 0 bytes) and the count comes back with
 *   the total; the call then returns BG_ERR_UNSUPPORTED before a byte is written, with *out_bytes set.
 *
 * bg_bgzf_frame[_dev] knows nothing of BAM.  The input is cut into payloads of 65 280 bytes (0xff00, htslib's), the last one
 *   shorter; each becomes one block: the 18-byte gzip header (MTIME 0, XFL 0, OS 255, the BC subfield with BSIZE - 1), a stored
 *   deflate block (01, LEN, NLEN, the payload), CRC-32 and ISIZE — 31 bytes around the payload, 65 311 for a full block.  This
 *   is htslib's level 0; every BGZF reader accepts it.  out_bytes = in_bytes + 31 * ceil(in_bytes / 65280), plus 28 for the
 *   end-of-file block with BG_BGZF_EOF; in_bytes == 0 gives no block (and the end-of-file block if asked).  Every offset is
 *   closed-form: byte i of the input is byte i + 31 * (i / 65280) + 23 of the output.  Nothing is read back; the device
 *   flavour is asynchronous on `stream`.  out == NULL with out_cap == 0 sizes; BG_ERR_OPS_CAP if out_cap is too small (nothing
 *   written); BG_ERR_INVALID_ARG: unknown flag bits, a null ctx or out_bytes, a null in with in_bytes > 0.  d_in and d_out may
 *   be at any address and must not overlap.
 *
 * bg_bgzf_deflate[_dev] (bgzf_deflate.hip; the bodies in csrc/bgzf_deflate_rule.h): bg_bgzf_frame with the payloads
 *   compressed.  THE RULE: the input is cut into payloads of 65 280 bytes exactly as bg_bgzf_frame cuts it; each becomes one
 *   gzip member with the same 18-byte header, CRC-32 and ISIZE around ONE deflate block (BFINAL set) in one of three
 *   encodings: stored, fixed Huffman codes, dynamic Huffman codes — the one with the fewest bits by exact count (stored:
 *   8 * (len + 5)); stored wins a tie, then fixed.  A block therefore never exceeds len + 31 bytes and BSIZE always fits; a
 *   block that comes out stored is bg_bgzf_frame's block byte for byte.  BG_BGZF_EOF appends the same 28 bytes.
 *   The tokens: a greedy parse from byte 0 over matches of 3 .. 258 bytes at distances 1 .. 32 768 that never start in front
 *   of the payload nor run behind it; blocks are independent.  Dynamic codes are length-limited Huffman codes (15 bits; 7 for
 *   the code-length alphabet) with HLIT, HDIST and HCLEN trimmed and always at least one distance code.
 *   The bytes are a function of the payload alone: the same on every run, at every alignment of source and destination, and
 *   from the CPU run of the bodies (tests/bgzf_deflate_host_bodies.cpp); nothing that decides a byte depends on the order in
 *   which lanes or wavefronts run.
 *   out_cap must hold the stored bound, bg_bgzf_frame's out_bytes for the same arguments: BG_ERR_OPS_CAP otherwise (nothing
 *   written); out == NULL with out_cap == 0 returns that bound in *out_bytes.  After a real call *out_bytes is the actual
 *   size: the total is read back once, with one stream synchronisation (as bg_bam_emit_batch_dev).  block_off may be NULL;
 *   otherwise it receives ceil(in_bytes / 65280) + 1 offsets into the output: the start of every block, then the end of the
 *   last (the end-of-file block is not counted) — the table a virtual offset needs now that block sizes are not closed-form.
 *   BG_ERR_INVALID_ARG as bg_bgzf_frame.  Scratch is the ctx's and does not grow with the input (sub-batches of 512 blocks).
 * Not covered: CSI indexes (the BAI index: the section below), read groups, supplementary records; lazy matching, hash chains,
 * compression levels. */
enum { BG_BGZF_EOF = 1 };
int bg_bam_header(const bg_sam_contig_t* contigs, uint64_t n_contigs, const char* names, int sort_order, uint8_t* out,
                  uint64_t out_cap, uint64_t* out_bytes);
int bg_bam_emit_batch_dev(bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* d_contigs,
                          uint64_t n_contigs, const char* d_names, const uint8_t* d_fastq_text, const bg_fastq_record_t* d_recs,
                          const uint8_t* d_seq, const uint8_t* d_qual, const bg_seed_hit_t* d_hits, const uint8_t* d_strand,
                          const uint8_t* d_ops, const bg_multi_hit_t* d_multi, const bg_pair_hit_t* d_pairs, const uint8_t* d_dup,
                          uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off, uint64_t* out_bytes, void* stream);
int bg_bam_emit_batch(bg_fm* fm, const bg_sam_params_t* sp, uint64_t n_reads, const bg_sam_contig_t* contigs,
                      uint64_t n_contigs, const char* names, const uint8_t* fastq_text, const bg_fastq_record_t* recs,
                      const uint8_t* seq, const uint8_t* qual, const bg_seed_hit_t* hits, const uint8_t* strand,
                      const uint8_t* ops, const bg_multi_hit_t* multi, const bg_pair_hit_t* pairs, const uint8_t* dup, uint8_t* out,
                      uint64_t out_cap, uint64_t* out_off, uint64_t* out_bytes);
int bg_bgzf_frame_dev(bg_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes, uint32_t flags, uint8_t* d_out, uint64_t out_cap,
                      uint64_t* out_bytes, void* stream);
int bg_bgzf_frame(bg_ctx* ctx, const uint8_t* in, uint64_t in_bytes, uint32_t flags, uint8_t* out, uint64_t out_cap,
                  uint64_t* out_bytes);
int bg_bgzf_deflate_dev(bg_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes, uint32_t flags, uint8_t* d_out, uint64_t out_cap,
                        uint64_t* d_block_off, uint64_t* out_bytes, void* stream);
int bg_bgzf_deflate(bg_ctx* ctx, const uint8_t* in, uint64_t in_bytes, uint32_t flags, uint8_t* out, uint64_t out_cap,
                    uint64_t* block_off, uint64_t* out_bytes);

/* ---- reading BGZF: the block table and the payloads (bgzf_inflate.hip; the bodies in csrc/bgzf_inflate_rule.h) ------------
 * The way back from a .bam or a bgzipped .fastq.gz that lies in HBM: bg_bgzf_blocks[_dev] finds the members, bg_bgzf_inflate
 * [_dev] inflates every one to its final place and checks it; the text then goes to bg_fastq_parse_dev, a BAM stream through
 * bg_bam_header_parse and bg_bam_records_dev (the section "reading BAM" below) to bg_bam_reads_dev, bg_bam_index_blocks_dev
 * and bg_sam_sort_dev, without the bytes visiting the host.
 *
 * bg_bgzf_blocks[_dev].  THE RULE: the stream is a chain of gzip members from byte 0; member b starts at block_off[b] and is
 *   BSIZE + 1 bytes long; the chain must end exactly at in_bytes.  block_off gets n_blocks + 1 entries, the last in_bytes (the
 *   table bg_bgzf_deflate fills; bg_bam_index takes it as it is); out_off gets n_blocks + 1 entries, the exclusive prefix sum
 *   of the members' ISIZE fields; *out_bytes = out_off[n_blocks].  Empty members (ISIZE 0, the 28-byte end-of-file block
 *   among them) are blocks like any other.  The chain is the truth, not the signatures: payload bytes that look like a member
 *   header are never reported.
 *   Accepted header, exactly: 1f 8b 08 04, any MTIME / XFL / OS, XLEN = 6, the subfield 42 43 02 00 BSIZE.  What stands at
 *   a chain position instead decides the error, in this order: no gzip magic (1f 8b) or fewer than 12 bytes left:
 *   BG_ERR_INVALID_ARG; CM != 8, FLG != 4 or XLEN != 6: BG_ERR_UNSUPPORTED; fewer than 18 bytes left: BG_ERR_INVALID_ARG;
 *   another subfield: BG_ERR_UNSUPPORTED; BSIZE + 1 < 28, a member running past in_bytes, ISIZE > 65 536:
 *   BG_ERR_INVALID_ARG.  Both leave the tables unwritten, *first_bad = the index of the offending member (optional;
 *   UINT64_MAX otherwise) and *n_blocks / *out_bytes = the members in front of it and their ISIZE sum.
 *   in_bytes == 0 gives 0 blocks.  Null tables with cap_blocks == 0 size the call (*n_blocks, *out_bytes); cap_blocks <
 *   n_blocks gives BG_ERR_OPS_CAP with both set and the tables unwritten (they hold cap_blocks + 1 entries).
 *   BG_ERR_TOO_LARGE: in_bytes >= 2^35.  n_blocks, out_bytes and the error are read back once, with one stream
 *   synchronisation (as bg_bam_emit_batch_dev).  Scratch is the ctx's: 18 bytes per 16 input bytes, the bound on how many
 *   positions can carry an accepted member (two of them lie at least 16 bytes apart: the fixed header bytes forbid every closer
 *   pair but the one 6 bytes apart, and that one needs BSIZE = 6, which 28 <= BSIZE + 1 refuses).
 *
 * bg_bgzf_inflate[_dev].  THE RULE: block b's deflate stream is in[block_off[b] + 18 .. block_off[b + 1] - 8), its payload
 *   goes to out[out_off[b] .. out_off[b + 1]).  The bytes are RFC 1951's: any number of deflate blocks (stored, fixed,
 *   dynamic, in any mix) up to the one with BFINAL.  A block is good if the stream decodes, ends inside its last byte (at
 *   most 7 padding bits, no unused byte), produces exactly out_off[b + 1] - out_off[b] bytes, that is the trailer's ISIZE, and
 *   the CRC-32 of those bytes is the trailer's.  Which code sets are legal is zlib's rule: an over-subscribed set is an error;
 *   an incomplete one too, except a literal/length or distance set whose longest code is 1 bit; the code-length alphabet's set
 *   must be complete; no distance code at all is legal (an error once a length symbol appears); symbol 256 must have a code;
 *   HLIT > 286, HDIST > 30, a repeat with nothing before it or running past HLIT + HDIST are errors; the unassigned code of
 *   an incomplete set, literal/length symbols 286 / 287 and distance codes 30 / 31 are errors where they are decoded; a
 *   distance beyond the bytes this block has produced is an error (blocks share no window).
 *   status (optional, one byte a block) gets BG_INFLATE_OK or the FIRST error in decode order; size and CRC are checked last,
 *   in that order.  BAD_SYMBOL is every code that decodes to nothing usable, distance codes included; BAD_DISTANCE is the
 *   distance that reaches too far.
 *   Any bad block: BG_ERR_INVALID_ARG with *first_bad (optional) = the lowest bad block; good blocks' payloads are written
 *   in full, a bad block's bytes inside its own range are unspecified.  Whatever the input, every read lies in the block's
 *   own member and every write in its own output range.
 *   BG_ERR_OPS_CAP if out_cap < out_off[n_blocks]; BG_ERR_INVALID_ARG with *first_bad = the first offending block if the
 *   tables are not ascending, block_off[n_blocks] > in_bytes, an output range exceeds 65 536 bytes or a member is shorter
 *   than 28 or longer than 65 536 bytes; a null ctx, or (n_blocks > 0) a null in or table, or a null out with out_cap > 0 (a null out with out_cap == 0 serves a
 *   stream of empty members); BG_ERR_TOO_LARGE: n_blocks >= 2^31.  Nothing is
 *   written in these cases.  One read-back (the error words) with one stream synchronisation.  d_in and d_out may be at any
 *   address and must not overlap.
 * Not covered: plain (non-BGZF) gzip, members with further extra subfields, .gzi / tabix, speculative decoding inside a
 * block. */
enum {
    BG_INFLATE_OK = 0,
    BG_INFLATE_BAD_TYPE = 1,     /* deflate block type 3 */
    BG_INFLATE_BAD_STORED = 2,   /* LEN is not ~NLEN */
    BG_INFLATE_BAD_LENGTHS = 3,  /* the dynamic header: counts, repeats, an illegal code set, no code for 256 */
    BG_INFLATE_BAD_SYMBOL = 4,   /* a code that is not assigned, literal/length 286 / 287, distance code 30 / 31 */
    BG_INFLATE_BAD_DISTANCE = 5, /* a distance beyond the bytes produced so far */
    BG_INFLATE_TRUNCATED = 6,    /* bits wanted beyond the stream */
    BG_INFLATE_TRAILING = 7,     /* unused bytes behind the final deflate block */
    BG_INFLATE_SIZE = 8,         /* not the output range's length, or not ISIZE */
    BG_INFLATE_CRC = 9
};
int bg_bgzf_blocks_dev(bg_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes, uint64_t* d_block_off, uint64_t* d_out_off,
                       uint64_t cap_blocks, uint64_t* n_blocks, uint64_t* out_bytes, uint64_t* first_bad, void* stream);
int bg_bgzf_blocks(bg_ctx* ctx, const uint8_t* in, uint64_t in_bytes, uint64_t* block_off, uint64_t* out_off, uint64_t cap_blocks,
                   uint64_t* n_blocks, uint64_t* out_bytes, uint64_t* first_bad);
int bg_bgzf_inflate_dev(bg_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes, uint64_t n_blocks, const uint64_t* d_block_off,
                        const uint64_t* d_out_off, uint8_t* d_out, uint64_t out_cap, uint8_t* d_status, uint64_t* first_bad,
                        void* stream);
int bg_bgzf_inflate(bg_ctx* ctx, const uint8_t* in, uint64_t in_bytes, uint64_t n_blocks, const uint64_t* block_off,
                    const uint64_t* out_off, uint8_t* out, uint64_t out_cap, uint8_t* status, uint64_t* first_bad);

/* ---- the BAI index of a coordinate-sorted BAM stream (bam_index.hip; the bodies in csrc/bam_index_rule.h) ----------------
 * What makes the file above usable by region: the bytes of the .bai file (SAM v1.6, section 5.2) beside it, from what is in
 * HBM when the file is framed.  bg_bam_index[_dev] reads BAM RECORDS, not hits: slot i is recs[off[i] .. off[i + 1]) — the pair
 * bg_bam_emit_batch_dev and bg_sam_sort_dev leave — and anything that is a coordinate-sorted run of BAM records will do.
 * contigs gives n_ref = n_contigs and the contig lengths (start and the names are not read).  block_off and base say how the
 * stream was framed: block_off is the table bg_bgzf_deflate[_dev] filled for these records (ceil(off[n_slots] / 65280) + 1
 * entries), or NULL where bg_bgzf_frame[_dev] framed them (closed form); base is the file offset of the first block of that
 * framing call: the length of the framed header.
 * THE RULE.  The bytes are a function of the inputs alone.
 *   slots      a slot of length 0 is ignored everywhere.  Of a record the call uses refID, pos, l_read_name, n_cigar_op, flag
 *              and the CIGAR words.  end = pos + the reference bases the CIGAR consumes (M, D, N, =, X), pos + 1 where that
 *              sum is 0 (the placeholder <l_seq>S<len>N of a record with a CG tag is no case of its own).  The bin is the
 *              specification's reg2bin(pos, end), recomputed: the record's own bin field is not read.
 *   voff(o)    of byte o of the stream: with a table (base + block_off[o / 65280]) << 16 | o % 65280; without one
 *              (base + 65311 * (o / 65280)) << 16 | o % 65280.  o = off[n_slots] is legal even where it is a multiple of 65 280:
 *              the table's last entry serves it.
 *   indexed    are the records with refID >= 0, unmapped mates that borrow a position included (as in htslib); those with
 *              refID < 0 only count into n_no_coor.
 *   chunks     over the indexed records of one reference in file order, every maximal run of consecutive records with the
 *              same bin is one chunk (voff(start of the first), voff(end of the last)); a bin's chunks are listed in file
 *              order.  No further merging and no bin compression: readers need neither.
 *   linear     a reference with records has n_intv = ((max end - 1) >> 14) + 1 (0 where max end is 0); ioffset[w] is
 *              voff(start) of its first record in file order whose end > w << 14.  On sorted input that is the smallest start
 *              offset among the records overlapping window w, an empty window taking the next non-empty window's value.
 *   pseudo-bin 37450, for every reference with records: chunk 0 = (voff(start of its first record), voff(end of its last)),
 *              chunk 1 = (its records with FLAG 0x4 clear, those with it set).
 *   bytes      all integers little-endian: "BAI\1", n_ref; per reference n_bin, the bins with at least one chunk in ascending
 *              bin number (bin, n_chunk, the chunks), the pseudo-bin last (n_bin counts it), n_intv, the offsets; a reference
 *              without records is n_bin = 0, n_intv = 0; then n_no_coor (uint64), always.  (htslib lists bins in hash order:
 *              byte identity with samtools index is no goal.)
 * Checks.  Each leaves nothing written and sets *first_bad (optional; UINT64_MAX where no slot is to blame) to the first
 *   offending slot, whose kind decides the status.  BG_ERR_INVALID_ARG: a non-empty slot shorter than 36 bytes, one whose
 *   block_size + 4 is not its length, one whose name, CIGAR, bases and qualities run past its end, refID >= n_contigs,
 *   pos < -1, end beyond the contig's length, off[i + 1] < off[i], or a record that sorts before the previous non-empty slot by
 *   ((uint32) refID, pos): the input must be coordinate-sorted, unplaced records last.  BG_ERR_UNSUPPORTED: a record with
 *   nothing else wrong whose end > 2^29, where BAI's bins stop.  BG_ERR_OPS_CAP if out_cap is too small (*out_bytes says what
 *   is needed); out == NULL with out_cap == 0 sizes.  BG_ERR_TOO_LARGE: n_slots >= 2^32 - 1.  Also BG_ERR_INVALID_ARG: a null
 *   ctx or out_bytes, (n_slots > 0) a null recs or off, (n_contigs > 0) a null contigs.
 * The errors and the total are read back once, with one stream synchronisation (as bg_bam_emit_batch_dev); the bytes are then
 * stored asynchronously on `stream`.  d_recs and d_out may be at any address: record fields are read byte by byte.  Scratch
 * is the ctx's, 17 words a slot and 6 a contig; nothing grows with the windows or with n_contigs x bins.
 * Not covered: CSI indexes (contigs beyond 2^29), htslib's bin compression and chunk merging, unsorted input, .gzi / tabix. */
int bg_bam_index_dev(bg_ctx* ctx, uint64_t n_slots, const uint8_t* d_recs, const uint64_t* d_off, const bg_sam_contig_t* d_contigs,
                     uint64_t n_contigs, const uint64_t* d_block_off, uint64_t base, uint8_t* d_out, uint64_t out_cap,
                     uint64_t* out_bytes, uint64_t* first_bad, void* stream);
int bg_bam_index(bg_ctx* ctx, uint64_t n_slots, const uint8_t* recs, const uint64_t* off, const bg_sam_contig_t* contigs,
                 uint64_t n_contigs, const uint64_t* block_off, uint64_t base, uint8_t* out, uint64_t out_cap, uint64_t* out_bytes,
                 uint64_t* first_bad);

/* ---- reading BAM: header, record table, reads, keys, index (bam_read.hip, bam_index.hip; the bodies in csrc/bam_read_rule.h) ----
 * What turns the inflated stream of any .bam (bg_bgzf_blocks / bg_bgzf_inflate above) into what the rest of the library takes:
 *   bg_bam_header_parse        the inverse of bg_bam_header: contigs, names, the SAM text, where the records start (host only)
 *   bg_bam_records[_dev]       the record table `off`: with recs = the stream, the pair bg_bam_index and bg_sam_sort take
 *   bg_bam_reads[_dev]         records -> the five FASTQ columns (uBAM in, a mapped BAM to be re-mapped)
 *   bg_bam_sort_keys[_dev]     a coordinate key per record, for bg_sam_sort[_dev]
 *   bg_bam_index_blocks[_dev]  bg_bam_index for a stream in any framing, from bg_bgzf_blocks' tables
 * `off` holds ABSOLUTE offsets into the stream: off[0] = body_off, record i is bam[off[i] .. off[i + 1]).
 *
 * bg_bam_header_parse.  in[0 .. bytes) is a prefix of the stream.  Fills contigs[i] (len = l_ref, name_off / name_len into
 *   `names`, the names back to back without their NULs, start = sum over j < i of (len_j + 1): the layout of
 *   bg_fasta_reference without BG_FASTA_REF_FMD, so bg_bam_sort_keys gives the keys bg_sam_sort_keys gives the hits),
 *   *text_off / *text_len (the SAM header text inside the prefix) and *body_off (the first record).  A prefix that ends inside
 *   the header: BG_ERR_OPS_CAP with *need = the smallest length known to be required so far (> bytes, never beyond the
 *   header's end: 9 bytes are counted for every reference not yet seen); a caller that fetches max(need, 2 * bytes) each time
 *   copies a logarithmic number of prefixes.  BG_ERR_INVALID_ARG: a wrong magic, a negative l_text, n_ref or l_ref, an
 *   l_name below 1, a name whose last byte is not NUL.  Null tables with zero caps size the call (*n_contigs,
 *   *names_bytes); caps that are too small: BG_ERR_OPS_CAP with the counts set, *need = 0 and nothing written.
 *
 * bg_bam_records[_dev].  THE RULE: the records are the chain from body_off — a record at o is followed by one at
 *   o + 4 + block_size — and the chain must end exactly at in_bytes.  A position o carries an accepted record when: at least
 *   36 bytes are left; block_size >= 32 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq (in 64 bits; block_size is
 *   unsigned); o + 4 + block_size <= in_bytes; l_read_name >= 1 and the name's last byte is NUL; l_seq >= 0; refID and
 *   next_refID lie in [-1, n_ref); pos >= -1 and next_pos >= -1.  What stands at a chain position without being accepted is
 *   the error: BG_ERR_INVALID_ARG, *first_bad (optional; UINT64_MAX otherwise) = *n_records = the records in front of it,
 *   the table unwritten.  The chain is the truth: bytes inside a record that look like one (qualities, a B array, a Z tag)
 *   are never reported.  body_off == in_bytes gives 0 records (off[0] = in_bytes).  A null off with cap_records == 0 sizes;
 *   cap_records < n_records: BG_ERR_OPS_CAP with *n_records set and the table unwritten (it holds cap_records + 1
 *   entries).  BG_ERR_TOO_LARGE: in_bytes >= 2^35, or 2^32 - 1 or more candidates (a 32-bit jump index).  BG_ERR_INVALID_ARG
 *   also: a null ctx or n_records, a null stream with in_bytes > 0, body_off > in_bytes.  *n_candidates (optional): the
 *   positions from body_off on that carry an accepted record, the chain's and the fakes.
 *   Unlike BGZF members, accepted positions have no minimum distance (two may lie 4 bytes apart) and no bound short of one
 *   a position: the candidates are counted first and that total is read back to size the scratch (the ctx's, 18 bytes a
 *   candidate; BG_ERR_OOM with nothing written where it cannot be had), then n_records and the error: TWO stream
 *   synchronisations, one more than bg_bgzf_blocks.
 *
 * bg_bam_reads[_dev].  prm: flags (BG_BAM_READS_ORIGINAL), require, exclude.  THE RULE: a record is kept when
 *   (flag & require) == require && (flag & exclude) == 0; read j is the j-th kept record in file order (mates are adjacent
 *   exactly where they are in the file).  A slot of length 0 is skipped.  recs[j]: id_off = off + 36 into the stream (the
 *   stream stands where the other calls take d_fastq_text), id_len = l_read_name - 1, 0 for the name "*"; has_desc = 0,
 *   desc_len = 0, desc_off = id_off + id_len; seq: one byte a base from "=ACMGRSVTWYHKDBN", high nibble first; qual: each
 *   byte + 33 modulo 256, qual_len = 0 where l_seq > 0 and the first quality byte is 0xFF (the SAM writer then writes "*", as
 *   before the record was encoded); seq_off / qual_off as bg_fastq_parse fills them (n_reads + 1 entries); check is
 *   Record::check on these fields (a base "=" is BG_FQCHECK_INVALID_SEQ).  With BG_BAM_READS_ORIGINAL a record with FLAG 0x10
 *   gives the bytes bg_revcomp_batch_dev gives for its bases ("=" stays) and its qualities reversed.  src (optional):
 *   src[j] = the slot of read j.  A null recs (all caps 0, every output null) sizes: *n_reads, *seq_bytes, *qual_bytes;
 *   cap_reads, seq_cap or qual_cap too small: BG_ERR_OPS_CAP with the three set and nothing written.
 *   BG_ERR_INVALID_ARG with *first_bad = the first non-empty slot that is not exactly one accepted record by the verdict
 *   above (the table may come from elsewhere; off must lie inside the stream); unknown flag bits; null pointers.
 *   BG_ERR_TOO_LARGE: n_records >= 2^32 - 1.  One read-back with one stream synchronisation; the write pass is then
 *   asynchronous on `stream`.  Byte pointers at any address: record bytes are read byte by byte, seq / qual are stored 16
 *   bytes wide between their own 16-byte boundaries.
 *
 * bg_bam_sort_keys[_dev].  key[i] = contigs[refID].start + pos where refID >= 0 and pos >= 0, UINT64_MAX otherwise and for a
 *   slot of length 0.  With bg_bam_header_parse's start this is bg_sam_sort_keys' key of the slot the record was written
 *   from.  Checks as bg_bam_reads, with n_ref = n_contigs.
 *
 * bg_bam_index_blocks[_dev].  bg_bam_index[_dev] with recs = the stream, off absolute, and the framing given by n_blocks,
 *   block_off and out_off as bg_bgzf_blocks fills them (n_blocks + 1 rows each; not checked), no base.  Everything in THE
 *   RULE of bg_bam_index holds except voff(o): b is the first block with out_off[b + 1] > o; where there is none (o is the
 *   stream's length) the first block with out_off[b] == o, the closing row where no block has; voff = block_off[b] << 16 |
 *   (o - out_off[b]).  Empty members in front of a byte are skipped, the stream's end points at the end-of-file block where
 *   there is one.
 * Not covered: CSI / tabix / .gzi, collating mates by name, aux tags as columns, CRAM, SAM text in, header lines beyond
 * what the text carries (the text is handed back, not interpreted). */
enum { BG_BAM_READS_ORIGINAL = 1 };
typedef struct {
    uint32_t flags;     /* BG_BAM_READS_* */
    uint16_t require;   /* FLAG bits a kept record has */
    uint16_t exclude;   /* FLAG bits a kept record lacks */
} bg_bam_reads_t;
int bg_bam_header_parse(const uint8_t* in, uint64_t bytes, bg_sam_contig_t* contigs, uint64_t cap_contigs, char* names,
                        uint64_t names_cap, uint64_t* n_contigs, uint64_t* names_bytes, uint64_t* text_off, uint64_t* text_len,
                        uint64_t* body_off, uint64_t* need);
int bg_bam_records_dev(bg_ctx* ctx, const uint8_t* d_bam, uint64_t in_bytes, uint64_t body_off, uint64_t n_ref, uint64_t* d_off,
                       uint64_t cap_records, uint64_t* n_records, uint64_t* n_candidates, uint64_t* first_bad, void* stream);
int bg_bam_records(bg_ctx* ctx, const uint8_t* bam, uint64_t in_bytes, uint64_t body_off, uint64_t n_ref, uint64_t* off,
                   uint64_t cap_records, uint64_t* n_records, uint64_t* n_candidates, uint64_t* first_bad);
int bg_bam_reads_dev(bg_ctx* ctx, const bg_bam_reads_t* prm, uint64_t n_records, const uint8_t* d_bam, const uint64_t* d_off,
                     uint64_t n_ref, bg_fastq_record_t* d_recs, uint64_t cap_reads, uint8_t* d_seq, uint64_t seq_cap,
                     uint64_t* d_seq_off, uint8_t* d_qual, uint64_t qual_cap, uint64_t* d_qual_off, uint64_t* d_src,
                     uint64_t* n_reads, uint64_t* seq_bytes, uint64_t* qual_bytes, uint64_t* first_bad, void* stream);
int bg_bam_reads(bg_ctx* ctx, const bg_bam_reads_t* prm, uint64_t n_records, const uint8_t* bam, const uint64_t* off,
                 uint64_t n_ref, bg_fastq_record_t* recs, uint64_t cap_reads, uint8_t* seq, uint64_t seq_cap, uint64_t* seq_off,
                 uint8_t* qual, uint64_t qual_cap, uint64_t* qual_off, uint64_t* src, uint64_t* n_reads, uint64_t* seq_bytes,
                 uint64_t* qual_bytes, uint64_t* first_bad);
int bg_bam_sort_keys_dev(bg_ctx* ctx, uint64_t n_records, const uint8_t* d_bam, const uint64_t* d_off,
                         const bg_sam_contig_t* d_contigs, uint64_t n_contigs, uint64_t* d_key, uint64_t* first_bad, void* stream);
int bg_bam_sort_keys(bg_ctx* ctx, uint64_t n_records, const uint8_t* bam, const uint64_t* off, const bg_sam_contig_t* contigs,
                     uint64_t n_contigs, uint64_t* key, uint64_t* first_bad);
int bg_bam_index_blocks_dev(bg_ctx* ctx, uint64_t n_slots, const uint8_t* d_recs, const uint64_t* d_off,
                            const bg_sam_contig_t* d_contigs, uint64_t n_contigs, uint64_t n_blocks, const uint64_t* d_block_off,
                            const uint64_t* d_out_off, uint8_t* d_out, uint64_t out_cap, uint64_t* out_bytes, uint64_t* first_bad,
                            void* stream);
int bg_bam_index_blocks(bg_ctx* ctx, uint64_t n_slots, const uint8_t* recs, const uint64_t* off, const bg_sam_contig_t* contigs,
                        uint64_t n_contigs, uint64_t n_blocks, const uint64_t* block_off, const uint64_t* out_off, uint8_t* out,
                        uint64_t out_cap, uint64_t* out_bytes, uint64_t* first_bad);

/* ---- pileup: counters per reference position from sorted BAM records (bam_pileup.hip; the bodies in csrc/bam_pileup_rule.h) ----
 * What lies over each reference position of a batch of regions: one row of counters a position, from a coordinate-sorted run
 * of BAM records in HBM.  (d_recs, d_off) is the pair bg_bam_index[_dev] takes: bg_bam_emit_batch_dev + bg_sam_sort_dev leave
 * it, and so does bg_bam_records_dev as (the stream, off).  contigs gives n_ref = n_contigs and the contig lengths.
 * THE RULE.  The bytes are a function of the inputs alone (integer counts; no float, no order of arrival).
 *   slots      a slot of length 0 is ignored everywhere.
 *   checks     on every non-empty slot: those of bg_bam_index as they stand (length, block_size, fields inside the record,
 *              refID < n_contigs, pos >= -1, end inside the contig, off[i + 1] >= off[i]; end > 2^29 is BG_ERR_UNSUPPORTED:
 *              lifting that limit belongs with CSI); a slot must not sort before the previous non-empty one by ((uint32)
 *              refID, pos); where n_cigar_op > 0 and l_seq > 0 the lengths of M, I, S, =, X must sum to l_seq; an operation
 *              code above 9 is refused (9, htslib's B, is taken and consumes nothing).  All of these: BG_ERR_INVALID_ARG.
 *              The placeholder of a CG tag — n_cigar_op == 2, the first op <l_seq>S, the second N, refID >= 0 — is
 *              BG_ERR_UNSUPPORTED: the real CIGAR sits in a tag this call does not read, and counting the placeholder would
 *              be silently wrong.  On any refusal *first_bad (optional) is the first offending slot, its kind decides the
 *              status (INVALID before UNSUPPORTED), and nothing is written.
 *   kept       a record is kept when refID >= 0, pos >= 0, FLAG 0x4 is clear (whatever `exclude` says),
 *              (flag & require) == require, (flag & exclude) == 0 and mapq >= min_mapq.
 *   the walk   of a kept record starts with r = pos, q = 0.  M, =, X of length n: position r + k (k < n) receives one count
 *              — with l_seq == 0 in column OTHER, no quality test; otherwise none if qual[q + k] < min_baseq (unsigned, on
 *              the raw byte: the absent quality 0xFF always passes), else in the column the 4-bit code of base q + k picks:
 *              1 A, 2 C, 4 G, 8 T, everything else OTHER —; r += n, q += n.  I: one count in column INS at r - 1 when
 *              r > pos (the anchor is the reference base in front; an insertion in front of the record's first reference
 *              base is dropped; every I operation counts one); q += n.  D: DEL at r .. r + n - 1; r += n.  N: SKIP at
 *              r .. r + n - 1; r += n.  S: q += n.  H, P: nothing.
 *   columns    without BG_PILEUP_STRANDS a row is BG_PILEUP_COLS = 8 uint32.  With it a row is 16: columns 0 .. 7 hold the
 *              records with FLAG 0x10 clear, 8 .. 15 those with it set.  Depth is the caller's sum of columns 0 .. 4, plus
 *              DEL if wanted.
 *   regions    0-based, half-open, in any order; they may overlap or repeat.  Each must satisfy 0 <= ref < n_contigs and
 *              0 <= beg <= end <= contigs[ref].len, else BG_ERR_INVALID_ARG with *first_bad = UINT64_MAX (looked at before
 *              the slots).  row_off[r] = the sum of the lengths of the regions in front of r; position p of region r is row
 *              row_off[r] + p - beg, W = 8 or 16 adjacent uint32.  Every row of every region is written, zeros included, and
 *              holds exactly what the region would get in a call of its own; nothing behind row n_rows is touched.
 *              d_row_off (optional) receives the n_regions + 1 offsets.
 *   sizing     a null d_rows with rows_cap == 0 sizes the call: *n_rows, every check still made, nothing written (d_row_off
 *              included).  rows_cap < n_rows: BG_ERR_OPS_CAP with *n_rows set and nothing written.
 *   limits     BG_ERR_TOO_LARGE: n_slots >= 2^32 - 1, n_regions >= 2^24, n_rows >= 2^32.  BG_ERR_INVALID_ARG also: unknown
 *              flag bits, reserved != 0, a null ctx, prm or n_rows, a null d_rows with rows_cap > 0, (n_slots > 0) a null
 *              recs or off, (n_contigs > 0) a null contigs, (n_regions > 0) a null regions.
 * d_rows is 4-byte aligned (rows go out 16 bytes wide where it is 16-byte aligned, as dwords otherwise); d_recs may sit at any
 * address.  The errors and the total are read back once, with one stream synchronisation; the rows are then written
 * asynchronously on `stream`.  Scratch is the ctx's: 33 bytes a slot and 24 a region; nothing grows with contig lengths.
 * Known costs: a tile (BG_PILEUP_TILE positions of one region) is one workgroup's work however deep the pile over it; a record
 * of many operations is walked again by every tile it spans (an operation itself is clipped to the tile by arithmetic).
 * Not covered: counting overlapping mates once, BAQ, reference bases in the rows (bg_bam_sites below holds the counters against
 * the reference without storing rows; bg_bam_indels names deletions by length and insertions by sequence), the CG tag,
 * unsorted input, per-read pileup iterators. */
typedef struct { int32_t ref, beg, end; } bg_bam_region_t;           /* 0-based, half-open; 12 bytes */
enum { BG_PILEUP_STRANDS = 1 };
enum { BG_PILEUP_A, BG_PILEUP_C, BG_PILEUP_G, BG_PILEUP_T, BG_PILEUP_OTHER, BG_PILEUP_DEL, BG_PILEUP_SKIP, BG_PILEUP_INS,
       BG_PILEUP_COLS /* 8 */ };
typedef struct {
    uint32_t flags;      /* BG_PILEUP_* */
    uint16_t require;    /* FLAG bits a kept record has */
    uint16_t exclude;    /* FLAG bits a kept record lacks */
    uint8_t min_mapq;    /* a kept record has mapq >= this */
    uint8_t min_baseq;   /* a counted base has a raw quality byte >= this */
    uint16_t reserved;   /* 0 */
} bg_bam_pileup_t;
int bg_bam_pileup_dev(bg_ctx* ctx, const bg_bam_pileup_t* prm, uint64_t n_slots, const uint8_t* d_recs, const uint64_t* d_off,
                      const bg_sam_contig_t* d_contigs, uint64_t n_contigs, const bg_bam_region_t* d_regions, uint64_t n_regions,
                      uint32_t* d_rows, uint64_t rows_cap, uint64_t* d_row_off, uint64_t* n_rows, uint64_t* first_bad, void* stream);
int bg_bam_pileup(bg_ctx* ctx, const bg_bam_pileup_t* prm, uint64_t n_slots, const uint8_t* recs, const uint64_t* off,
                  const bg_sam_contig_t* contigs, uint64_t n_contigs, const bg_bam_region_t* regions, uint64_t n_regions,
                  uint32_t* rows, uint64_t rows_cap, uint64_t* row_off, uint64_t* n_rows, uint64_t* first_bad);

/* ---- candidate variant sites and region summaries: the pileup held against the reference (bam_sites.hip; the bodies in
 * csrc/bam_sites_rule.h) ----
 * The counters of bg_bam_pileup compared with the reference text where they are counted: one compact record for every
 * candidate variant site and one summary for every region.  No row goes to HBM, so the regions may be whole genomes.
 * (d_recs, d_off), contigs and regions are those of bg_bam_pileup; (d_text, n_text) is the index text contigs[i].start
 * addresses: what bg_fasta_reference[_dev] leaves, in the layout bg_bam_header_parse gives the contig table.
 * THE RULE.  The result is a function of the inputs alone (integer arithmetic; no float, no order of arrival).
 *   counters   slots, checks, order, kept, the walk and the regions are those of bg_bam_pileup, word for word (the same
 *              bodies).  The counters of a position are the 16 columns of the BG_PILEUP_STRANDS form, always.
 *   reference  the reference byte of position p of contig ref is text[contigs[ref].start + p] with a-z folded to A-Z.  A, C,
 *              G, T name the reference column.  Any other byte (N, IUPAC codes) makes the position unjudged: it yields no
 *              site and counts into n_ref_other; its depth still counts.  A `$` is never read.  A region whose contig does not
 *              lie inside [0, n_text) (start + len > n_text) is a region error: BG_ERR_INVALID_ARG with *first_bad =
 *              UINT64_MAX, judged with the other region checks, before the slots.
 *   depth      depth(p) = A + C + G + T + OTHER + DEL over both strands.
 *   candidates of a judged position, in this order: the three non-reference columns among A, C, G, T, ascending
 *              (BG_SITE_SNV, alt = the ASCII base); DEL (BG_SITE_DEL: one candidate a deleted position, not one a deletion
 *              event); INS (BG_SITE_INS, anchored at p as the pileup anchors it).  alt_fwd / alt_rev are the candidate's
 *              column in the two halves of the row, alt = alt_fwd + alt_rev.  A candidate is a site when depth >= min_depth,
 *              alt >= max(min_alt, 1), (uint64) alt * 1000 >= (uint64) min_alt_permille * depth (equality passes),
 *              alt_fwd >= min_alt_strand and alt_rev >= min_alt_strand.  A position gives 0 to 5 sites.
 *   site       bg_bam_site_t, 32 bytes: ref_base is the folded byte, alt 0 for DEL and INS, ref_count the reference column over
 *              both strands, region the index of the region the site belongs to.
 *   order      sites come in region order, then by position, then in candidate order.  d_site_off[r] (optional, n_regions + 1
 *              entries) is the index of region r's first site.  Regions may overlap, repeat and come in any order; a region's
 *              sites are what it would get in a call of its own.
 *   summary    bg_bam_region_summary_t, 48 bytes, one a region (d_summary is optional), zeros for an empty region: sum_depth;
 *              match = the reference column summed over the judged positions, mismatch = the other three base columns over the
 *              judged positions; covered[k] = the positions with depth >= cover[k] (0 counts every position); max_depth;
 *              n_ref_other.
 *   sizing     a null d_sites with sites_cap == 0 sizes the call: *n_sites, every check still made, nothing written (summaries
 *              and d_site_off included).  sites_cap < n_sites: BG_ERR_OPS_CAP with *n_sites set and nothing written.
 *   limits     BG_ERR_TOO_LARGE: those of bg_bam_pileup (n_rows counts the regions' positions) and n_sites >= 2^32.
 *              BG_ERR_INVALID_ARG also: flags != 0, reserved != 0, min_alt_permille > 1000, a null d_text with n_text > 0, the
 *              null pointers bg_bam_pileup refuses.  Every refusal of bg_bam_pileup is a refusal here, with the same status and
 *              the same *first_bad, and nothing is written.
 * d_sites and d_summary are 4-byte aligned (site records go out 16 bytes wide where d_sites is 16-byte aligned, as dwords
 * otherwise); d_text and d_recs may sit at any address.  The counters are counted twice, once to count the sites of every tile
 * and once to place them, instead of being parked in HBM.  TWO read-backs with one stream synchronisation each (the errors
 * and the tiles; the number of sites); the records are then written asynchronously on `stream`.  A tile's share of its
 * region's summary is parked in scratch and a pass of its own sums a region's tiles (integer sums and maxima: exact, whatever
 * the order).  Scratch is the ctx's: the pileup's and 12 bytes a tile, 48 more a tile where d_summary is given.
 * Not covered: genotype likelihoods, overlapping mates, BAQ, the CG tag (deletion events and inserted sequences:
 * bg_bam_indels below, left-aligned against the reference: bg_bam_indels_left behind it; VCF text: bg_vcf_emit below that). */
enum { BG_SITE_SNV = 0, BG_SITE_DEL = 1, BG_SITE_INS = 2 };
typedef struct {
    uint32_t flags;             /* 0 */
    uint16_t require;           /* FLAG bits a kept record has */
    uint16_t exclude;           /* FLAG bits a kept record lacks */
    uint8_t min_mapq;           /* a kept record has mapq >= this */
    uint8_t min_baseq;          /* a counted base has a raw quality byte >= this */
    uint16_t reserved;          /* 0 */
    uint32_t min_depth;         /* a site's position has depth >= this */
    uint32_t min_alt;           /* a site has alt >= max(this, 1) */
    uint32_t min_alt_permille;  /* ... and alt * 1000 >= this * depth; at most 1000 */
    uint32_t min_alt_strand;    /* ... and alt_fwd, alt_rev >= this */
    uint32_t cover[4];          /* covered[k] counts the positions with depth >= cover[k] */
} bg_bam_sites_t;               /* 44 bytes */
typedef struct {
    int32_t ref, pos;           /* 0-based */
    uint32_t region;
    uint8_t kind, ref_base, alt, reserved;  /* BG_SITE_*; the folded reference byte; the ASCII base of an SNV, else 0; 0 */
    uint32_t depth, ref_count, alt_fwd, alt_rev;
} bg_bam_site_t;                /* 32 bytes */
typedef struct {
    uint64_t sum_depth, match, mismatch;
    uint32_t covered[4];
    uint32_t max_depth, n_ref_other;
} bg_bam_region_summary_t;      /* 48 bytes */
int bg_bam_sites_dev(bg_ctx* ctx, const bg_bam_sites_t* prm, uint64_t n_slots, const uint8_t* d_recs, const uint64_t* d_off,
                     const bg_sam_contig_t* d_contigs, uint64_t n_contigs, const uint8_t* d_text, uint64_t n_text,
                     const bg_bam_region_t* d_regions, uint64_t n_regions, bg_bam_site_t* d_sites, uint64_t sites_cap,
                     uint64_t* d_site_off, bg_bam_region_summary_t* d_summary, uint64_t* n_sites, uint64_t* first_bad,
                     void* stream);
int bg_bam_sites(bg_ctx* ctx, const bg_bam_sites_t* prm, uint64_t n_slots, const uint8_t* recs, const uint64_t* off,
                 const bg_sam_contig_t* contigs, uint64_t n_contigs, const uint8_t* text, uint64_t n_text,
                 const bg_bam_region_t* regions, uint64_t n_regions, bg_bam_site_t* sites, uint64_t sites_cap,
                 uint64_t* site_off, bg_bam_region_summary_t* summary, uint64_t* n_sites, uint64_t* first_bad);

/* ---- indel events: deletions by length and insertions by sequence, per anchor (bam_indels.hip; the bodies in
 * csrc/bam_indels_rule.h) ----
 * What bg_bam_sites cannot name: one record for every distinct indel event of a batch of regions — a deletion of a given
 * length, or an insertion of a given sequence, behind a given anchor — with counts per strand and the depth of the anchor,
 * thresholded as sites are, and the inserted sequences beside the records.  (d_recs, d_off), contigs and regions are those of
 * bg_bam_pileup; no reference text is needed.  A writer of VCF text is a formatting pass over bg_bam_site_t (SNVs) and these.
 * THE RULE.  The result is a function of the inputs alone (integer arithmetic; no float, no order of arrival).
 *   shared     slots, checks, order, kept, regions and every refusal are those of bg_bam_pileup, word for word (the same
 *              bodies), with the same status and the same *first_bad; nothing is written on a refusal.
 *   raw events the walk of a kept record is the pileup's: r = pos, q = 0.  An I of length n >= 1 with r > pos is a raw insertion:
 *              anchor r - 1, length n, sequence the 4-bit codes of bases q .. q + n - 1.  A D of length n >= 1 with r > pos is a
 *              raw deletion: anchor r - 1, length n.  An operation with r == pos has nothing of the record in front of it and is
 *              dropped, as the pileup drops such an insertion.  An operation of length 0 gives no event; N, S, H, P and code 9
 *              give none.  Adjacent operations are not merged (2D 3D is two events) and nothing is shifted (no
 *              left-alignment).  A record with l_seq == 0 gives its deletions and drops its insertions.  min_baseq never
 *              removes an event.  A raw event belongs to every region whose [beg, end) holds its anchor.
 *   events     within a region, raw events with equal (anchor, kind, len and, for insertions, every 4-bit code) are ONE event.
 *              alt_fwd counts its records with FLAG 0x10 clear, alt_rev those with it set, alt = alt_fwd + alt_rev.  depth is
 *              bg_bam_sites' depth of the anchor: A + C + G + T + OTHER + DEL over both strands, under the same min_baseq.
 *   kept       an event is kept under bg_bam_sites' four conditions: depth >= min_depth, alt >= max(min_alt, 1), (uint64) alt *
 *              1000 >= (uint64) min_alt_permille * depth (equality passes), alt_fwd >= min_alt_strand and alt_rev >=
 *              min_alt_strand.
 *   order      events come by region, then anchor, then DEL before INS, then len ascending; insertions of one length then by
 *              their 4-bit codes as unsigned numbers, left to right.  d_event_off[r] (optional, n_regions + 1 entries) is the
 *              index of region r's first event.  Regions may overlap, repeat and come in any order; a region's events are what
 *              it would get in a call of its own.
 *   sequences  the bytes of d_seq are ASCII through "=ACMGRSVTWYHKDBN".  The sequences of the kept insertions lie in event order
 *              without gaps: an insertion's len bytes start at d_seq[seq_off]; a deletion carries the running offset and has no
 *              bytes.  *n_seq is their total.
 *   sizing     a null d_events with events_cap == 0 sizes the call: *n_events and *n_seq, every check still made, nothing
 *              written; d_seq must then be null with seq_cap == 0.  events_cap < n_events or seq_cap < n_seq: BG_ERR_OPS_CAP
 *              with both totals set and nothing written.
 *   limits     BG_ERR_TOO_LARGE: those of bg_bam_pileup, and raw events, events or sequence bytes >= 2^32.
 *              BG_ERR_INVALID_ARG also: flags != 0, reserved != 0, min_alt_permille > 1000, a null n_events or n_seq, a null
 *              d_seq with seq_cap > 0, a sizing call with a d_seq or a seq_cap, the null pointers bg_bam_pileup refuses.
 * d_events and d_event_off are 8-byte aligned; d_seq and d_recs may sit at any address.  THREE read-backs with one stream
 * synchronisation each (the errors and the tiles; the raw events; the events and sequence bytes); the records and sequences
 * are then written asynchronously on `stream`.  A count pass walks the candidates of every tile, an emit pass counts the depth
 * of the tiles that have raw events (8 columns, 16 KB of LDS) and writes them to scratch, a merge sort orders them by the full
 * key (the comparator reads the inserted codes from the records: exact at any length, no hashing), heads of runs and prefix
 * sums of the strand bits give every event's counts without an atomic.  Scratch is the ctx's: the pileup's, 12 bytes a tile and
 * 88 a raw event plus the sort's own.
 * Not covered: left-alignment against the reference (bg_bam_indels_left below does it), merging adjacent operations, genotype
 * likelihoods, overlapping mates, BAQ, the CG tag (VCF text: bg_vcf_emit below). */
typedef struct {
    uint32_t flags;             /* 0 */
    uint16_t require;           /* FLAG bits a kept record has */
    uint16_t exclude;           /* FLAG bits a kept record lacks */
    uint8_t min_mapq;           /* a kept record has mapq >= this */
    uint8_t min_baseq;          /* enters the depth only, never an event */
    uint16_t reserved;          /* 0 */
    uint32_t min_depth;         /* a kept event's anchor has depth >= this */
    uint32_t min_alt;           /* a kept event has alt >= max(this, 1) */
    uint32_t min_alt_permille;  /* ... and alt * 1000 >= this * depth; at most 1000 */
    uint32_t min_alt_strand;    /* ... and alt_fwd, alt_rev >= this */
} bg_bam_indels_t;              /* 28 bytes */
typedef struct {
    int32_t ref, pos;           /* the anchor, 0-based: the reference base in front of the event */
    uint32_t region;
    uint8_t kind, reserved[3];  /* BG_SITE_DEL or BG_SITE_INS; 0 */
    uint32_t len;               /* deleted reference bases / inserted bases, >= 1 */
    uint32_t depth, alt_fwd, alt_rev;
    uint64_t seq_off;           /* INS: its len bytes start at d_seq[seq_off]; DEL: the running offset, no bytes */
} bg_bam_indel_t;               /* 40 bytes */
int bg_bam_indels_dev(bg_ctx* ctx, const bg_bam_indels_t* prm, uint64_t n_slots, const uint8_t* d_recs, const uint64_t* d_off,
                      const bg_sam_contig_t* d_contigs, uint64_t n_contigs, const bg_bam_region_t* d_regions, uint64_t n_regions,
                      bg_bam_indel_t* d_events, uint64_t events_cap, uint8_t* d_seq, uint64_t seq_cap, uint64_t* d_event_off,
                      uint64_t* n_events, uint64_t* n_seq, uint64_t* first_bad, void* stream);
int bg_bam_indels(bg_ctx* ctx, const bg_bam_indels_t* prm, uint64_t n_slots, const uint8_t* recs, const uint64_t* off,
                  const bg_sam_contig_t* contigs, uint64_t n_contigs, const bg_bam_region_t* regions, uint64_t n_regions,
                  bg_bam_indel_t* events, uint64_t events_cap, uint8_t* seq, uint64_t seq_cap, uint64_t* event_off,
                  uint64_t* n_events, uint64_t* n_seq, uint64_t* first_bad);

/* ---- indel events, left-aligned against the reference (bam_indels.hip; the bodies in csrc/bam_indels_left_rule.h) ----
 * bg_bam_indels counts an event exactly as the records spell it, and in a homopolymer or a tandem repeat one indel has as many
 * spellings as the repeat has positions: its records then fall apart into shares that are judged alone.  bg_bam_indels_left
 * shifts every raw event to the left against the reference text BEFORE events are merged, so that the spellings of one indel
 * meet in one event.  The arguments are those of bg_bam_indels[_dev] with (d_text, n_text), the index text bg_bam_sites reads,
 * behind n_contigs; the outputs are those of bg_bam_indels[_dev], and bg_vcf_emit[_dev] takes them unchanged.
 * THE RULE.  The result is a function of the inputs alone (integer arithmetic; no float, no order of arrival).
 *   shared     slots, checks, order, kept records, regions, the raw events of a record and every refusal are those of
 *              bg_bam_indels, word for word (the same bodies): an operation with r == pos or of length 0 is dropped, and so are
 *              the insertions of a record without bases.  The regions' contigs are held against the text as bg_bam_sites holds
 *              them: contig.start + contig.len > n_text is a region error (BG_ERR_INVALID_ARG, *first_bad = UINT64_MAX); a null
 *              d_text with n_text > 0 is BG_ERR_INVALID_ARG, as are flags != 0, reserved != 0 and min_alt_permille > 1000.
 *   text       F(p) = text[contigs[ref].start + p] with a-z folded to A-Z.  A text byte or an inserted byte is a BASE only if
 *              it is A, C, G or T.  Only positions pos < p < contig.len of the record's contig are read: a `$` never is.
 *   deletion   a raw deletion (a, n) deletes a + 1 .. a + n.  One step takes a to a - 1.  A step is allowed while fewer than
 *              max_shift steps have been taken, a > pos (the new anchor stays >= pos: an event never moves in front of the
 *              record that carries it), a + n < contig.len, and F(a) == F(a + n) is a base.
 *   insertion  a raw insertion (a, n, s[0 .. n)): s is the 4-bit codes read as ASCII through "=ACMGRSVTWYHKDBN".  Step j (j =
 *              0, 1, ...) is allowed while j < max_shift, a - j > pos, and c_j == F(a - j) is a base, where c_j = s[n - 1 - j]
 *              for j < n and F(a - j + n) beyond.  With k steps taken the anchor is a' = a - k and byte i of the sequence is
 *              F(a' + 1 + i) for i < min(k, n) and s[i - k] behind (which is s rotated right by k mod n: every step compared
 *              the text byte that enters with the byte that leaves; no rotated copy is ever materialised).
 *   after      everything else is bg_bam_indels' rule applied to the shifted events: an event belongs to every region whose
 *              [beg, end) holds the SHIFTED anchor; shifted events with equal (anchor, kind, len and every byte of the shifted
 *              sequence) are ONE event; counts per strand; depth is bg_bam_sites' depth of the shifted anchor under min_baseq;
 *              the four conditions; the order (region, anchor, DEL before INS, len, then the shifted sequence as 4-bit codes
 *              left to right, a text base taking the code of its letter); seq_off, sizing, BG_ERR_OPS_CAP, limits and
 *              alignment requirements.
 *   therefore  max_shift == 0 gives the bytes of bg_bam_indels[_dev] wherever the text check passes; UINT32_MAX never binds.
 *              Two operations of one record that normalise to one event count twice.  A record that begins inside a repeat
 *              stops at its own pos, so its event may stay apart from the others (GATK's per-read left-alignment behaves the
 *              same way).  alt <= depth may fail only as it can in bg_bam_indels.
 * d_text may sit at any address.  Read-backs, passes and scratch (88 bytes a raw event: k rides in a word that was spare) are
 * those of bg_bam_indels_dev.  The two tile passes walk a candidate record's operations beyond the tile's end, as far as
 * max_shift allows, because an event anchored behind a tile may land in it; a' >= pos is what keeps a tile's candidates (the
 * records that overlap it) complete.  A long record's later operations are therefore shifted again by every tile it spans.
 * Not covered: merging adjacent operations, trimming shared bases, joining alleles, shifting in front of a record's pos. */
typedef struct {
    uint32_t flags;             /* 0 */
    uint16_t require;           /* FLAG bits a kept record has */
    uint16_t exclude;           /* FLAG bits a kept record lacks */
    uint8_t min_mapq;           /* a kept record has mapq >= this */
    uint8_t min_baseq;          /* enters the depth only, never an event */
    uint16_t reserved;          /* 0 */
    uint32_t min_depth;         /* a kept event's shifted anchor has depth >= this */
    uint32_t min_alt;           /* a kept event has alt >= max(this, 1) */
    uint32_t min_alt_permille;  /* ... and alt * 1000 >= this * depth; at most 1000 */
    uint32_t min_alt_strand;    /* ... and alt_fwd, alt_rev >= this */
    uint32_t max_shift;         /* the steps an event may take; 0: none (bg_bam_indels' events), UINT32_MAX: no limit */
} bg_bam_indels_left_t;         /* 32 bytes: bg_bam_indels_t, then max_shift */
int bg_bam_indels_left_dev(bg_ctx* ctx, const bg_bam_indels_left_t* prm, uint64_t n_slots, const uint8_t* d_recs,
                           const uint64_t* d_off, const bg_sam_contig_t* d_contigs, uint64_t n_contigs, const uint8_t* d_text,
                           uint64_t n_text, const bg_bam_region_t* d_regions, uint64_t n_regions, bg_bam_indel_t* d_events,
                           uint64_t events_cap, uint8_t* d_seq, uint64_t seq_cap, uint64_t* d_event_off, uint64_t* n_events,
                           uint64_t* n_seq, uint64_t* first_bad, void* stream);
int bg_bam_indels_left(bg_ctx* ctx, const bg_bam_indels_left_t* prm, uint64_t n_slots, const uint8_t* recs, const uint64_t* off,
                       const bg_sam_contig_t* contigs, uint64_t n_contigs, const uint8_t* text, uint64_t n_text,
                       const bg_bam_region_t* regions, uint64_t n_regions, bg_bam_indel_t* events, uint64_t events_cap,
                       uint8_t* seq, uint64_t seq_cap, uint64_t* event_off, uint64_t* n_events, uint64_t* n_seq,
                       uint64_t* first_bad);

/* ---- VCF text from candidate sites and indel events (vcf_emit.hip; the bodies in csrc/vcf_rule.h) ----
 * One VCF v4.3 data line for every SNV site and every indel event, in one contiguous buffer, formatted from exactly what
 * bg_bam_sites[_dev] and bg_bam_indels[_dev] leave behind: (d_sites, n_sites) the sites, (d_events, n_events) the events,
 * (d_seq, n_seq) the inserted bases, (d_contigs, n_contigs, d_names) and (d_text, n_text) the contig table and the index text
 * those calls take.  Eight columns, no sample columns.
 * THE RULE.  The bytes are a function of the inputs alone (integer arithmetic; no float, no order of arrival).
 *   lines      a site of kind BG_SITE_SNV gives one line; sites of kind BG_SITE_DEL and BG_SITE_INS give none (the events name
 *              them) and are still checked; every event gives one line.  One line per allele: the alleles of a position are
 *              not joined.
 *   order      by region, then pos, then the SNVs of a (region, pos) in front of its events, each kind in the order of its
 *              own list (bg_bam_indels returns an anchor's deletions in front of its insertions, so SNV, DEL, INS).  Both lists
 *              arrive non-decreasing in (region, pos), as the two calls return them, so a line's index is the element's rank in
 *              its own list (the sites compacted to the SNVs) plus one binary search in the other list: no sort and no atomic
 *              places a line.  Regions are not reordered: a sorted file takes ascending regions that do not overlap.
 *   columns    CHROM POS ID REF ALT QUAL FILTER INFO, separated by tabs, ended by '\n'.  CHROM the contig's name bytes, POS =
 *              pos + 1, ID, QUAL and FILTER ".".
 *   R(p)       the reference byte text[contigs[ref].start + p] with a-z folded to A-Z, then: A, C, G, T, N as they are; M, R, W,
 *              D, H, V -> A; Y, S, B -> C; K -> G; anything else -> N (VCF v4.3: an IUPAC code in REF becomes the first base,
 *              alphabetically, that it stands for).
 *   S(b)       an inserted byte of d_seq: A, C, G, T as they are, anything else ('=', N, IUPAC) -> N.
 *   REF, ALT   SNV: REF = R(pos), ALT = alt.  DEL of len: REF = R(pos) .. R(pos + len), ALT = R(pos).  INS of len: REF = R(pos),
 *              ALT = R(pos) followed by S of the len bytes at d_seq[seq_off].
 *   INFO       SNV: DP=<depth>;RO=<ref_count>;AO=<alt_fwd + alt_rev>;SAF=<alt_fwd>;SAR=<alt_rev>;TYPE=snp.  Events: the same
 *              without RO, with TYPE=del or TYPE=ins.  AO is a 64-bit sum.  Numbers are decimal without padding.
 *   checks     the combined list holds the sites at 0 .. n_sites - 1 and event j at n_sites + j.  The smallest index of an
 *              element that fails a check is *first_bad (UINT64_MAX if none); the status is then BG_ERR_INVALID_ARG and nothing
 *              is written.  ref outside [0, n_contigs); a contig that does not lie inside [0, n_text); pos outside [0,
 *              contig.len); a kind the list may not hold (sites: SNV, DEL, INS; events: DEL, INS); a non-zero reserved byte; an
 *              SNV whose ref_base is not the folded text byte, or whose alt is not one of A, C, G, T, or equals ref_base; an
 *              event with len == 0; a DEL with pos + len >= contig.len (a `$` is never read); an INS with seq_off + len >
 *              n_seq; an element whose (region, pos) is smaller than its predecessor's in its list.
 *   sizing     a null d_out with out_cap == 0 sizes the call: *n_lines and *out_bytes, every check still made, nothing written,
 *              d_line_off included.  out_cap < out_bytes: BG_ERR_OPS_CAP with both totals set and nothing written.
 *   offsets    d_line_off (optional, n_lines + 1 entries): where every line starts and the last one ends.
 *   empty      no element at all is BG_OK with 0 lines.  A null array with a count of 0 is accepted; every other null (the
 *              result pointers included) is BG_ERR_INVALID_ARG, as are flags != 0 and reserved != 0.
 *   limits     offsets are 64-bit and a line is measured in 64 bits (a deletion may be longer than any staging buffer).
 *              BG_ERR_TOO_LARGE: 2^32 elements or more, a single line of 2^32 bytes or more (a deletion of 4 Gbp: pos is 32-bit,
 *              and no contig of a BAM header is that long).
 * d_out, d_text, d_seq and d_names may sit at any address; d_sites is 4-byte aligned, d_events and d_line_off 8-byte aligned.
 * ONE read-back with one stream synchronisation (the refused index, the number of lines, the bytes); the sizing call ends
 * there, the text is then written asynchronously on `stream`.  A line of at most 256 bytes is put together in LDS by eight
 * lanes and leaves in 16-byte stores where the destination allows; a longer one is formatted in place.  Scratch is the ctx's:
 * at most 32 bytes an element.  bg_vcf_emit stages host arrays through it (names: up to the last contig's last byte).
 * bg_vcf_header (host only, no GPU) writes "##fileformat=VCFv4.3\n##source=biogpu\n", one "##contig=<ID=name,length=len>\n" a
 * contig, an ##INFO line for each of DP, RO, AO, SAF, SAR and TYPE and the "#CHROM ... INFO" line; *out_bytes receives the
 * length, out == NULL with out_cap == 0 sizes, BG_ERR_OPS_CAP if out_cap is too small (nothing written).
 * Not covered: left-alignment of indels (bg_bam_indels_left hands over events that are left-aligned already; the writer
 * shifts nothing), trimming of shared bases, joining alleles into multi-allelic lines, genotypes and sample
 * columns, QUAL and FILTER values, tabix or CSI indexes, BCF, reading VCF. */
typedef struct {
    uint32_t flags;             /* 0 */
    uint32_t reserved;          /* 0 */
} bg_vcf_params_t;              /* 8 bytes */
int bg_vcf_header(const bg_sam_contig_t* contigs, uint64_t n_contigs, const char* names, char* out, uint64_t out_cap,
                  uint64_t* out_bytes);
int bg_vcf_emit_dev(bg_ctx* ctx, const bg_vcf_params_t* prm, const bg_bam_site_t* d_sites, uint64_t n_sites,
                    const bg_bam_indel_t* d_events, uint64_t n_events, const uint8_t* d_seq, uint64_t n_seq,
                    const bg_sam_contig_t* d_contigs, uint64_t n_contigs, const char* d_names, const uint8_t* d_text,
                    uint64_t n_text, char* d_out, uint64_t out_cap, uint64_t* d_line_off, uint64_t* n_lines, uint64_t* out_bytes,
                    uint64_t* first_bad, void* stream);
int bg_vcf_emit(bg_ctx* ctx, const bg_vcf_params_t* prm, const bg_bam_site_t* sites, uint64_t n_sites,
                const bg_bam_indel_t* events, uint64_t n_events, const uint8_t* seq, uint64_t n_seq,
                const bg_sam_contig_t* contigs, uint64_t n_contigs, const char* names, const uint8_t* text, uint64_t n_text,
                char* out, uint64_t out_cap, uint64_t* line_off, uint64_t* n_lines, uint64_t* out_bytes, uint64_t* first_bad);

/* ---- the reference text from parsed FASTA records (fasta_ingest.hip) --------------------------------------
 * The index text of n_records parsed records (bg_fasta_parse[_dev] above), with the contig table and names bg_sam_emit_batch[_dev] and bg_sam_header
 * take as they are.  Without BG_FASTA_REF_FMD the text is S0 $ S1 $ ... S(k-1) $ and *n_text = sum(len_i + 1).  With it,
 * T = S0 $ S1 ... $ S(k-1) (n_t = sum(len_i) + k - 1 bytes) and the text is T $ R $ with R = dna::revcomp(T), the byte map
 * of bg_revcomp_batch_dev ('$' maps to itself): *n_text = 2 n_t + 2, the text bg_seed_extend_smem_batch requires.
 * BG_FASTA_REF_UPPER folds a-z to A-Z first (soft-masked genomes); every other byte is copied as it is (whether it is in
 * the index's alphabet remains the FM builder's check).  contigs[i] = {start of S_i in the text, len_i, name_off, id_len},
 * the ids back to back in names; a zero-length sequence gives a zero-length contig.
 * text_out == NULL with text_cap == 0 is a sizing call (fills *n_text and *names_bytes).  BG_ERR_OPS_CAP if text_cap or
 * names_cap is too small, BG_ERR_INVALID_ARG for n_records == 0, unknown flag bits, or a record with check != OK (*first_bad
 * = its index, otherwise UINT64_MAX): nothing is written in any of these cases.  The device flavour reads the sizes back
 * with one synchronisation of `stream`; its write pass is asynchronous on `stream`.  The host flavour uses no GPU (ctx may
 * be NULL). */
enum { BG_FASTA_REF_FMD = 1, BG_FASTA_REF_UPPER = 2 };
/* d_fasta_text, d_seq, d_text_out and d_names may be at any address: the index text is stored 16 bytes at a time at a 16-byte
 * aligned d_text_out, byte by byte at any other address. */
int bg_fasta_reference_dev(bg_ctx* ctx, uint64_t n_records, const bg_fasta_record_t* d_recs, const uint8_t* d_fasta_text,
                           const uint8_t* d_seq, uint32_t flags, uint8_t* d_text_out, uint64_t text_cap,
                           bg_sam_contig_t* d_contigs, char* d_names, uint64_t names_cap, uint64_t* n_text,
                           uint64_t* names_bytes, uint64_t* first_bad, void* stream);
int bg_fasta_reference(bg_ctx* ctx, uint64_t n_records, const bg_fasta_record_t* recs, const uint8_t* fasta_text,
                       const uint8_t* seq, uint32_t flags, uint8_t* text_out, uint64_t text_cap, bg_sam_contig_t* contigs,
                       char* names, uint64_t names_cap, uint64_t* n_text, uint64_t* names_bytes, uint64_t* first_bad);

/* ---- approximate pattern matching in batches of texts (myers.hip) and trimming (fastq_trim.hip) ----------------------
 * bio::pattern_matching::myers::Myers<u64> (src/pattern_matching/myers/): Myers' bit-parallel algorithm for patterns of
 * 1 to 64 symbols with DistType = u8; `myers::long` (block-based) follows below.  Out of scope: Myers<u128> and
 * find_all_lazy's incremental interface (LazyMatches: hit_at / path_at on a search in progress).
 *
 * The pattern crosses the boundary as its tabulated `peq` (simple.rs:55-74; closures and hash maps do not cross it):
 * peq[c] has bit i set where pattern symbol i accepts text byte c, ambiguities (builder.rs:84-92) and text wildcards
 * (builder.rs:115-118, all ones) included; bits at or above m are ignored (the reference's wildcard sets them too).
 * m == 0 is BG_ERR_INVALID_ARG ("Pattern is empty", simple.rs:53), m > 64 BG_ERR_TOO_LARGE ("Pattern too long",
 * simple.rs:52).  These and the other argument checks come before the ctx is looked at.
 *
 * Jobs: n_texts texts (text + off[n_texts + 1], the seq / seq_off bg_fastq_parse_dev leaves; every text shorter than 2^32)
 * against 1 <= n_pat <= 1024 patterns (0: BG_ERR_INVALID_ARG, more: BG_ERR_TOO_LARGE); job t * n_pat + p is text t
 * against pattern p.  max_dist is clamped to 255 (myers_impl.rs:194, 224).
 *
 * A hit is a bg_alignment_t filled as update_aln (helpers.rs:83-99) fills an Alignment: score = dist, xstart = 0,
 * xend = xlen = m, ylen = the text's length, yend = end + 1, ystart = yend - aligned columns, mode = BG_MODE_SEMIGLOBAL,
 * n_clips = 0; operations in pattern order as BG_OP_* bytes (x = pattern, y = text: Ins consumes a pattern symbol, Del a
 * text byte), chosen as _traceback_at does (traceback.rs:235-318 with simple.rs:202-297: Subst, then Ins, then Del, then
 * Match) on the two extra columns left of the text (traceback.rs:153-186).  bg_cigar_batch[_dev] and bg_pretty_batch take
 * the records as they are.  No hit: score = BG_MIN_SCORE, xlen = m, ylen, mode, every other byte 0.
 *
 * bg_myers_best_batch[_dev]: per job the hit find_all(text, max_dist).min_by_key(dist) returns — the smallest distance,
 *   the first end among equals (myers_impl.rs:197-207, 214-225) — with the start and path next_alignment gives there
 *   (myers_impl.rs:400-406, 456-479).  max_dist >= 255 makes it find_best_end plus its alignment; an empty text has no hit
 *   (find_best_end panics).  Job j's operations end at ops + (j + 1) * ops_stride and ops_off points at the first;
 *   ops_stride >= 2 * max m always suffices (m vertical or diagonal moves, at most dist <= m horizontal ones).  With a
 *   smaller stride a job whose path does not fit gets status = BG_ERR_OPS_CAP in its record, its exact n_ops, ops_off =
 *   j * ops_stride and no operations, and the call returns BG_ERR_OPS_CAP (the device flavour then reads a flag back: one
 *   synchronisation of `stream`; with ops_stride >= 2 * max m or ops == NULL it is asynchronous, and uploads nothing when
 *   the patterns are those of the ctx's previous Myers call).  ops == NULL skips the operations, not ystart / n_ops.
 * bg_myers_find_all_batch[_dev]: the iteration of find_all (myers_impl.rs:482-494): every end column whose distance is at
 *   most max_dist, in text order.  The first max_hits (1 .. 64, else BG_ERR_INVALID_ARG) of job j fill
 *   aln[j * max_hits ..], unused slots are no-hit records, count[j] is the job's total.  Coordinates and distance only
 *   (n_ops = 0).  flags & BG_MYERS_ENDS_ONLY is find_all_end (myers_impl.rs:185-195, 284-294): no traceback, ystart = yend.
 * Options (bg_set_option): myers_chunk_jobs — jobs per launch (0: by a 256 MB budget for the traceback columns; rounded
 *   up to a multiple of 256); myers_lds_bytes — LDS bytes the peq tables of one pattern group may take (0: 48 KB; at
 *   least 4096).  Tests use both to reach the sub-batch and group loops with small inputs. */
typedef struct { uint64_t peq[256]; uint32_t m; uint32_t _reserved; } bg_myers_pattern_t;
enum { BG_MYERS_ENDS_ONLY = 1 };
enum { BG_MYERS_MAX_PATTERNS = 1024, BG_MYERS_MAX_HITS = 64 };
int bg_myers_best_batch(bg_ctx* ctx, const bg_myers_pattern_t* pats, uint32_t n_pat, uint32_t max_dist, uint64_t n_texts,
                        const uint8_t* text, const uint64_t* off, bg_alignment_t* aln, uint8_t* ops, uint64_t ops_stride);
int bg_myers_best_batch_dev(bg_ctx* ctx, const bg_myers_pattern_t* pats /* host */, uint32_t n_pat, uint32_t max_dist,
                            uint64_t n_texts, const uint8_t* d_text, const uint64_t* d_off, bg_alignment_t* d_aln,
                            uint8_t* d_ops, uint64_t ops_stride, void* stream);
int bg_myers_find_all_batch(bg_ctx* ctx, const bg_myers_pattern_t* pats, uint32_t n_pat, uint32_t max_dist, uint32_t max_hits,
                            uint32_t flags, uint64_t n_texts, const uint8_t* text, const uint64_t* off, bg_alignment_t* aln,
                            uint32_t* count);
int bg_myers_find_all_batch_dev(bg_ctx* ctx, const bg_myers_pattern_t* pats /* host */, uint32_t n_pat, uint32_t max_dist,
                                uint32_t max_hits, uint32_t flags, uint64_t n_texts, const uint8_t* d_text,
                                const uint64_t* d_off, bg_alignment_t* d_aln, uint32_t* d_count, void* stream);

/* ---- patterns of more than 64 symbols: the block-based variant (myers_long.hip) ---------------------------------------
 * bio::pattern_matching::myers::long::Myers<u64> (src/pattern_matching/myers/long.rs): the pattern cut into blocks of 64
 * symbols, a carry of -1, 0 or +1 handed from block to block in every text column (advance_block, long.rs:136-179), with
 * DistType = usize.  The same calls as above with these differences, and nothing else:
 *   Patterns.  Pattern p has m[p] symbols in ceil(m[p] / 64) blocks; block b's table is
 *     peq[(blk_off[p] + b) * 256 + byte], bit i set where pattern symbol 64 * b + i accepts the byte (long.rs:86-115).
 *     blk_off has n_pat + 1 entries, blk_off[0] = 0 and blk_off[p + 1] - blk_off[p] == ceil(m[p] / 64), else
 *     BG_ERR_INVALID_ARG.  Bits at or above a block's chunk length are ignored (the reference's wildcards set them,
 *     long.rs:105-109); Peq::high_mask (long.rs:113) is derived from m.  m == 0 is BG_ERR_INVALID_ARG ("Pattern is empty",
 *     long.rs:83); m > BG_MYERS_LONG_MAX_M is BG_ERR_TOO_LARGE (the reference has no limit).  peq, blk_off and m are host
 *     arrays in both flavours.  Patterns of several block counts may share a call, and m <= 64 is legal: for
 *     max_dist <= 255 such a pattern gives the records and operations of the calls above byte for byte.
 *   Distances are 32-bit and max_dist is clamped to the pattern's m instead of 255 ("distances cannot exceed m",
 *     States::new, long.rs:205-206): a job's ring is m + min(max_dist, m) + 2 columns (myers_impl.rs:327).
 *   Paths are those of _traceback_at with LongTracebackHandler (long.rs:402-563), block boundaries and the one-symbol last
 *     block (long.rs:430-434) included.  The reference computes, per column, only the blocks of its Ukkonen band
 *     (long.rs:239-268) and reports a column when all were computed (known_dist, long.rs:272-274); the kernels compute every
 *     block, which gives the same ends, distances and paths (myers_long.hip says why; the tests compare).
 *   Traceback scratch per job: (16 * NB + 4) * (m + min(max_dist, m) + 2) bytes, NB the block count of the kernel
 *     instantiation (1, 2, 3, 4, 8, 16) that holds the pattern — 533 000 bytes at m = 1024, about 500 jobs per launch under
 *     the 256 MB budget of myers_chunk_jobs = 0.
 * Job numbering, records, the no-hit record, the operation slots with BG_ERR_OPS_CAP (2 * max m always suffices), max_hits,
 * BG_MYERS_ENDS_ONLY, 1 .. 1024 patterns, the empty text, the order of the argument checks, both options and the _dev
 * flavour's asynchrony are those of bg_myers_*_batch[_dev].  bg_fastq_trim[_dev] takes the best records as they are. */
enum { BG_MYERS_LONG_MAX_M = 1024 };
int bg_myers_long_best_batch(bg_ctx* ctx, const uint64_t* peq, const uint64_t* blk_off, const uint32_t* m, uint32_t n_pat,
                             uint32_t max_dist, uint64_t n_texts, const uint8_t* text, const uint64_t* off, bg_alignment_t* aln,
                             uint8_t* ops, uint64_t ops_stride);
int bg_myers_long_best_batch_dev(bg_ctx* ctx, const uint64_t* peq /* host */, const uint64_t* blk_off /* host */,
                                 const uint32_t* m /* host */, uint32_t n_pat, uint32_t max_dist, uint64_t n_texts,
                                 const uint8_t* d_text, const uint64_t* d_off, bg_alignment_t* d_aln, uint8_t* d_ops,
                                 uint64_t ops_stride, void* stream);
int bg_myers_long_find_all_batch(bg_ctx* ctx, const uint64_t* peq, const uint64_t* blk_off, const uint32_t* m, uint32_t n_pat,
                                 uint32_t max_dist, uint32_t max_hits, uint32_t flags, uint64_t n_texts, const uint8_t* text,
                                 const uint64_t* off, bg_alignment_t* aln, uint32_t* count);
int bg_myers_long_find_all_batch_dev(bg_ctx* ctx, const uint64_t* peq /* host */, const uint64_t* blk_off /* host */,
                                     const uint32_t* m /* host */, uint32_t n_pat, uint32_t max_dist, uint32_t max_hits,
                                     uint32_t flags, uint64_t n_texts, const uint8_t* d_text, const uint64_t* d_off,
                                     bg_alignment_t* d_aln, uint32_t* d_count, void* stream);

/* Trimming parsed FASTQ records by the hits of bg_myers_best_batch[_dev] or bg_myers_long_best_batch[_dev] (rust-bio has no trimmer: the rule is defined
 * here).  hits holds n * n_pat records, read r's at r * n_pat; a pattern has a hit where score != BG_MIN_SCORE.
 *   BG_TRIM_3P keeps [0, e) of the sequence, e the smallest ystart over the read's patterns with a hit, seq_len if none;
 *   BG_TRIM_5P keeps [b, seq_len), b the largest yend over the patterns with a hit, 0 if none
 * (both clamped to seq_len); the same byte range clamped to qual_len is kept of the qualities.  Output records are copies
 * with seq_off, qual_off, seq_len, qual_len rewritten (ids, descriptions and `check` unchanged); sequences, qualities and
 * their n + 1 offsets are compacted (seq_off_out[0] = 0), i.e. what the seed-and-extend *_dev calls and
 * bg_sam_emit_batch_dev take.  A read trimmed to nothing stays as an empty record.  seq_out / qual_out need the capacity
 * of the inputs and no output may alias an input (lanes read the source while others write: the call does not work in place).  Lengths, the exclusive scan of scan.hip, the copy; totals (optional, host, 2 entries: sequence and
 * quality bytes kept) costs the device flavour its only synchronisation of `stream`.  Unknown mode: BG_ERR_INVALID_ARG. */
enum { BG_TRIM_3P = 0, BG_TRIM_5P = 1 };
/* (the byte columns d_seq, d_qual, d_seq_out, d_qual_out may be at any address: read and written byte by byte) */
int bg_fastq_trim_dev(bg_ctx* ctx, uint64_t n, int mode, const bg_alignment_t* d_hits, uint32_t n_pat,
                      const bg_fastq_record_t* d_recs, const uint8_t* d_seq, const uint64_t* d_seq_off, const uint8_t* d_qual,
                      const uint64_t* d_qual_off, bg_fastq_record_t* d_recs_out, uint8_t* d_seq_out, uint64_t* d_seq_off_out,
                      uint8_t* d_qual_out, uint64_t* d_qual_off_out, uint64_t* totals, void* stream);
int bg_fastq_trim(bg_ctx* ctx, uint64_t n, int mode, const bg_alignment_t* hits, uint32_t n_pat, const bg_fastq_record_t* recs,
                  const uint8_t* seq, const uint64_t* seq_off, const uint8_t* qual, const uint64_t* qual_off,
                  bg_fastq_record_t* recs_out, uint8_t* seq_out, uint64_t* seq_off_out, uint8_t* qual_out,
                  uint64_t* qual_off_out, uint64_t* totals);

/* ---- FASTQ out (fastq_emit.hip): select parsed or trimmed records, write FASTQ text -----------------------------------
 * bg_fastq_filter[_dev] drops records and compacts what stays (rust-bio has no filter: the rule is defined here).  The inputs
 * are the columns bg_fastq_parse[_dev] or bg_fastq_trim[_dev] leave: n records, their sequences and qualities with n + 1
 * offsets each; a record's sequence length is seq_off[r + 1] - seq_off[r], as the trim takes it.
 *   A record PASSES if every criterion that is switched on holds:
 *     min_len <= sequence length <= max_len (0 and 0xFFFFFFFF: no bound);
 *     at most max_n bytes 'N' or 'n' in the sequence (0xFFFFFFFF: not counted, the sequence is not read);
 *     BG_FQF_CHECK_OK: recs[r].check == BG_FQCHECK_OK;
 *     BG_FQF_DISCARD_UNTRIMMED: the record is trimmed; BG_FQF_DISCARD_TRIMMED: it is not.  A record is "trimmed" if some
 *       pattern of it has a hit, hits[r * n_pat + p].score != BG_MIN_SCORE: the records of the best call the trim was given
 *       (hits and n_pat are not looked at without one of the two flags; hits may then be null and n_pat 0).
 *   A record is KEPT if it passes; with BG_FQF_PAIRED records 2p and 2p + 1 are mates and are kept or dropped together:
 *     the pair is kept if both pass, with BG_FQF_PAIR_BOTH unless both fail.
 * The kept records come out in input order, compacted: copies with seq_off and qual_off rewritten (ids, descriptions,
 * lengths and `check` unchanged; id_off and desc_off keep pointing into the FASTQ text), sequences and qualities with
 * n_kept + 1 offsets each (the first 0; capacity n + 1).  keep (optional) receives n bytes 0 or 1.  totals (optional, host, 3
 * entries: records kept, sequence bytes, quality bytes) costs the device flavour its only synchronisation of `stream`.
 * Capacities are those of the inputs; no output may alias an input.  A filter with nothing switched on copies its input.
 * BG_ERR_INVALID_ARG: unknown flag bits, both DISCARD flags, a DISCARD flag with null hits or n_pat == 0, BG_FQF_PAIR_BOTH
 * without BG_FQF_PAIRED, BG_FQF_PAIRED with odd n, min_len > max_len, null pointers as bg_fastq_trim refuses them;
 * BG_ERR_TOO_LARGE: n_pat > BG_MYERS_MAX_PATTERNS.  All of them before any device call. */
enum { BG_FQF_PAIRED = 1, BG_FQF_PAIR_BOTH = 2, BG_FQF_DISCARD_UNTRIMMED = 4, BG_FQF_DISCARD_TRIMMED = 8, BG_FQF_CHECK_OK = 16 };
typedef struct {
    uint32_t flags;     /* BG_FQF_* */
    uint32_t min_len;   /* pass: sequence length >= min_len (0: every length) */
    uint32_t max_len;   /* pass: sequence length <= max_len (0xFFFFFFFF: no bound) */
    uint32_t max_n;     /* pass: at most max_n bytes 'N' or 'n' in the sequence; 0xFFFFFFFF: not counted, the sequence is not read */
} bg_fastq_filter_t;
/* (the byte columns d_seq, d_qual, d_seq_out, d_qual_out, d_keep may be at any address: read and written byte by byte) */
int bg_fastq_filter_dev(bg_ctx* ctx, uint64_t n, const bg_fastq_filter_t* flt, const bg_alignment_t* d_hits, uint32_t n_pat,
                        const bg_fastq_record_t* d_recs, const uint8_t* d_seq, const uint64_t* d_seq_off, const uint8_t* d_qual,
                        const uint64_t* d_qual_off, bg_fastq_record_t* d_recs_out, uint8_t* d_seq_out, uint64_t* d_seq_off_out,
                        uint8_t* d_qual_out, uint64_t* d_qual_off_out, uint8_t* d_keep, uint64_t* totals, void* stream);
int bg_fastq_filter(bg_ctx* ctx, uint64_t n, const bg_fastq_filter_t* flt, const bg_alignment_t* hits, uint32_t n_pat,
                    const bg_fastq_record_t* recs, const uint8_t* seq, const uint64_t* seq_off, const uint8_t* qual,
                    const uint64_t* qual_off, bg_fastq_record_t* recs_out, uint8_t* seq_out, uint64_t* seq_off_out,
                    uint8_t* qual_out, uint64_t* qual_off_out, uint8_t* keep, uint64_t* totals);
/* bio::io::fastq::Writer::write(id, desc, seq, qual) (io/fastq.rs:573-593; also Display for Record, 473-485) for records
 * first, first + step, ... below n: m lines and m + 1 offsets.  step 1 writes every record; (0, 2) and (1, 2) split
 * interleaved mates into an R1 and an R2 text.  A line is
 *     '@' id [' ' desc] '\n' seq '\n' '+' '\n' qual '\n'
 * with the space and the description where has_desc != 0 (has_desc with desc_len == 0 gives "@id \n"); id and description are
 * id_len / desc_len bytes of the FASTQ text at id_off / desc_off, sequence and qualities seq_len / qual_len bytes at
 * seq + seq_off / qual + qual_off: the record's own fields, as bg_sam_emit_batch_dev takes them (a line is shorter than 2^32
 * bytes).  Like the reference's writer the call checks nothing: a record with unequal lengths or an empty sequence is written
 * as it is.  The reference's READER rejects the latter — the empty quality line of "@id\n\n+\n\n" raises IncompleteRecord
 * (fastq.rs:298-300) — so records that bg_fastq_trim left empty go through bg_fastq_filter with min_len >= 1 first.
 * Output conventions of bg_sam_emit_batch_dev: one contiguous buffer, lines in order; all lengths and offsets are computed
 * first and the total is read back with one synchronisation of `stream` into *out_bytes; out == NULL with out_cap == 0 is a
 * sizing call that fills out_off; a total above out_cap returns BG_ERR_OPS_CAP before one byte is written.
 * BG_ERR_INVALID_ARG: step == 0, a null out_off or out_bytes, a null out with out_cap != 0, or (m > 0) a null text, recs,
 * seq or qual.  The host flavour takes the extents of the text, seq and qual from the records it writes. */
int bg_fastq_emit_dev(bg_ctx* ctx, uint64_t n, uint64_t first, uint64_t step, const uint8_t* d_fastq_text,
                      const bg_fastq_record_t* d_recs, const uint8_t* d_seq, const uint8_t* d_qual, char* d_out, uint64_t out_cap,
                      uint64_t* d_out_off, uint64_t* out_bytes, void* stream);
int bg_fastq_emit(bg_ctx* ctx, uint64_t n, uint64_t first, uint64_t step, const uint8_t* fastq_text, const bg_fastq_record_t* recs,
                  const uint8_t* seq, const uint8_t* qual, char* out, uint64_t out_cap, uint64_t* out_off, uint64_t* out_bytes);

/* ---- demultiplexing by barcode (fastq_demux.hip): a sample per read, the records grouped by sample -------------------
 * rust-bio has no demultiplexer, as it has no trimmer and no filter: both rules are defined here.
 *
 * bg_fastq_demux_assign[_dev] turns the n * n_pat records of bg_myers_best_batch[_dev] or bg_myers_long_best_batch[_dev]
 * (read r's at r * n_pat) into one sample per read.  pat_bin (host, n_pat entries) names the sample of every pattern:
 * pat_bin[p] < n_bins, several patterns may share one; BG_DMX_IGNORE skips a pattern, so that adapters and barcodes can go
 * through one Myers call.
 *   1. A hit COUNTS if score != BG_MIN_SCORE, its pattern is not ignored, with BG_DMX_ANCHOR_5P ystart <= max_offset, with
 *      BG_DMX_ANCHOR_3P ylen - yend <= max_offset.  With neither anchor flag a hit anywhere counts and max_offset is not
 *      looked at.
 *   2. The WINNER is the counting hit with the smallest (score, p); `best` is its score, b the bin of its pattern.
 *   3. `second` is the smallest score among the counting hits whose bin is not b, infinite if there is none.
 *   4. bin[r] = n_bins (UNASSIGNED) if no hit counts; n_bins + 1 (AMBIGUOUS) if second - best < min_margin; b otherwise.
 *      With min_margin = 0 nothing is ambiguous and a tie between bins goes to the lower pattern index.
 *   5. hit_out[r] is the winning record, copied verbatim, where the read is assigned (bin[r] < n_bins); otherwise a no-hit
 *      record: score = BG_MIN_SCORE, ylen and mode of hits[r * n_pat], every other byte 0.  bg_fastq_trim[_dev] with
 *      n_pat = 1 on hit_out cuts exactly the read's own barcode, and nothing off a read that has none.
 *   6. pat_out[r] (optional) is the p of the record in hit_out[r], BG_DMX_IGNORE where that is a no-hit record.
 *   7. With BG_DMX_PAIRED (n even) records 2q and 2q + 1 are mates.  BG_DMX_MATE1 and / or BG_DMX_MATE2 say whose hits count
 *      (neither flag: both).  The pair's candidates are the counting hits of those mates, mate 1 before mate 2 among equal
 *      (score, p); rules 2 to 4 over them give ONE bin, which both mates get.  hit_out and pat_out carry the winner on the
 *      mate that holds it and a no-hit record on the other.
 * Refused before any device call — BG_ERR_INVALID_ARG: null params, unknown flag bits, both anchor flags, a MATE flag
 * without BG_DMX_PAIRED, BG_DMX_PAIRED with odd n, n_bins == 0, n_pat == 0, a null pat_bin, a pat_bin entry that is neither
 * below n_bins nor BG_DMX_IGNORE, (n > 0) a null hits, bin or hit_out; BG_ERR_TOO_LARGE: n_bins > BG_DMX_MAX_BINS,
 * n_pat > BG_MYERS_MAX_PATTERNS.  hit_out must not alias hits.  The device flavour is asynchronous on `stream` (pat_bin is
 * consumed before it returns); the call is deterministic.
 *
 * bg_fastq_demux_split[_dev] is a stable partition of the columns of a parse, a trim or a filter by bin.  There are
 * n_bins + 2 groups: the samples, then unassigned, then ambiguous; a bin value above n_bins + 1 counts as unassigned.
 * The output columns are the input columns reordered so that group 0's records come first, each group in input order:
 * records are copies with seq_off / qual_off rewritten, sequences and qualities are compacted with n + 1 offsets each
 * (capacities of the inputs).  bin_off (n_bins + 3 entries): group g's records are bin_off[g] .. bin_off[g + 1], and
 * bin_off[n_bins + 2] = n.  perm (optional, n entries): perm[k] is the input index of output record k.  With hit (n
 * records, e.g. assign's hit_out) hit_out[k] = hit[perm[k]], so trimming works before or after the split.  bin_off_host
 * (optional, host, n_bins + 3 entries) costs the device flavour its only synchronisation of `stream`.  n == 0 writes zero
 * offsets and returns.  No output may alias an input.
 *   Pairs: mates that share a bin, as assign leaves them, stay adjacent because the partition is stable, so there is no
 *   pair flag, and every bin_off of interleaved mates is even.
 *   Per-sample texts: ONE bg_fastq_emit_dev over the split columns writes every sample's FASTQ into one buffer; sample g's
 *   text is out[out_off[bin_off[g]] .. out_off[bin_off[g + 1]]).  With (first, step) = (0, 2) and (1, 2) that gives the R1
 *   and the R2 texts, out_off indexed by bin_off[g] / 2.  Records trimmed to nothing are written as they are (see
 *   bg_fastq_emit above).
 * Refused before any device call — BG_ERR_INVALID_ARG: n_bins == 0, a null bin_off or output offsets, hit_out without hit,
 * (n > 0) a null bin or column; BG_ERR_TOO_LARGE: n_bins > BG_DMX_MAX_BINS.
 * Out of scope: combinatorial dual-index tables (an i7 x i5 pair of pattern sets mapped to a sample), correcting barcodes
 * against a whitelist beyond what the Myers call's max_dist gives, and writing files. */
enum { BG_DMX_ANCHOR_5P = 1, BG_DMX_ANCHOR_3P = 2, BG_DMX_PAIRED = 4, BG_DMX_MATE1 = 8, BG_DMX_MATE2 = 16 };
enum { BG_DMX_MAX_BINS = 1024 };
#define BG_DMX_IGNORE 0xFFFFFFFFu /* a pat_bin entry: the pattern names no sample; a pat_out entry: no winner */
typedef struct {
    uint32_t flags;       /* BG_DMX_* */
    uint32_t n_bins;      /* samples: 1 .. BG_DMX_MAX_BINS */
    uint32_t min_margin;  /* ambiguous: second - best < min_margin */
    uint32_t max_offset;  /* with an anchor flag: how far from its end of the read a counting hit may lie */
} bg_demux_params_t;
int bg_fastq_demux_assign_dev(bg_ctx* ctx, uint64_t n, const bg_demux_params_t* params, const bg_alignment_t* d_hits, uint32_t n_pat,
                              const uint32_t* pat_bin /* host, n_pat */, uint32_t* d_bin, bg_alignment_t* d_hit_out,
                              uint32_t* d_pat_out /* optional */, void* stream);
int bg_fastq_demux_assign(bg_ctx* ctx, uint64_t n, const bg_demux_params_t* params, const bg_alignment_t* hits, uint32_t n_pat,
                          const uint32_t* pat_bin, uint32_t* bin, bg_alignment_t* hit_out, uint32_t* pat_out /* optional */);
/* (the byte columns d_seq, d_qual, d_seq_out, d_qual_out may be at any address: read and written byte by byte) */
int bg_fastq_demux_split_dev(bg_ctx* ctx, uint64_t n, uint32_t n_bins, const uint32_t* d_bin, const bg_alignment_t* d_hit /* optional, n */,
                             const bg_fastq_record_t* d_recs, const uint8_t* d_seq, const uint64_t* d_seq_off, const uint8_t* d_qual,
                             const uint64_t* d_qual_off, bg_fastq_record_t* d_recs_out, uint8_t* d_seq_out, uint64_t* d_seq_off_out,
                             uint8_t* d_qual_out, uint64_t* d_qual_off_out, bg_alignment_t* d_hit_out /* optional */,
                             uint64_t* d_perm /* optional, n */, uint64_t* d_bin_off /* n_bins + 3 */, uint64_t* bin_off_host /* optional */,
                             void* stream);
int bg_fastq_demux_split(bg_ctx* ctx, uint64_t n, uint32_t n_bins, const uint32_t* bin, const bg_alignment_t* hit /* optional, n */,
                         const bg_fastq_record_t* recs, const uint8_t* seq, const uint64_t* seq_off, const uint8_t* qual,
                         const uint64_t* qual_off, bg_fastq_record_t* recs_out, uint8_t* seq_out, uint64_t* seq_off_out, uint8_t* qual_out,
                         uint64_t* qual_off_out, bg_alignment_t* hit_out /* optional */, uint64_t* perm /* optional, n */,
                         uint64_t* bin_off /* n_bins + 3 */);

/* ---- qualities (fastq_qual.hip): cut points, a pass / fail bin and per-cycle tables from the quality column ----------
 * rust-bio has none of this, as it has no trimmer, filter or demultiplexer: the three rules are defined here.  All
 * arithmetic is integer, so every result is bit-exact and the same on every run.
 *
 * Common.  The quality of byte c is q = max(0, c - phred_offset), phred_offset 0 .. 255.  Read r's qualities are
 * qual[qual_off[r] .. qual_off[r + 1]), L of them.  The calls take the columns a parse, a trim, a filter or a split leaves
 * and change none of them; each has a device flavour (device pointers, asynchronous on `stream` unless a host total is
 * asked for) and a host-buffer flavour that stages through it.  Every refusal comes before any device call and says why
 * (bg_last_error).
 *
 * bg_fastq_qual_cut[_dev]: where to cut each read.  Both ends are computed on the whole read, independently.
 *   BG_QCUT_RUNSUM at the 3' end (the BWA / cutadapt rule): s = 0, best = 0, e = L; for i = L - 1 down to 0:
 *     s += cutoff_3p - q[i]; stop if s < 0; if s > best: best = s, e = i.
 *   BG_QCUT_RUNSUM at the 5' end: s = 0, best = 0, b = 0; for i = 0 to L - 1:
 *     s += cutoff_5p - q[i]; stop if s < 0; if s > best: best = s, b = i + 1.
 *     (s is a signed 64-bit number.)
 *   BG_QCUT_WINDOW at the 3' end (Trimmomatic's SLIDINGWINDOW): W = min(window, L); the smallest i in 0 .. L - W with
 *     q[i] + ... + q[i + W - 1] < cutoff_3p * W; if there is none e = L; otherwise e = i, then while e > 0 and
 *     q[e - 1] < cutoff_3p: e -= 1.  (A low last symbol inside a passing window stays.)
 *   BG_QCUT_NONE: b = 0, e = L.
 *   If e < b then e = b.
 *   cut_out[r], one bg_alignment_t per read: where L == 0 or nothing is cut (b == 0 and e == L) a no-hit record —
 *     score = BG_MIN_SCORE, ylen = L, every other byte 0; otherwise score = L - (e - b), the symbols removed, ystart = e,
 *     yend = b, ylen = L, every other byte 0.  NOTE ystart >= yend here, unlike a Myers hit: the record is made for the trim.
 *   Composition: bg_fastq_trim[_dev](BG_TRIM_3P, cut_out, n_pat = 1) keeps [0, e); bg_fastq_trim[_dev](BG_TRIM_5P, ...) of its
 *     output with the same records (gathered again if a filter or a split came in between) then keeps [b, e).  The trim's
 *     own clamping handles records whose sequence and quality lengths differ.  BG_FQF_DISCARD_TRIMMED / _UNTRIMMED of the
 *     filter read the same records.
 *   totals (optional, host, 2 entries: reads cut, quality symbols removed) costs the device flavour its only
 *     synchronisation of `stream`.
 *   BG_ERR_INVALID_ARG: null params, an unknown method, BG_QCUT_WINDOW as method_5p, window == 0 with BG_QCUT_WINDOW,
 *     phred_offset > 255, a null qual_off, (n > 0) a null qual or cut_out.  Both methods BG_QCUT_NONE is legal and writes
 *     no-hit records.
 *
 * bg_fastq_qual_select[_dev]: statistics of each read and a pass / fail bin.
 *   stats_out[r] (optional): sum_q = the sum of q; len = L; n_low = symbols with q < low_q; min_q = the smallest q, 0 for
 *     L == 0; weight_sum = the sum of weight[c] over the read's RAW bytes c, 0 without a table.  weight (optional, host,
 *     256 entries) is consumed before the call returns.
 *   A read PASSES if every criterion holds:
 *     sum_q >= (uint64) min_mean_q * L;
 *     (uint64) n_low * 100 <= (uint64) max_low_pct * L — a max_low_pct of 100 or more always holds;
 *     with a table, weight_sum <= max_weight.
 *     An empty read passes all three: length is the filter's business.
 *   bin_out[r] (optional) is 0 for pass and 1 for fail: bg_fastq_demux_split[_dev] with n_bins = 1 puts the passed records
 *     in group 0 and the failed ones in the "unassigned" group, and one bg_fastq_emit_dev writes both texts.
 *   BG_QSEL_PAIRED / BG_QSEL_PAIR_BOTH have the filter's meaning: records 2p and 2p + 1 are mates and get one verdict — pass
 *     if both pass, with BG_QSEL_PAIR_BOTH unless both fail — so mates stay adjacent through the split.  stats_out is each
 *     mate's own.
 *   Expected errors: a table weight[c] = round(10^(-q(c) / 10) * 2^20) and max_weight = max_ee * 2^20 make the third
 *     criterion "at most max_ee expected errors"; floating point stays outside this interface.
 *   totals (optional, host, 1 entry: records whose bin is 0) costs the device flavour its only synchronisation.
 *   BG_ERR_INVALID_ARG: null params, unknown flag bits, BG_QSEL_PAIR_BOTH without BG_QSEL_PAIRED, BG_QSEL_PAIRED with odd
 *     n, phred_offset > 255, a non-zero _reserved, a null qual_off, (n > 0) a null qual or both outputs null.
 *
 * bg_fastq_qc_tables[_dev]: per-cycle tables of records first, first + step, ... below n (as bg_fastq_emit selects them:
 *   (0, 2) and (1, 2) give the R1 and the R2 tables of interleaved mates).  max_cycles is 1 .. BG_QC_MAX_CYCLES;
 *   R = max_cycles + 1 rows, row max_cycles collects every position at or beyond max_cycles.  `tables` is ONE buffer of
 *   bg_qc_tables_words(max_cycles) 64-bit words, zeroed by the call, holding in this order
 *     base[R][5]        counts of A/a, C/c, G/g, T/t and anything else, by position in the SEQUENCE;
 *     qhist[R][64]      counts of min(q, 63), by position in the QUALITY string;
 *     len_hist[R + 1]   sequence lengths 0 .. max_cycles, longer ones in the last entry;
 *     meanq_hist[64]    min(63, sum_q / L) (integer division) of the reads with L > 0;
 *     n_reads[1].
 *   so bg_qc_tables_words = 5 R + 64 R + (R + 1) + 64 + 1.  Sums of integers commute: the tables are the same on every run.
 *   BG_ERR_INVALID_ARG: step == 0, max_cycles outside its range, phred_offset > 255, a null tables or offsets, with
 *     records selected a null seq or qual.
 *
 * Out of scope: poly-G / poly-X tail trimming, trimming ends by 'N', window cutting from the 5' end, per-tile or
 * per-sample tables in one call (call it once per group of a split), floating-point error probabilities in this interface. */
enum { BG_QCUT_NONE = 0, BG_QCUT_RUNSUM = 1, BG_QCUT_WINDOW = 2 };
enum { BG_QSEL_PAIRED = 1, BG_QSEL_PAIR_BOTH = 2 };
enum { BG_QC_MAX_CYCLES = 1024 };
typedef struct {
    uint32_t phred_offset;  /* 0 .. 255 */
    uint32_t method_5p;     /* BG_QCUT_NONE or BG_QCUT_RUNSUM */
    uint32_t method_3p;     /* BG_QCUT_NONE, BG_QCUT_RUNSUM or BG_QCUT_WINDOW */
    uint32_t cutoff_5p;
    uint32_t cutoff_3p;
    uint32_t window;        /* BG_QCUT_WINDOW: symbols per window, at least 1 */
} bg_qual_cut_t;
typedef struct {
    uint64_t sum_q, weight_sum;
    uint32_t len, n_low, min_q, _reserved;
} bg_qual_stats_t;
typedef struct {
    uint32_t flags;         /* BG_QSEL_* */
    uint32_t phred_offset;  /* 0 .. 255 */
    uint32_t min_mean_q;    /* pass: sum_q >= min_mean_q * L */
    uint32_t low_q;         /* a symbol is low if q < low_q */
    uint32_t max_low_pct;   /* pass: n_low * 100 <= max_low_pct * L; 100 or more: always */
    uint32_t _reserved;     /* 0 */
    uint64_t max_weight;    /* with a table: pass: weight_sum <= max_weight */
} bg_qual_select_t;
uint64_t bg_qc_tables_words(uint32_t max_cycles);
/* (d_qual may be at any address: read byte by byte) */
int bg_fastq_qual_cut_dev(bg_ctx* ctx, uint64_t n, const bg_qual_cut_t* params, const uint8_t* d_qual, const uint64_t* d_qual_off,
                          bg_alignment_t* d_cut_out, uint64_t* totals /* optional, host, 2 */, void* stream);
int bg_fastq_qual_cut(bg_ctx* ctx, uint64_t n, const bg_qual_cut_t* params, const uint8_t* qual, const uint64_t* qual_off,
                      bg_alignment_t* cut_out, uint64_t* totals /* optional, 2 */);
int bg_fastq_qual_select_dev(bg_ctx* ctx, uint64_t n, const bg_qual_select_t* params, const uint32_t* weight /* optional, host, 256 */,
                             const uint8_t* d_qual, const uint64_t* d_qual_off, bg_qual_stats_t* d_stats_out /* optional */,
                             uint32_t* d_bin_out /* optional */, uint64_t* totals /* optional, host, 1 */, void* stream);
int bg_fastq_qual_select(bg_ctx* ctx, uint64_t n, const bg_qual_select_t* params, const uint32_t* weight /* optional, 256 */,
                         const uint8_t* qual, const uint64_t* qual_off, bg_qual_stats_t* stats_out /* optional */,
                         uint32_t* bin_out /* optional */, uint64_t* totals /* optional, 1 */);
int bg_fastq_qc_tables_dev(bg_ctx* ctx, uint64_t n, uint64_t first, uint64_t step, uint32_t phred_offset, uint32_t max_cycles,
                           const uint8_t* d_seq, const uint64_t* d_seq_off, const uint8_t* d_qual, const uint64_t* d_qual_off,
                           uint64_t* d_tables, void* stream);
int bg_fastq_qc_tables(bg_ctx* ctx, uint64_t n, uint64_t first, uint64_t step, uint32_t phred_offset, uint32_t max_cycles,
                       const uint8_t* seq, const uint64_t* seq_off, const uint8_t* qual, const uint64_t* qual_off, uint64_t* tables);

/* ------------------------------------------------------------------ several GPUs (comm.hip)
 * north_star: "query batches shard embarrassingly across the 8 GPUs of one node with a single RCCL all-gather over xGMI
 * only to collect per-query scores/intervals".  One process and one bg_ctx per GPU.  rust-bio has no counterpart (a
 * single-process library); the shim's align_batch_sharded / backward_search_sharded (rust/bio-gpu-shim) are built on these.
 *   bg_shard_range     rank's contiguous slice [rank * N / W, (rank + 1) * N / W) of N units
 *   bg_shard_balanced  world + 1 boundaries of contiguous slices of (nearly) equal total cost (sum of DP cells of mixed-
 *                      length pairs, of pattern lengths): boundary r = first unit where the running cost passes r/W of it
 *   bg_comm_unique_id  (one rank) the 128-byte id every rank hands to bg_comm_init — distribute it however the job
 *                      talks (a file, an environment variable, MPI)
 *   bg_comm_init       RCCL communicator of this rank's ctx (ncclCommInitRank; librccl.so is opened at run time:
 *                      BG_ERR_UNSUPPORTED if it is not there)
 *   bg_comm_init_host  host-staged communicator for the ranks of ONE node, named `name` (POSIX shared memory): moves the
 *                      records through host memory.  For what RCCL cannot do — several ranks on one GPU (tests) — and,
 *                      with ctx == NULL, for plain host pointers (no GPU at all)
 *   bg_gather_records  every rank contributes n_local records of rec_bytes bytes (device pointers; host pointers for
 *                      a ctx-less host communicator) and receives all of them in rank order in `all` (capacity: the sum
 *                      of the counts); counts_out (optional, host, world entries) says how many each rank brought.  RCCL:
 *                      one ncclAllGather on `stream` when the shards are equal, grouped broadcasts when they are ragged;
 *                      the call returns when the collective is queued (the counts cost one stream synchronisation).
 *   bg_gather_records_cap  the same with the size of `all` stated in records: the counts (and every rank's all_cap) travel
 *                      first, and when the ranks' records together exceed the smallest all_cap EVERY rank returns
 *                      BG_ERR_OPS_CAP before a single record has moved.
 * The host-staged flavour never leaves a rank behind: a local failure (segment, mapping, copy) is published in the control
 * block and all ranks return it together after the call's last barrier; a barrier that is not completed within 120 s (a
 * rank is gone) returns BG_ERR_HIP with the data segment unmapped and unlinked.  bg_comm_init_host survives a control
 * segment of the same name left behind by a crashed or earlier run (ranks confirm with a nonce that the segment they
 * mapped is the one this run's rank 0 created, and attach again otherwise). */
#define BG_COMM_ID_BYTES 128
typedef struct bg_comm bg_comm;
int bg_shard_range(uint64_t n_units, int rank, int world, uint64_t* lo, uint64_t* hi);
int bg_shard_balanced(const uint64_t* costs, uint64_t n, int world, uint64_t* bounds);
int bg_comm_unique_id(uint8_t* id /* BG_COMM_ID_BYTES */);
int bg_comm_init(bg_ctx* ctx, int rank, int world, const uint8_t* id /* BG_COMM_ID_BYTES */, bg_comm** out);
int bg_comm_init_host(bg_ctx* ctx, int rank, int world, const char* name, bg_comm** out);
int bg_gather_records(bg_comm* comm, const void* local, uint64_t n_local, uint32_t rec_bytes, void* all, uint64_t* counts_out,
                      void* stream);
int bg_gather_records_cap(bg_comm* comm, const void* local, uint64_t n_local, uint32_t rec_bytes, void* all, uint64_t all_cap,
                          uint64_t* counts_out, void* stream);
/* ... for records in HOST memory (the results of the host-buffer entry points): staged through device scratch (sized from
 * the gathered counts) for an RCCL communicator, through the shared segment for a host-staged one; all_cap = records `all`
 * can hold: BG_ERR_OPS_CAP on every rank, nothing written, if the ranks bring more.  Synchronous. */
int bg_gather_records_host(bg_comm* comm, const void* local, uint64_t n_local, uint32_t rec_bytes, void* all, uint64_t all_cap,
                           uint64_t* counts_out);
/* What the communicator is, read back from the library that runs it — so that a multi-GPU line can prove "RCCL saw N
 * ranks" instead of repeating what the caller asked for.  info (5 entries): [0] world as given to bg_comm_init*,
 * [1] ncclCommCount() of the RCCL communicator (0 for a host-staged one: no RCCL involved), [2] ncclCommUserRank() (-1
 * host-staged), [3] path of the last gather: 0 none yet, 1 one ncclAllGather, 2 grouped ncclBroadcasts (ragged shards),
 * 3 host-staged through shared memory, [4] gathers done on this communicator. */
int bg_comm_world(bg_comm* comm, int64_t* info);
int bg_comm_free(bg_comm* comm);

/* Timing of the last *_dev / batch call's kernels on this ctx, measured with HIP events on
 * the stream the kernels ran on (used by bench.py for the roofline line). */
typedef struct {
    float fill_ms, traceback_ms, fm_ms;
    uint32_t fill_launches, traceback_launches, fm_launches;
} bg_timing_t;
int bg_get_timing(bg_ctx* ctx, bg_timing_t* out);
/* Pairs of the last banded call on this ctx that the packed-int16 fill flagged (a band cell below the floor of its strip's
 * 16-bit range) and the int32 kernels recomputed.  Waits for the call's kernels. */
int bg_band_redo_pairs(bg_ctx* ctx, uint64_t* out);
/* Fill kernel families, one bit each, for bg_last_fill_kernels. */
enum {
    BG_FILL_K1_WIDE = 0x1,       /* K1, int32 values (sw_fill.inc) */
    BG_FILL_K1_NARROW = 0x2,     /* K1, scaled int32 keys */
    BG_FILL_K1_LF = 0x4,         /* K1's local flavour (scaled keys, no clip machinery) */
    BG_FILL_K1P = 0x8,           /* K1p, two pairs per lane in int16 halves (sw_fill_pk16.inc) */
    BG_FILL_K1P_LF = 0x10,       /* K1p's local flavour */
    BG_FILL_K3 = 0x20,           /* banded, one pair per wavefront (banded_fill.hip) */
    BG_FILL_K3V2_WIDE = 0x40,    /* banded, eight pairs per wavefront, int32 values (banded_fill2.inc) */
    BG_FILL_K3V2_NARROW = 0x80,  /* ... scaled int32 keys */
    BG_FILL_K3I = 0x100,         /* banded interior runs, scaled int32 keys (banded_fill2i.hip) */
    BG_FILL_K3P = 0x200          /* banded interior runs, uint16 keys per strip (banded_fill2p.hip) */
};
/* The fill kernel families the last bg_align_batch* or bg_align_banded_* call on this ctx launched, OR-ed over its
 * sub-batches (BG_FILL_* bits; 0 before the first such call).  A family counts when it was launched, even if it found
 * nothing to do (K3i behind K3p only recomputes the pairs K3p flagged). */
int bg_last_fill_kernels(bg_ctx* ctx, uint32_t* mask);
/* 1 when the last bg_align_batch* call ran K1p's local flavour (BG_FILL_K1P_LF) with its keys in the offset frame (the cell
 * taken where every key fits it; the option "no_pk16_frame" turns it off), else 0. */
int bg_last_fill_framed(bg_ctx* ctx, int* framed);
/* 1 when that framed cell was the one of v_pk_maximum3_f16: best key and row maxima by maxima of three, the local floor
 * through D, the match term by one saturating subtract.  Taken where every key of the frame is also a finite
 * half-precision bit pattern, below 0x7c00, and a match is worth at most 15 more than a mismatch (16 (match - mismatch)
 * + 2 <= 256); the option "no_pk16_max3" turns it off: same results, the cell of v_pk_max_i16.  Else 0.  Implies
 * bg_last_fill_framed. */
int bg_last_fill_max3(bg_ctx* ctx, int* max3);
int bg_enable_timing(bg_ctx* ctx, int on);

#ifdef __cplusplus
}
#endif
#endif
