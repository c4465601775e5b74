// C-ABI entry points of the banded aligner: bg_align_banded_batch, bg_band_create_batch.
// Host side of `banded::Aligner::{custom,global,semiglobal,local}` (pairwise/banded.rs:282,872,901,972):
// the wrappers' clip overrides, Band::create per pair on host threads (band_host.cpp), the
// MAX_CELLS early-out (banded.rs:104,407-420), then K3 + K4 over sub-batches.
#include <algorithm>
#include <atomic>
#include <functional>
#include <thread>

#include "band_host.h"
#include <sched.h>

#include <chrono>

#include "band_device.h"
#include "banded_kernels.h"

using namespace bgband_dev;

int bg_compact_matrix(const int32_t* matrix, std::vector<uint8_t>& code_map, std::vector<int32_t>& table);

namespace bgband { extern std::atomic<uint64_t> g_prof[4]; }
namespace {

constexpr uint64_t kMaxCells = 5000000;  // banded.rs:104

struct HostPair {
    uint32_t m = 0, n = 0, flags = BP_OK;
    uint32_t start_0 = 0, end_0 = 0, start_n = 0, end_n = 0;
    uint64_t cells = 0;
    uint64_t tb_bytes = 0;
};

unsigned host_threads() { return bg_host_threads(); }

bgband::ClipScores clip_scores(const bg_scoring_t* sc, int mode) {
    bgband::ClipScores c;
    c.gap_open = sc->gap_open;
    c.gap_extend = sc->gap_extend;
    c.xclip_prefix = sc->xclip_prefix;
    c.xclip_suffix = sc->xclip_suffix;
    c.yclip_prefix = sc->yclip_prefix;
    c.yclip_suffix = sc->yclip_suffix;
    // banded.rs:872-1004: the wrappers overwrite the clips before Band::create runs
    if (mode == BG_MODE_GLOBAL) c.xclip_prefix = c.xclip_suffix = c.yclip_prefix = c.yclip_suffix = BG_MIN_SCORE;
    if (mode == BG_MODE_SEMIGLOBAL) {
        c.xclip_prefix = c.xclip_suffix = BG_MIN_SCORE;
        c.yclip_prefix = c.yclip_suffix = 0;
    }
    if (mode == BG_MODE_LOCAL) c.xclip_prefix = c.xclip_suffix = c.yclip_prefix = c.yclip_suffix = 0;
    c.match_score = sc->match_score;
    c.match_scores_some = sc->match_scores_some != 0;
    return c;
}

// Per-column row ranges -> per-row column ranges, written straight into the pinned staging arrays.
// For a monotone band (Band::monotone) the columns containing row i form one interval: its first
// column is the first one whose range reaches down to i, its last the last one starting at or above
// i — two O(m + n) sweeps instead of visiting every band cell.
void rows_from_columns(const bgband::Band& b, HostPair& hp, int2* rowc, uint32_t* row_off) {
    const uint32_t m = hp.m, n = hp.n;
    for (uint32_t i = 0; i <= m; i++) rowc[i] = make_int2(1, 0);
    uint32_t done = 0;  // rows < done were inside an earlier column
    for (uint32_t j = 0; j <= n; j++) {
        if (b.end[j] <= b.start[j]) continue;
        const uint32_t e = std::min<uint32_t>(b.end[j], m + 1);
        for (uint32_t i = std::max(b.start[j], done); i < e; i++) rowc[i].x = (int)j;
        done = std::max(done, e);
    }
    uint32_t lim = m + 1;  // rows >= lim are inside a later column
    for (uint32_t j = n + 1; j-- > 0;) {
        if (b.end[j] <= b.start[j]) continue;
        const uint32_t e = std::min<uint32_t>(std::min<uint32_t>(b.end[j], m + 1), lim);
        for (uint32_t i = b.start[j]; i < e; i++) rowc[i].y = (int)j;
        lim = std::min(lim, b.start[j]);
    }
    uint64_t off = 0, covered = 0;
    row_off[0] = 0;  // row 0 is a closed form, not stored
    if (rowc[0].y >= rowc[0].x) covered += (uint64_t)(rowc[0].y - rowc[0].x + 1);
    // rows 1..m in line groups of eight: 16-cell groups, the groups of the eight rows interleaved (banded_kernels.h)
    for (uint32_t q0 = 0; q0 < m; q0 += kTbLineRows) {
        uint64_t groups = 0;
        for (uint32_t q = q0; q < std::min(m, q0 + kTbLineRows); q++) {
            const int2 rc = rowc[q + 1];
            if (rc.y >= rc.x) {
                covered += (uint64_t)(rc.y - rc.x + 1);
                groups = std::max<uint64_t>(groups, ((uint64_t)(rc.y - rc.x + 1) + (kTbRowAlign - 1)) / kTbRowAlign);
            }
        }
        for (uint32_t q = q0; q < std::min(m, q0 + kTbLineRows); q++) row_off[q + 1] = (uint32_t)(off + (q - q0) * kTbRowAlign);
        off += groups * kTbGroupStride;
    }
    hp.tb_bytes = (off + 15) & ~15ull;
    // every row's band columns must form ONE interval (no holes) for the device layout
    if (covered != hp.cells || off > 0xFFFFFFF0ull) hp.flags = BP_UNSUPPORTED;
}

// everything the device needs to know about one pair's band (the band itself is already in `band`)
void build_pair(uint32_t m, uint32_t n, const bgband::Band& band, HostPair& hp, int2* rowc, uint32_t* row_off) {
    hp.m = m;
    hp.n = n;
    hp.flags = BP_OK;
    hp.tb_bytes = 0;
    hp.cells = band.num_cells();
    hp.start_0 = band.start[0];
    hp.end_0 = band.end[0];
    hp.start_n = band.start[n];
    hp.end_n = band.end[n];
    if (hp.cells > kMaxCells) {
        hp.flags = BP_TOO_MANY_CELLS;
    } else if (n == 0 || !band.monotone()) {
        // with an empty y the reference's own traceback does not terminate in most modes;
        // non-monotone bands never come out of Band::create
        hp.flags = BP_UNSUPPORTED;
    } else {
        rows_from_columns(band, hp, rowc, row_off);
    }
    if (hp.flags != BP_OK) {
        for (uint32_t i = 0; i <= m; i++) {
            rowc[i] = make_int2(1, 0);
            row_off[i] = 0;
        }
        hp.tb_bytes = 0;
    }
}

// grow-only pinned host buffer
int pinned_reserve(void** p, size_t* cur, size_t need) {
    if (need <= *cur) return BG_OK;
    if (*p) {
        hipHostFree(*p);
        *p = nullptr;
        *cur = 0;
    }
    need = (need + 4095) & ~(size_t)4095;
    BG_HIP(hipHostMalloc(p, need, hipHostMallocDefault));
    *cur = need;
    return BG_OK;
}

}  // namespace

// The device arrays of a host-buffer call: its sequences, offsets, records and strided operation slots.
enum BandIoBuf { kIoX, kIoY, kIoXOff, kIoYOff, kIoOut, kIoOps, kBandIoBufs };

// The device band builder's own arrays (band_device.hip), one slice per pair of a sub-batch.
enum BandBuildBuf {
    kHead, kNext, kHy,                     // B1: the k-mer table of y
    kMx, kMy, kPath, kQpos, kUpos, kCont,  // B1, B2: cap_matches entries per pair
    kColStart, kColEnd,                    // B3: max_n + 1 row ranges per pair
    kState,                                // the BandDevPair the host reads back
    kRow0,                                 // n_pairs + 1 first rows inside rowc / row_off
    kGTree, kGScore, kGBack,               // B2 with its tree in global memory
    kBandBuildBufs
};
// One line per array: its bytes for the d.n_pairs pairs of a sub-batch, and the BandDevArgs member it backs.
// band_join reserves and binds from this table alone.
struct BandBuildSlot {
    BandBuildBuf name;
    size_t (*bytes)(const BandDevArgs& d);
    void (*bind)(BandDevArgs& d, void* p);
};
#define BAND_SLOT(name, member, expr)                                                                              \
    {name, [](const BandDevArgs& d) -> size_t { const size_t n = d.n_pairs; return expr; },           \
     [](BandDevArgs& d, void* p) { d.member = (decltype(d.member))p; }}
const BandBuildSlot kBandBuildSlots[kBandBuildBufs] = {
    BAND_SLOT(kHead, head, n * d.table_size * 4),
    BAND_SLOT(kNext, next, n * d.max_n * 4),
    BAND_SLOT(kHy, hy, n * d.max_n * 8),
    BAND_SLOT(kMx, mx, n * d.cap_matches * 4),
    BAND_SLOT(kMy, my, n * d.cap_matches * 4),
    BAND_SLOT(kPath, path, n * d.cap_matches * 4),
    BAND_SLOT(kQpos, qpos, n * d.cap_matches * 4),
    BAND_SLOT(kUpos, upos, n * d.cap_matches * 4),
    BAND_SLOT(kCont, cont, n * d.cap_matches * 4),
    BAND_SLOT(kColStart, col_start, n * (d.max_n + 1) * 4),
    BAND_SLOT(kColEnd, col_end, n * (d.max_n + 1) * 4),
    BAND_SLOT(kState, state, n * sizeof(BandDevPair)),
    BAND_SLOT(kRow0, row0, (n + 1) * 8),
    BAND_SLOT(kGTree, g_tree, n * (d.cap_matches + 1) * 16),
    BAND_SLOT(kGScore, g_score, n * d.cap_matches * 4),
    BAND_SLOT(kGBack, g_back, n * d.cap_matches * 2),
};
#undef BAND_SLOT

// Scratch that survives between calls (bg_ctx::band): two sets, so that the traceback of one
// sub-batch (K4, latency bound, a handful of wavefronts) overlaps the fill of the next one (K3) and
// the host threads that build the following band.  Who records and who waits for each event: see band_run.
struct bg_band_scratch {
    struct Set {
        // pinned staging
        void *h_pairs = nullptr, *h_rowc = nullptr, *h_roff = nullptr;
        size_t hc_pairs = 0, hc_rowc = 0, hc_roff = 0;
        // device
        void *d_pairs = nullptr, *d_rowc = nullptr, *d_roff = nullptr, *d_tb = nullptr, *d_aux = nullptr;
        size_t dc_pairs = 0, dc_rowc = 0, dc_roff = 0, dc_tb = 0, dc_aux = 0;
        hipEvent_t copied = nullptr, filled = nullptr, traced = nullptr, built = nullptr, matched = nullptr;
        bool built_valid = false;  // `built` has been recorded in this call
        hipEvent_t fill_gone = nullptr;  // the fill kernel itself is off the device (its epilogue may still run)
        hipEvent_t pre_done = nullptr;   // ... and what its preparation stream (aux_stream) did for it is done
        hipEvent_t cleared = nullptr;    // the aux block has been zeroed (on aux_stream)
        bool busy = false;
    } set[2];
    // device band builder (band_device.hip): its own arrays, one set per sub-batch parity (the join of c + 2 runs next to
    // the chaining of c + 1), and its per-pair state
    void* build[2][kBandBuildBufs] = {};
    size_t build_cap[2][kBandBuildBufs] = {};
    hipStream_t build_stream = nullptr;
    hipEvent_t seq_ready = nullptr;
    void* h_state = nullptr;  // pinned copy of the builder's BandDevPair array
    size_t h_state_cap = 0;
    void* io[kBandIoBufs] = {};
    size_t io_cap[kBandIoBufs] = {};
    void* h_ops = nullptr;  // pinned landing zone of the operations
    size_t h_ops_cap = 0;
    void *d_cmp = nullptr, *d_cscan = nullptr;  // host-buffer flavour: the operations compacted on the device, scan scratch
    size_t d_cmp_cap = 0, d_cscan_cap = 0;
    uint64_t* d_cell = nullptr;                 // ... and their running byte count over the sub-batches of a call
    uint64_t* d_dlslot = nullptr;               // per sub-batch {bytes, end offset} of its compacted operations (ring of kDlSlots)
    hipStream_t dl_stream = nullptr;            // ... which a few blocks on this high-priority stream bring to h_ops meanwhile
    static constexpr uint64_t kDlSlots = 1024;
    hipStream_t tb_stream = nullptr;
    hipStream_t aux_stream = nullptr;   // clears the aux block of the next sub-batch under the running fill, and prepares that fill
    hipStream_t copy_stream = nullptr;  // host-buffer flavour: sequence slices go up here; the k-mer join runs here
    uint32_t* d_started = nullptr;  // blocks of the K3v2 launches of the current call that have started (see banded_fill2.hip)
    uint32_t started_target = 0;    // ... and how many have been launched
};

extern "C" int bg_band_redo_pairs(bg_ctx* ctx, uint64_t* out) {
    if (!ctx || !out) return BG_ERR_INVALID_ARG;
    *out = 0;
    if (!ctx->band || !ctx->band->d_started) return BG_OK;
    BG_HIP(hipSetDevice(ctx->device));  // (the caller's current device may be another one: several contexts, torch elsewhere)
    BG_HIP(hipDeviceSynchronize());
    uint32_t v = 0;
    BG_HIP(hipMemcpy(&v, ctx->band->d_started + 1, 4, hipMemcpyDeviceToHost));
    *out = v;
    return BG_OK;
}

void bg_band_scratch_free(bg_band_scratch* b) {
    if (!b) return;
    for (auto& s : b->set) {
        hipHostFree(s.h_pairs); hipHostFree(s.h_rowc); hipHostFree(s.h_roff);
        hipFree(s.d_pairs); hipFree(s.d_rowc); hipFree(s.d_roff); hipFree(s.d_tb); hipFree(s.d_aux);
        for (hipEvent_t e : {s.copied, s.filled, s.traced, s.built, s.matched, s.fill_gone, s.pre_done, s.cleared})
            if (e) hipEventDestroy(e);
    }
    for (void* p : b->io) hipFree(p);
    for (auto& set : b->build)
        for (void* p : set) hipFree(p);
    hipFree(b->d_cmp);
    hipFree(b->d_cscan);
    hipFree(b->d_cell);
    hipFree(b->d_dlslot);
    hipFree(b->d_started);
    hipHostFree(b->h_state);
    hipHostFree(b->h_ops);
    for (hipStream_t s : {b->dl_stream, b->tb_stream, b->aux_stream, b->copy_stream, b->build_stream})
        if (s) hipStreamDestroy(s);
    if (b->seq_ready) hipEventDestroy(b->seq_ready);
    delete b;
}

namespace {

template <typename F>
void parallel_for(uint64_t n, uint64_t grain, F&& fn) {
    unsigned nt = host_threads();
    nt = (unsigned)std::min<uint64_t>(nt, std::max<uint64_t>(1, n / grain));
    if (nt <= 1) {
        fn(0, 0, n);
        return;
    }
    std::atomic<uint64_t> next{0};
    bg_pool_run(nt, [&](unsigned t) {
        for (;;) {
            const uint64_t lo = next.fetch_add(grain);
            if (lo >= n) break;
            fn(t, lo, std::min<uint64_t>(n, lo + grain));
        }
    });
}

int check_scoring(const bg_scoring_t* sc) {
    if (sc->gap_open > 0 || sc->gap_extend > 0 || sc->xclip_prefix > 0 || sc->xclip_suffix > 0 ||
        sc->yclip_prefix > 0 || sc->yclip_suffix > 0)
        return BG_ERR_POSITIVE_PENALTY;
    return BG_OK;
}

}  // namespace

// Band::create for a batch (banded.rs:1278): writes n+1 half-open row ranges per pair at
// band_off[p] (same offsets for start and end); band_cells = Band::num_cells.
extern "C" int bg_band_create_batch(const bg_scoring_t* sc, int mode, uint32_t k, uint32_t w, uint64_t n_pairs,
                                    const uint8_t* x, const uint64_t* x_off, const uint8_t* y, const uint64_t* y_off,
                                    const uint64_t* band_off, uint32_t* start, uint32_t* end, uint64_t* band_cells) {
    if (!sc || !x_off || !y_off || (n_pairs && (!band_off || !start || !end))) return BG_ERR_INVALID_ARG;
    int rc = check_scoring(sc);
    if (rc) return rc;
    const bgband::ClipScores cs = clip_scores(sc, mode);
    parallel_for(n_pairs, 4, [&](unsigned, uint64_t lo, uint64_t hi) {
        bgband::Band band;
        bgband::Workspace ws;
        for (uint64_t p = lo; p < hi; p++) {
            const uint32_t m = (uint32_t)(x_off[p + 1] - x_off[p]), n = (uint32_t)(y_off[p + 1] - y_off[p]);
            band.create(x + x_off[p], m, y + y_off[p], n, k, w, cs, ws);
            memcpy(start + band_off[p], band.start.data(), (size_t)(n + 1) * 4);
            memcpy(end + band_off[p], band.end.data(), (size_t)(n + 1) * 4);
            if (band_cells) band_cells[p] = band.num_cells();
        }
    });
    if (getenv("BG_TRACE")) fprintf(stderr, "[bg banded] cpu-ms: kmers %.1f sdp %.1f band %.1f (threads %u)\n", bgband::g_prof[0] / 1e6, bgband::g_prof[1] / 1e6, bgband::g_prof[2] / 1e6, host_threads());
    return BG_OK;
}

namespace {

// `make_band(p, cs, band, ws)` fills the band of pair p under the call's clip scores; false = invalid input.
// Called once per pair, from host threads only.
using BandMaker = std::function<bool(uint64_t, const bgband::ClipScores&, bgband::Band&, bgband::Workspace&)>;

// One call of any of the three entry points.
//   dev          false: x, y, out, ops are the caller's host buffers, the operations come back compacted (ops_cap, ops_used);
//                true: they are device pointers and stay in HBM, d_x_off / d_y_off are the offsets' device copies and every
//                pair has a slot of ops_stride >= max_x + max_y + 4 bytes in ops (ops may be null)
//   x_off, y_off on the host, always: the host side of the pipeline needs the lengths
//   has_kw       the bands come from Band::create with (k, w): the device builder applies; otherwise only make_band knows them
struct BandCall {
    bg_ctx* ctx = nullptr;
    const bg_scoring_t* sc = nullptr;
    int mode = 0;
    uint64_t n_pairs = 0;
    const uint64_t *x_off = nullptr, *y_off = nullptr;
    bool dev = false;
    const uint8_t *x = nullptr, *y = nullptr;
    const uint64_t *d_x_off = nullptr, *d_y_off = nullptr;
    bg_alignment_t* out = nullptr;
    uint8_t* ops = nullptr;
    uint64_t ops_cap = 0, ops_stride = 0;
    uint64_t* ops_used = nullptr;
    uint64_t* band_cells = nullptr;
    bool has_kw = false;
    uint32_t k = 0, w = 0;
    BandMaker make_band;
};

// Streams of the pipeline by queue priority.  The runtime maps a process's streams onto a few hardware queues PER PRIORITY
// LEVEL, and a hardware queue hands out its packets in order: a short kernel queued behind a long, starved one (the k-mer
// join under a fill) waits for that one's last block to be dispatched, whatever streams the two were launched on
// (profiles/r05_banded_timeline_hostsync.txt: the next fill's preparation started 1.3 ms after the join two sub-batches
// ahead ended, every cycle).  So the join goes to the low-priority queues, a fill's preparation to the high-priority
// ones, and neither can sit in front of the other or of the fill: the gap between two fills drops from 10.8 to 1.9 ms
// (profiles/r05_banded_timeline_prio.txt) — and the call gains nothing, because the join that used to run in that gap now
// starves under two fills in a row and the chaining behind it starts late (profiles/r05_banded_pipeline_experiments.txt).
int band_stream_create(hipStream_t* s, int level) {
    int lo = 0, hi = 0;
    if (level == 0 || hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess || lo == hi)
        return hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess ? BG_OK : BG_ERR_HIP;
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, level > 0 ? hi : lo) == hipSuccess ? BG_OK : BG_ERR_HIP;
}

// Every stream and event of the pipeline, at the context's first banded call (bg_band_scratch_free destroys them).
//   tb_stream     K4, the compaction and the final download
//   copy_stream   low priority: the sequence slices of a host-buffer call, and every k-mer join with its chain preparation.
//                 (The join has no stream of its own: the process maps its streams onto a handful of hardware queues, and two
//                 more of them cost the full bench — a dozen streams by then — 12 % of this leg where the leg alone gained 3 %;
//                 it shares the stream of the sequence uploads, which it waits for anyway.)
//   build_stream  the rest of the device builder: chaining, raster, row ranges, state read-back
//   aux_stream    high priority: clears the aux block and prepares the next fill (it shares the stream that clears the aux
//                 block: the clear is one of the things the preparation waits for)
//   dl_stream     high priority, only once a host-buffer call wants operations: brings them to the pinned buffer
int band_scratch_create(bg_band_scratch* b, bool want_ops) {
    int rc;
    if (!b->tb_stream) {
        if ((rc = band_stream_create(&b->tb_stream, 0))) return rc;
        if (want_ops && (rc = band_stream_create(&b->dl_stream, 1))) return rc;
        if ((rc = band_stream_create(&b->copy_stream, -1))) return rc;
        if ((rc = band_stream_create(&b->build_stream, 0))) return rc;
        if ((rc = band_stream_create(&b->aux_stream, 1))) return rc;
        for (auto& s : b->set)
            for (hipEvent_t* e : {&s.copied, &s.filled, &s.traced, &s.built, &s.matched, &s.fill_gone, &s.pre_done, &s.cleared})
                BG_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
        BG_HIP(hipEventCreateWithFlags(&b->seq_ready, hipEventDisableTiming));
        BG_HIP(hipMalloc((void**)&b->d_started, 64));
    }
    if (want_ops) {
        if (!b->dl_stream && (rc = band_stream_create(&b->dl_stream, 1))) return rc;
        if (!b->d_cell) BG_HIP(hipMalloc((void**)&b->d_cell, 64));
        if (!b->d_dlslot) BG_HIP(hipMalloc((void**)&b->d_dlslot, bg_band_scratch::kDlSlots * 16));
    }
    return BG_OK;
}
int band_scratch_init(bg_ctx* ctx, bool want_ops) {
    if (ctx->band) return band_scratch_create(ctx->band, want_ops);
    bg_band_scratch* b = new bg_band_scratch;
    const int rc = band_scratch_create(b, want_ops);
    if (rc) {
        bg_band_scratch_free(b);  // (a half-made scratch is not kept)
        return rc;
    }
    ctx->band = b;
    return BG_OK;
}

// Which fill a call runs.  Everything here depends on the scoring, the longest sequences, the context's test options and the
// call's size — not on the sub-batch, which only adds its pairs and pointers (band_stage).
struct BandFillPlan {
    int sm = SCORE_PARAMS;  // where the kernels read the match function (SCORE_*)
    bool narrow = false;    // the scaled-key variant of K3v2 applies
    bool small_k3 = false;  // a whole small call: K3
    bool v2 = false;        // launch_band_fill2 (K3v2 with K3i / K3p for the interior runs); false: K3
    int32_t split = 0, packed = 0, pk_thresh = 0;  // BandArgs members of the same names
};

// `sc`: the scoring with the mode's clips applied; `alpha`: the compacted alphabet of a tabulated match function, 0 without one
BandFillPlan plan_band_fill(const SwScoring& sc, int alpha, uint64_t max_x, uint64_t max_y, const bg_ctx* ctx, uint64_t n_pairs) {
    BandFillPlan f;
    if (alpha) f.sm = alpha <= kMaxLdsAlphabet ? SCORE_LDS : SCORE_GLOBAL;
    // every reachable score within 24 bits: the scaled-key variant of K3v2 applies (same bound as sw_api.hip)
    const int64_t mag = std::max<int64_t>({std::abs((int64_t)sc.go), std::abs((int64_t)sc.ge), std::abs((int64_t)sc.match),
                                           std::abs((int64_t)sc.mismatch), 1});
    auto clip_ok = [](int32_t c) { return c <= kNarrowNegClip || c >= -(1 << 22); };  // 'minus infinity' or small (banded_kernels.h)
    f.narrow = !ctx->force_wide && mag * ((int64_t)max_x + (int64_t)max_y + 8) < (1 << 24) && clip_ok(sc.xp) && clip_ok(sc.xs) &&
               clip_ok(sc.yp) && clip_ok(sc.ys);
    // Geometry by call size: K3v2 binds a pair to 8 lanes for ~30 ms whatever the batch (throughput comes from the
    // 16 384 pairs in flight); a small call finishes sooner with one pair per wavefront (K3: 19 ms; measured cross-over
    // between 2 048 and 4 096 pairs, tools/exp/time_banded_small.py).  band_fill_v1: 1 always K3, -1 never (tests)
    // (a sub-batch is never larger than its call; the short remainder sub-batch of a large call runs first, under the next
    // one's band construction: K3v2 / K3p there)
    f.small_k3 = ctx->band_fill_v1 >= 0 && n_pairs <= 2048;
    f.v2 = f.sm == SCORE_PARAMS && ctx->band_fill_v1 <= 0 && !f.small_k3;
    if (!f.v2) return f;  // K3 takes no interior runs (split = 0: K4 reads it too)
    // interior runs (band_split): scaled keys, x kept whole, a real y-prefix clip — semiglobal-like scorings
    f.split = (f.narrow && !ctx->band_interior_off && sc.xp <= kNarrowNegClip && sc.xs <= kNarrowNegClip && sc.yp > kNarrowNegClip) ? 1 : 0;
    // ... and, where the scoring and the lengths fit its 16-bit strip-relative keys, K3p takes the runs first
    // (banded_fill2p.hip: target / threshold as computed there; at least 2^14 key units == 1024 score units of room)
    const int64_t mk = ((int64_t)sc.match << 4) + 12, mis = ((int64_t)-sc.mismatch << 4) - 10;
    const int64_t target = (0xfff0 - (mk + mis) - ((int64_t)sc.match << 9) - 32) & ~15ll;
    const int64_t thresh = ((int64_t)sc.match << 9) + 16 + ((int64_t)-sc.go << 4) + 32;
    f.packed = (f.split && !ctx->band_packed_off && sc.match >= 0 && sc.match <= 64 && sc.mismatch <= -1 && sc.mismatch >= -1024 &&
                sc.go <= -1 && sc.go >= -1024 && sc.ge <= 0 && sc.ge >= -1024 && max_y < 65536 && target - thresh >= (1 << 14)) ? 1 : 0;
    f.pk_thresh = (int32_t)ctx->band_packed_thresh;
    return f;
}

// `f` under the context's timing events: with ctx->timing its span on `st` adds to *ms and counts as one launch
template <typename F>
int timed(bg_ctx* ctx, hipStream_t st, hipEvent_t* ev, float* ms, uint32_t* launches, F&& f) {
    if (ctx->timing) BG_HIP(hipEventRecord(ev[0], st));
    const int rc = f();
    if (rc) return rc;
    BG_HIP(hipGetLastError());
    if (!ctx->timing) return BG_OK;
    BG_HIP(hipEventRecord(ev[1], st));
    BG_HIP(hipEventSynchronize(ev[1]));
    float span = 0;
    BG_HIP(hipEventElapsedTime(&span, ev[0], ev[1]));
    *ms += span;
    *launches += 1;
    return BG_OK;
}

// One sub-batch in flight.  Two exist, by parity: while K3 / K4 of one run, the band of the next one is being built — by
// band_device.hip on its own stream, or by the host threads.  The vectors and the builder's arguments outlive the sub-batch:
// the next one of the same parity reuses them.
struct BandPass {
    unsigned parity = 0;
    bg_band_scratch::Set* S = nullptr;
    uint64_t n = 0;                  // the sub-batch's number in its call
    uint64_t p0 = 0, want = 0;       // pairs [p0, p0 + want) have a band ...
    uint64_t take = 0;               // ... and the first `take` of them fit the scratch budget (band_collect)
    uint64_t tb_bytes = 0, aux_words = 0;  // what those need
    bool matched = false;            // the k-mer join of [p0, p0 + want) has been launched (band_join)
    BandDevArgs d = {};
    std::vector<HostPair> hp;
    std::vector<uint64_t> row0;
    hipStream_t sp = nullptr;        // the stream that prepares this sub-batch's fill (see BandRun::use_pre)
    BandArgs a = {};
};

// What the sub-batches of a call share.
struct BandRun {
    const BandCall& c;
    bg_ctx* ctx;
    bg_band_scratch& B;
    hipStream_t st, st_tb, st_build, st_join;  // the caller's stream (fills), B.tb_stream, B.build_stream, B.copy_stream
    bgband::ClipScores cs;
    uint64_t max_x = 0, max_y = 0;
    uint64_t chunk_pairs = 0;  // sub-batch size: enough wavefronts to fill the chip, small enough that a large batch pipelines
    uint64_t first_want = 0;   // the remainder sub-batch that goes first (band_want), 0: none
    uint64_t grain = 1;        // pairs per piece of work of the host builder
    uint64_t budget = 0;       // traceback + aux bytes a scratch set may take
    bool build_on_device = false;
    // The preparation of a fill — the pair table's upload, the waits for the band, the cleared aux block and the sequences,
    // and K3v2's phase 1 (the strips before the interior runs) — does not depend on the fill before it, but on the fill
    // stream it queued behind it: 2 ms between two long kernels, every cycle.  On a stream of its own (aux_stream) it runs
    // under the previous fill's tail (event timing keeps one stream).
    bool use_pre = false;
    bool compact_on_device = false;  // host-buffer call with operations: compacted on the device, sub-batch by sub-batch
    BandFillPlan plan;
    band_fill_fn fill = nullptr;  // K3 of the plan's score source
    BandArgs a = {};              // what every sub-batch's kernels share
    // host-buffer call: sequence slices (pairs [k * chunk_pairs, (k + 1) * chunk_pairs)) and their upload events;
    // ev[0]: the offsets are up, ev[k + 1]: slice k is on the device
    std::vector<hipEvent_t> slice_ev;
    uint64_t n_slices = 0, slices_up = 0;
    uint64_t waited_fill = 0, waited_join = 0, waited_pre = 0;  // slices the fill / join / preparation stream has waited for
    BandPass pass[2];
    // BG_TRACE laps of the host thread
    bool trace = false;
    std::chrono::steady_clock::time_point t_last;

    BandRun(const BandCall& call, bg_band_scratch& scratch) : c(call), ctx(call.ctx), B(scratch) {}
    ~BandRun() {
        for (hipEvent_t e : slice_ev)
            if (e) hipEventDestroy(e);
    }
    void lap(const char* what) {
        if (!trace) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[bg banded] %-18s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t_last).count());
        t_last = t1;
    }
    void lap_cpu() const {
        if (trace) fprintf(stderr, "[bg banded] cpu-ms: kmers %.1f sdp %.1f band %.1f (threads %u)\n", bgband::g_prof[0] / 1e6, bgband::g_prof[1] / 1e6, bgband::g_prof[2] / 1e6, host_threads());
    }
};

// Sub-batch sizes: a batch that is not a whole number of sub-batches takes its REMAINDER FIRST.  A fill is one round
// of resident wavefronts that lasts as long as its slowest pair whatever the sub-batch size, so a short sub-batch at
// the end costs a full fill with the device idle around it (100 000 pairs = 6 x 16 384 + 1 696: 30 ms of 345); up
// front it runs under the band construction of the first full sub-batch, which nothing else would overlap.
uint64_t band_want(const BandRun& R, uint64_t p0) {
    if (p0 == 0 && R.first_want) return R.first_want;
    return std::min<uint64_t>(R.chunk_pairs, R.c.n_pairs - p0);
}

// Host-buffer call: the sequences go up in slices of one sub-batch each on the copy stream: the first sub-batch starts
// after 1 / n-th of the upload, the rest travels under its band construction and fill.  Slices [slices_up, upto).
int band_upload_slices(BandRun& R, uint64_t upto) {
    const BandCall& c = R.c;
    hipStream_t cp = R.B.copy_stream;
    for (; R.slices_up < std::min(upto, R.n_slices); R.slices_up++) {
        const uint64_t q0 = R.slices_up * R.chunk_pairs, q1 = std::min(c.n_pairs, q0 + R.chunk_pairs);
        if (R.slices_up == 0) {  // behind the offsets (and whatever the caller's stream ran before)
            hipEvent_t e0;
            BG_HIP(hipEventCreateWithFlags(&e0, hipEventDisableTiming));
            R.slice_ev.push_back(e0);
            BG_HIP(hipEventRecord(e0, R.st));
            BG_HIP(hipStreamWaitEvent(cp, e0, 0));
        }
        if (c.x_off[q1] > c.x_off[q0])
            BG_HIP(bg_copy_pieces((uint8_t*)R.a.x + c.x_off[q0], c.x + c.x_off[q0], c.x_off[q1] - c.x_off[q0], hipMemcpyHostToDevice, cp));
        if (c.y_off[q1] > c.y_off[q0])
            BG_HIP(bg_copy_pieces((uint8_t*)R.a.y + c.y_off[q0], c.y + c.y_off[q0], c.y_off[q1] - c.y_off[q0], hipMemcpyHostToDevice, cp));
        hipEvent_t e;
        BG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        R.slice_ev.push_back(e);
        BG_HIP(hipEventRecord(e, cp));
    }
    return BG_OK;
}

// stream `s` may touch the sequences of pairs [0, upto) only behind their slices
int band_need_seq(BandRun& R, hipStream_t s, uint64_t& waited, uint64_t upto) {
    if (!R.n_slices) return BG_OK;
    const uint64_t k1 = std::min(R.n_slices, (upto + R.chunk_pairs - 1) / R.chunk_pairs);
    const int rc = band_upload_slices(R, k1);
    if (rc) return rc;
    for (; waited < k1; waited++) BG_HIP(hipStreamWaitEvent(s, R.slice_ev[waited + 1], 0));
    return BG_OK;
}

// First half of the device builder for sub-batch n, which starts at p0: the k-mer join (B1) and the event
// preparation of the chaining.  They get along badly with a running fill (65 VGPRs and 20 KB of LDS per block, 16 KB
// of LDS per wavefront, against the 86 VGPRs per SIMD and 30 KB per CU two fill wavefronts leave: 10.7 + 3.2 ms alone,
// 40 + 35 ms under the fill), while the chaining's event loop (24 VGPRs, no LDS) loses little there.  So these two
// run for sub-batch c + 1 on the idle device just before fill c is launched — band_stage(c) calls this once it knows
// where c + 1 starts — and the event loop of c + 1 then has the whole fill to itself.  It touches nothing of the scratch
// set (K4 of c - 1 may still be reading that), only the builder's own arrays, which raster c has finished with.
// The join (and the chain preparation behind it) runs off the builder's stream: the builder's kernels are one chain per
// sub-batch — join, preparation, chaining, raster, row ranges — and under the fill that chain, not the fill, was the
// cycle (44 ms per 16 384 pairs, 14 of them the join).  With the builder's arrays twice the join of c + 2 runs next to
// the chaining of c + 1.
int band_join(BandRun& R, uint64_t p0, uint64_t n) {
    const BandCall& c = R.c;
    bg_band_scratch& B = R.B;
    BandPass& P = R.pass[n & 1];
    int rc = BG_OK;
    P.matched = false;
    if (!R.build_on_device) return BG_OK;
    const uint64_t want = band_want(R, p0);
    if ((rc = band_need_seq(R, R.st_join, R.waited_join, p0 + want))) return rc;
    // this parity's arrays were last read by the raster of two sub-batches ago
    if (n >= 2 && P.S->built_valid) BG_HIP(hipStreamWaitEvent(R.st_join, P.S->built, 0));
    // This join does not wait for the chaining of the sub-batch before it.  Under a running fill the registers two fill
    // wavefronts per SIMD leave hold EITHER that chaining OR this join plus a part of it, and whichever is dispatched
    // first keeps the other one in rounds.  Measured in round 5: ordering them costs more than the race (279 against
    // 265 ms per 100 000 pairs: the join then starves behind the raster and K4 instead, and the next chaining starts
    // late), so the dispatch order is left to the hardware.
    uint32_t max_m = 0, max_n = 0;
    for (uint64_t q = 0; q < want; q++) {
        max_m = std::max<uint32_t>(max_m, (uint32_t)(c.x_off[p0 + q + 1] - c.x_off[p0 + q]));
        max_n = std::max<uint32_t>(max_n, (uint32_t)(c.y_off[p0 + q + 1] - c.y_off[p0 + q]));
    }
    BandDevArgs d = {};
    d.x = R.a.x, d.x_off = R.a.x_off, d.y = R.a.y, d.y_off = R.a.y_off;
    d.pair0 = p0;
    d.n_pairs = (uint32_t)want;
    d.k = c.k, d.w = c.w;
    d.gap_open = R.cs.gap_open, d.gap_extend = R.cs.gap_extend;
    d.xclip_prefix = R.cs.xclip_prefix, d.xclip_suffix = R.cs.xclip_suffix;
    d.yclip_prefix = R.cs.yclip_prefix, d.yclip_suffix = R.cs.yclip_suffix;
    d.match_score = (uint32_t)(R.cs.match_scores_some ? R.cs.match_score : 2);  // banded.rs:105,1315-1318
    d.max_m = max_m;
    d.max_n = std::max<uint32_t>(max_n, 1);
    d.table_bits = 4;
    while ((1u << d.table_bits) < 2 * d.max_n) d.table_bits++;
    d.table_size = 1u << d.table_bits;
    d.cap_matches = kMaxChainMatches + 1;
    d.chain_global = R.ctx->band_chain_global;
    d.chain_rows = R.ctx->band_chain_rows ? 1 : 0;
    d.join_global = R.ctx->band_join_global ? 1 : 0;
    for (const BandBuildSlot& s : kBandBuildSlots) {
        void** p = &B.build[P.parity][s.name];
        if ((rc = bg_reserve(p, &B.build_cap[P.parity][s.name], std::max<size_t>(s.bytes(d), 64)))) return rc;
        s.bind(d, *p);
    }
    if ((rc = launch_band_match(d, R.st_join))) return rc;
    if ((rc = launch_band_chain(d, R.st_join, 1))) return rc;
    BG_HIP(hipEventRecord(P.S->matched, R.st_join));
    P.d = d;
    P.p0 = p0;
    P.want = want;
    P.matched = true;
    return BG_OK;
}

// The band of sub-batch n, which starts at p0: launched on the device builder's stream, or built here by the host threads.
int band_build(BandRun& R, uint64_t p0, uint64_t n) {
    const BandCall& c = R.c;
    bg_band_scratch& B = R.B;
    BandPass& P = R.pass[n & 1];
    bg_band_scratch::Set& S = *P.S;
    int rc = BG_OK;
    if (R.build_on_device && !(P.matched && P.p0 == p0))
        if ((rc = band_join(R, p0, n))) return rc;
    const uint64_t want = band_want(R, p0);
    P.n = n;
    P.p0 = p0;
    P.want = want;
    P.hp.assign(want, HostPair());
    std::vector<uint64_t>& row0 = P.row0;
    row0.resize(want + 1);
    row0[0] = 0;
    for (uint64_t q = 0; q < want; q++) row0[q + 1] = row0[q] + (c.x_off[p0 + q + 1] - c.x_off[p0 + q]) + 1;
    // The set's staging and device buffers were last used two sub-batches ago — by K4 of sub-batch c - 2, which ends
    // ~14 ms after ITS fill.  Rounds 2-4 waited for that on the HOST, here, before launching anything of sub-batch c: the
    // chaining of c then started 5 ms into the fill of c - 1 it is meant to run under (profiles/
    // r05_banded_timeline_chain_rows.txt: chain_rows 68.85 behind K4's end at 68.79, the fill at 63.55), and the builder's
    // chain — not the fill — timed the cycle.  The chaining touches none of the set's buffers (the builder's own arrays are
    // double-buffered by parity and guarded by `built`): only the raster, which writes the set's row ranges, has to wait,
    // and it can do so on the device; the host waits in band_collect, before it writes the pinned staging.  (A buffer that
    // has to GROW is freed and allocated anew: then, and for host-built bands, the host waits here as before.)
    const size_t need_rc = std::max<size_t>(row0[want] * sizeof(int2), 64), need_ro = std::max<size_t>(row0[want] * 4, 64);
    const bool grows = S.hc_rowc < need_rc || S.hc_roff < need_ro || S.hc_pairs < want * sizeof(BandPair) || S.dc_rowc < need_rc ||
                       S.dc_roff < need_ro || B.h_state_cap < want * sizeof(BandDevPair);
    if ((grows || !R.build_on_device) && S.busy) {
        BG_HIP(hipEventSynchronize(S.traced));
        S.busy = false;
    }
    if ((rc = pinned_reserve(&S.h_rowc, &S.hc_rowc, need_rc))) return rc;
    if ((rc = pinned_reserve(&S.h_roff, &S.hc_roff, need_ro))) return rc;
    if ((rc = pinned_reserve(&S.h_pairs, &S.hc_pairs, want * sizeof(BandPair)))) return rc;
    if (R.build_on_device) {
        // ---- Band::create on the device (band_device.hip); the few pairs it hands back are built in band_collect.
        // The k-mer join is already on its way (band_join)
        BandDevArgs d = P.d;
        if ((rc = bg_reserve(&S.d_rowc, &S.dc_rowc, need_rc))) return rc;
        if ((rc = bg_reserve(&S.d_roff, &S.dc_roff, need_ro))) return rc;
        d.rowc = (int2*)S.d_rowc;
        d.row_off = (uint32_t*)S.d_roff;
        if ((rc = pinned_reserve(&B.h_state, &B.h_state_cap, want * sizeof(BandDevPair)))) return rc;
        BG_HIP(hipStreamWaitEvent(R.st_build, S.matched, 0));
        BG_HIP(hipMemcpyAsync((void*)d.row0, row0.data(), (want + 1) * 8, hipMemcpyHostToDevice, R.st_build));
        // The chaining of sub-batch c + 1 runs UNDER the fill of c: it mostly waits on memory and fits the registers
        // the fill leaves free — provided it starts after every block of the fill is resident
        // (launch_band_wait_started: the fill's grid is a single round of blocks, and a co-runner that is on a CU
        // first delays the whole kernel: fill 57 -> 116 ms).  The raster kernels start when that fill is done and
        // overlap K4 of sub-batch c.
        if (B.started_target) launch_band_wait_started(B.d_started, B.started_target, R.st_build);
        if ((rc = launch_band_chain(d, R.st_build, 2))) return rc;
        if (S.busy) BG_HIP(hipStreamWaitEvent(R.st_build, S.traced, 0));  // the raster writes the set's row ranges: K4 of c - 2 has read them
        if ((rc = launch_band_raster(d, R.st_build))) return rc;
        BG_HIP(hipMemcpyAsync(B.h_state, d.state, want * sizeof(BandDevPair), hipMemcpyDeviceToHost, R.st_build));
        BG_HIP(hipEventRecord(S.built, R.st_build));
        S.built_valid = true;
        // The builder's own arrays are free again: the join and the chain preparation of the NEXT sub-batch go right
        // behind, without waiting for the host to learn this one's sizes (band_stage used to issue them: 2 ms of round trip
        // on the builder's path, and they landed in the gap between two fills).  Speculative in one respect: the next
        // sub-batch starts at p0 + want only if the scratch budget takes all of this one — otherwise band_stage re-issues.
        if (p0 + want < c.n_pairs)
            if ((rc = band_join(R, p0 + want, n + 1))) return rc;
        return BG_OK;
    }
    int2* h_rowc = (int2*)S.h_rowc;
    uint32_t* h_roff = (uint32_t*)S.h_roff;
    std::atomic<bool> bad_input{false};
    parallel_for(want, R.grain, [&](unsigned, uint64_t lo, uint64_t hi) {
        bgband::Band band;
        bgband::Workspace ws;
        for (uint64_t q = lo; q < hi; q++) {
            const uint64_t p = p0 + q;
            const uint32_t m = (uint32_t)(c.x_off[p + 1] - c.x_off[p]), n_ = (uint32_t)(c.y_off[p + 1] - c.y_off[p]);
            if (!c.make_band(p, R.cs, band, ws) || band.start.size() != (size_t)n_ + 1) {
                bad_input = true;
                band.reset(m, n_);
            }
            build_pair(m, n_, band, P.hp[q], h_rowc + row0[q], h_roff + row0[q]);
        }
    });
    if (bad_input) return BG_ERR_INVALID_ARG;
    R.lap("band build");
    R.lap_cpu();
    return BG_OK;
}

// The host learns the sub-batch's bands: waits for the set (K4 of two sub-batches ago) and the device builder, builds the
// pairs that one handed back, and takes as many pairs as fit the scratch budget (the rest is rebuilt with the next
// sub-batch).  Writes the pair table into the set's pinned staging.
int band_collect(BandRun& R, BandPass& P) {
    const BandCall& c = R.c;
    bg_band_scratch::Set& S = *P.S;
    std::vector<HostPair>& hp = P.hp;
    const std::vector<uint64_t>& row0 = P.row0;
    const uint64_t p0 = P.p0, want = P.want;
    P.sp = R.use_pre ? R.B.aux_stream : R.st;  // (see BandRun::use_pre)
    if (S.busy) {  // (band_build left this wait to the device: the host writes the set's pinned staging from here on)
        BG_HIP(hipEventSynchronize(S.traced));
        S.busy = false;
    }
    if (R.build_on_device) {
        int2* h_rowc = (int2*)S.h_rowc;
        uint32_t* h_roff = (uint32_t*)S.h_roff;
        BG_HIP(hipEventSynchronize(S.built));
        R.lap("band build (device)");
        const BandDevPair* hs = (const BandDevPair*)R.B.h_state;
        std::vector<uint64_t> redo;
        for (uint64_t q = 0; q < want; q++) {
            HostPair& h = hp[q];
            h.m = (uint32_t)(c.x_off[p0 + q + 1] - c.x_off[p0 + q]);
            h.n = (uint32_t)(c.y_off[p0 + q + 1] - c.y_off[p0 + q]);
            h.flags = hs[q].flags;
            h.cells = hs[q].cells;
            h.tb_bytes = hs[q].tb_bytes;
            h.start_0 = hs[q].start_0;
            h.end_0 = hs[q].end_0;
            h.start_n = hs[q].start_n;
            h.end_n = hs[q].end_n;
            if (h.flags == BP_HOST_FALLBACK) redo.push_back(q);
        }
        if (!redo.empty()) {
            parallel_for(redo.size(), 1, [&](unsigned, uint64_t lo, uint64_t hi) {
                bgband::Band band;
                bgband::Workspace ws;
                for (uint64_t t = lo; t < hi; t++) {
                    const uint64_t q = redo[t];
                    c.make_band(p0 + q, R.cs, band, ws);
                    build_pair(hp[q].m, hp[q].n, band, hp[q], h_rowc + row0[q], h_roff + row0[q]);
                }
            });
            for (uint64_t q : redo) {
                const size_t nr = (size_t)hp[q].m + 1;
                BG_HIP(hipMemcpyAsync((int2*)S.d_rowc + row0[q], h_rowc + row0[q], nr * sizeof(int2), hipMemcpyHostToDevice, P.sp));
                BG_HIP(hipMemcpyAsync((uint32_t*)S.d_roff + row0[q], h_roff + row0[q], nr * 4, hipMemcpyHostToDevice, P.sp));
            }
            if (R.trace) fprintf(stderr, "[bg banded] %zu of %llu pairs rebuilt on the host\n", redo.size(), (unsigned long long)want);
        }
    }
    BandPair* dp = (BandPair*)S.h_pairs;
    uint64_t take = 0, tbb = 0, auxw = 0;
    for (; take < want; take++) {
        const HostPair& h = hp[take];
        const uint64_t t2 = tbb + h.tb_bytes, a2 = auxw + ((BandAux(h.m, h.n).words() + 3) & ~3ull);
        if (take > 0 && t2 + a2 * 4 > R.budget) break;
        BandPair& d = dp[take];
        d.rowc_off = row0[take];
        d.tb_off = tbb;
        d.aux_off = auxw;
        d.start_0 = h.start_0;
        d.end_0 = h.end_0;
        d.start_n = h.start_n;
        d.end_n = h.end_n;
        d.flags = h.flags;
        d._pad = 0;
        if (c.band_cells) c.band_cells[p0 + take] = h.cells;
        tbb = t2;
        auxw = a2;
    }
    P.take = take;
    P.tb_bytes = tbb;
    P.aux_words = auxw;
    return BG_OK;
}

// Everything the fill of the sub-batch waits for, on its preparation stream `sp`: the pair table (and a host-built band)
// goes up, the aux block is cleared, the sequences and the band are there.  Fills in the sub-batch's kernel arguments.
int band_stage(BandRun& R, BandPass& P) {
    bg_band_scratch& B = R.B;
    bg_band_scratch::Set& S = *P.S;
    hipStream_t sp = P.sp;
    const uint64_t p0 = P.p0, take = P.take, rows = P.row0[take];
    int rc = BG_OK;
    if ((rc = bg_reserve(&S.d_pairs, &S.dc_pairs, take * sizeof(BandPair)))) return rc;
    if ((rc = bg_reserve(&S.d_rowc, &S.dc_rowc, std::max<size_t>(rows * sizeof(int2), 64)))) return rc;
    if ((rc = bg_reserve(&S.d_roff, &S.dc_roff, std::max<size_t>(rows * 4, 64)))) return rc;
    if ((rc = bg_reserve(&S.d_tb, &S.dc_tb, std::max<size_t>(P.tb_bytes, 64)))) return rc;
    if ((rc = bg_reserve(&S.d_aux, &S.dc_aux, std::max<size_t>(P.aux_words * 4, 64)))) return rc;
    BG_HIP(hipMemcpyAsync(S.d_pairs, S.h_pairs, take * sizeof(BandPair), hipMemcpyHostToDevice, sp));
    if (!R.build_on_device) {
        BG_HIP(hipMemcpyAsync(S.d_rowc, S.h_rowc, rows * sizeof(int2), hipMemcpyHostToDevice, R.st));
        BG_HIP(hipMemcpyAsync(S.d_roff, S.h_roff, rows * 4, hipMemcpyHostToDevice, R.st));
    }
    BG_HIP(hipEventRecord(S.copied, sp));
    // the aux block is cleared on a stream of its own: 7 GB per sub-batch, 1.8 ms that used to sit between two fills
    // (the set's previous user, K4 of two sub-batches ago, is done: band_collect waited for it)
    BG_HIP(hipMemsetAsync(S.d_aux, 0, P.aux_words * 4, B.aux_stream));
    BG_HIP(hipEventRecord(S.cleared, B.aux_stream));
    BG_HIP(hipStreamWaitEvent(sp, S.cleared, 0));
    P.a = R.a;
    P.a.pairs = (const BandPair*)S.d_pairs;
    P.a.rowc = (const int2*)S.d_rowc;
    P.a.row_off = (const uint32_t*)S.d_roff;
    P.a.tb = (uint8_t*)S.d_tb;
    P.a.aux = (int32_t*)S.d_aux;
    P.a.pair0 = p0;
    P.a.n_pairs = (uint32_t)take;
    if ((rc = band_need_seq(R, sp, sp == R.st ? R.waited_fill : R.waited_pre, p0 + take))) return rc;
    if (R.build_on_device) BG_HIP(hipStreamWaitEvent(sp, S.built, 0));
    if (R.build_on_device && p0 + take < R.c.n_pairs) {  // the next sub-batch's k-mer join goes first (see band_join)
        const BandPass& N = R.pass[(P.n + 1) & 1];
        if (!(N.matched && N.p0 == p0 + take))
            if ((rc = band_join(R, p0 + take, P.n + 1))) return rc;
        // The fill does not wait for that join: with K3i / K3p on 32-byte rings (two blocks = 66 KB per CU) the join
        // (91 KB) and the chaining's preparation (16 KB per wavefront) fit NEXT to a fill, so fills run back to back
        // (round 3's 64-byte rings, 124 KB of LDS per block, left the join only a window between two fills).
    }
    return BG_OK;
}

// K3 / K3v2 on the caller's stream, whichever the call's plan names (plan_band_fill).
int band_fill(BandRun& R, BandPass& P) {
    bg_ctx* ctx = R.ctx;
    bg_band_scratch::Set& S = *P.S;
    hipStream_t st = R.st, sp = P.sp;
    const int rc = timed(ctx, st, ctx->ev, &ctx->last.fill_ms, &ctx->last.fill_launches, [&]() -> int {
        if (R.plan.v2) {
            if (R.build_on_device) R.B.started_target += band_fill2_blocks(P.a.n_pairs);
            // K3v2 / K3p (K3i): eight pairs per wavefront; the epilogue goes to the traceback stream, ahead of K4 — the fill
            // stream goes straight on with the next sub-batch (event timing keeps everything on one stream)
            ctx->fill_mask |= launch_band_fill2(P.a, R.plan.narrow, st, S.fill_gone, ctx->timing ? nullptr : R.st_tb, sp != st ? sp : nullptr, S.pre_done);
        } else {
            if (sp != st) {
                BG_HIP(hipEventRecord(S.pre_done, sp));
                BG_HIP(hipStreamWaitEvent(st, S.pre_done, 0));
            }
            R.fill<<<dim3((unsigned)((P.take + 3) / 4)), dim3(256), 0, st>>>(P.a);
            ctx->fill_mask |= BG_FILL_K3;
        }
        return BG_OK;
    });
    if (rc) return rc;
    BG_HIP(hipEventRecord(S.filled, st));
    return BG_OK;
}

// K4 on its own stream: it overlaps the next sub-batch's K3
int band_traceback(BandRun& R, BandPass& P) {
    bg_ctx* ctx = R.ctx;
    BG_HIP(hipStreamWaitEvent(R.st_tb, P.S->filled, 0));
    return timed(ctx, R.st_tb, ctx->ev, &ctx->last.traceback_ms, &ctx->last.traceback_launches, [&]() -> int {
        launch_band_traceback(P.a, R.st_tb);
        return BG_OK;
    });
}

// Behind K4 on the traceback stream.  Host-buffer call with operations: this sub-batch's operations go, compacted, behind
// those of the sub-batches before it (running byte count in B.d_cell) while the next fill runs; its records get their
// final ops_off; a few blocks on the download stream bring them to the pinned buffer.  Every call: `traced`, the set is busy.
int band_download(BandRun& R, BandPass& P) {
    bg_band_scratch& B = R.B;
    bg_band_scratch::Set& S = *P.S;
    int rc = BG_OK;
    uint64_t* dl = nullptr;
    if (R.compact_on_device) {
        if (P.n && P.n % bg_band_scratch::kDlSlots == 0) BG_HIP(hipStreamSynchronize(B.dl_stream));  // the ring comes round
        dl = B.d_dlslot + 2 * (P.n % bg_band_scratch::kDlSlots);
        if ((rc = bg_compact_ops_dev(R.a.out + P.p0, P.take, R.a.ops, (uint8_t*)B.d_cmp, true, B.d_cell, dl, B.d_cscan, true, R.st_tb))) return rc;
        BG_HIP(hipMemcpyAsync(dl + 1, B.d_cell, 8, hipMemcpyDeviceToDevice, R.st_tb));
    }
    BG_HIP(hipEventRecord(S.traced, R.st_tb));
    if (dl) {
        BG_HIP(hipStreamWaitEvent(B.dl_stream, S.traced, 0));
        if ((rc = bg_range_to_host((const uint8_t*)B.d_cmp, (uint8_t*)B.h_ops, dl, B.dl_stream))) return rc;
    }
    S.busy = true;
    R.lap("enqueue");
    return BG_OK;
}

// The tail of a call: waits for the streams; a host-buffer call gets its records and its operations, and the accounting of
// ops_cap: the status is BG_ERR_OPS_CAP where a pair's operations do not fit, *ops_used the full need either way.
int band_drain(BandRun& R) {
    const BandCall& c = R.c;
    bg_band_scratch& B = R.B;
    if (c.dev) {  // everything stays in HBM; records keep the strided ops_off like bg_align_batch_dev
        BG_HIP(hipStreamSynchronize(R.st_tb));
        BG_HIP(hipStreamSynchronize(R.st));
        for (auto& s : B.set) s.busy = false;
        R.lap("drain");
        return BG_OK;
    }
    // results: the records (their ops_off final) and the compact operations come back on the traceback stream
    bg_alignment_t* out = c.out;
    BG_HIP(hipMemcpyAsync(out, R.a.out, c.n_pairs * sizeof(bg_alignment_t), hipMemcpyDeviceToHost, R.st_tb));
    uint64_t used = 0;
    if (R.compact_on_device) BG_HIP(hipMemcpyAsync(&used, B.d_cell, 8, hipMemcpyDeviceToHost, R.st_tb));
    BG_HIP(hipStreamSynchronize(R.st_tb));
    BG_HIP(hipStreamSynchronize(R.st));
    for (auto& s : B.set) s.busy = false;
    // (the operations are in B.h_ops once the download stream has drained: synchronised below)
    int status = BG_OK;
    bool cap_hit = false;
    uint64_t fit = used;  // bytes of whole pairs that fit the caller's buffer
    for (uint64_t p = 0; p < c.n_pairs; p++) {  // (while the operations travel)
        if (out[p].status && status == BG_OK) status = out[p].status;
        if (!R.compact_on_device) {  // no operations wanted: offsets of an (empty) compact buffer all the same
            out[p].ops_off = used;
            used += out[p].n_ops;
        } else if (!cap_hit && out[p].ops_off + out[p].n_ops > c.ops_cap) {
            cap_hit = true;
            fit = out[p].ops_off;
        }
    }
    if (cap_hit && status == BG_OK) status = BG_ERR_OPS_CAP;
    if (R.compact_on_device && used) {
        BG_HIP(hipStreamSynchronize(B.dl_stream));
        R.lap("drain + d2h");
        const uint8_t* h_ops = (const uint8_t*)B.h_ops;
        const uint64_t nb = std::min(fit, c.ops_cap);
        parallel_for(nb, 1 << 20, [&](unsigned, uint64_t lo, uint64_t hi) { memcpy(c.ops + lo, h_ops + lo, hi - lo); });
    }
    if (c.ops_used) *c.ops_used = used;
    R.lap("compact ops");
    return status;
}

// The banded pipeline over one call.  Streams: st (the caller's: fills), tb (K4, compaction), build (device builder),
// join = copy (low priority: sequence slices, k-mer joins), aux (high priority: aux clears, fill preparation), dl
// (high priority: operations to the pinned buffer); sp is aux for a device-built, untimed call (use_pre) and st otherwise.
// Sub-batch c uses set c & 1 and the builder's arrays c & 1.  Who records each event, and who waits for it:
//   seq_ready    st, once per call (offsets uploaded, d_started zeroed)       build, join: before their first work
//   slice ev[0]  st, before the first slice goes up                           copy: host-buffer sequences go behind the offsets
//   slice ev[k+1] copy, behind slice k                                        st / join / sp: before a sub-batch that reads
//                                                                             pairs of slice k (band_need_seq, one cursor each)
//   matched      join, behind join + chain preparation of c (band_join)       build: before the chaining of c
//   built        build, behind raster + state read-back of c (band_build)     host: band_collect(c); sp: before fill c;
//                                                                             join: before join c + 2 (the builder's arrays)
//   traced       tb, behind K4 and the compaction of c (band_download)        host: band_collect(c + 2), or band_build(c + 2)
//                                                                             where a buffer grows or the host builds;
//                                                                             build: before raster c + 2; dl: before its copy
//   copied       sp, behind the pair table's upload (band_stage)              nobody waits for it
//   cleared      aux, behind the aux block's clear (band_stage)               sp: before fill c
//   pre_done     sp, behind the preparation (band_fill: K3 here, K3v2 in      st: before fill c (only where sp != st)
//                launch_band_fill2 behind its phase 1)
//   fill_gone    st, inside launch_band_fill2 behind the fill kernel          tb: the epilogue of c goes there (untimed calls)
//   filled       st, behind fill c (band_fill)                                tb: before K4 of c
// The host waits: for `traced` and `built` as above, for the dl ring every kDlSlots sub-batches, under event timing for
// each timed span, and in band_drain for tb, st and (operations wanted) dl.
int band_run(const BandCall& c) {
    bg_ctx* ctx = c.ctx;
    const uint64_t n_pairs = c.n_pairs;
    if (!ctx || !c.sc || c.mode < BG_MODE_CUSTOM || c.mode > BG_MODE_LOCAL) return BG_ERR_INVALID_ARG;
    ctx->fill_mask = 0;
    ctx->fill_framed = false;
    ctx->fill_max3 = false;
    int rc = check_scoring(c.sc);
    if (rc) return rc;
    if (c.ops_used) *c.ops_used = 0;
    if (n_pairs == 0) return BG_OK;
    if (!c.x_off || !c.y_off || !c.out) return BG_ERR_INVALID_ARG;
    BG_HIP(hipSetDevice(ctx->device));
    const bool compact_on_device = !c.dev && c.ops != nullptr;
    if ((rc = band_scratch_init(ctx, compact_on_device))) return rc;
    BandRun R(c, *ctx->band);
    bg_band_scratch& B = R.B;
    hipStream_t st = R.st = ctx->stream;
    R.st_tb = B.tb_stream;
    R.st_build = B.build_stream;
    R.st_join = B.copy_stream;
    R.compact_on_device = compact_on_device;
    R.cs = clip_scores(c.sc, c.mode);
    const bgband::ClipScores& cs = R.cs;
    for (uint64_t p = 0; p < n_pairs; p++) {
        R.max_x = std::max(R.max_x, c.x_off[p + 1] - c.x_off[p]);
        R.max_y = std::max(R.max_y, c.y_off[p + 1] - c.y_off[p]);
    }
    const uint64_t max_x = R.max_x, max_y = R.max_y;
    if (max_x > (1u << 24) || max_y > (1u << 24)) return BG_ERR_TOO_LARGE;
    const uint64_t stride = c.dev ? c.ops_stride : ((max_x + max_y + 4 + 3) & ~3ull);
    if (c.dev && c.ops && stride < max_x + max_y + 4) return BG_ERR_OPS_CAP;

    BandArgs& a = R.a;
    a.sc = {cs.gap_open, cs.gap_extend, cs.xclip_prefix, cs.xclip_suffix, cs.yclip_prefix, cs.yclip_suffix,
            c.sc->match_score, c.sc->mismatch_score};
    a.mode = c.mode;
    a.filter_clips = (c.mode == BG_MODE_SEMIGLOBAL || c.mode == BG_MODE_LOCAL);
    a.ops_stride = stride;
    if (c.sc->matrix) {  // (the tabulated match function is compacted exactly like in sw_api.hip)
        std::vector<uint8_t> code_map;
        std::vector<int32_t> table;
        a.alpha = bg_compact_matrix(c.sc->matrix, code_map, table);
        if ((rc = bg_reserve(&ctx->table, &ctx->table_bytes, 256 + table.size() * 4))) return rc;
        BG_HIP(hipMemcpy((uint8_t*)ctx->table + 256, table.data(), table.size() * 4, hipMemcpyHostToDevice));
        BG_HIP(hipMemcpy(ctx->table, code_map.data(), 256, hipMemcpyHostToDevice));
        a.code_map = (const uint8_t*)ctx->table;
        a.table = (const int32_t*)((uint8_t*)ctx->table + 256);
    }
    R.build_on_device = c.has_kw && !ctx->band_on_host;
    R.use_pre = R.build_on_device && !ctx->timing;
    R.plan = plan_band_fill(a.sc, a.alpha, max_x, max_y, ctx, n_pairs);
    R.fill = get_band_fill(R.plan.sm);
    a.split = R.plan.split;
    a.packed = R.plan.packed;
    a.pk_thresh = R.plan.pk_thresh;
    if (R.plan.v2) {
        a.tb_flip = kTbFlip;
        a.started = R.build_on_device ? B.d_started : nullptr;
        a.redo_count = B.d_started + 1;
    }

    R.trace = getenv("BG_TRACE") != nullptr;
    R.t_last = std::chrono::steady_clock::now();

    // sequences and result records of the whole batch live on the device; band data goes in sub-batches
    const uint64_t xb = c.x_off[n_pairs], yb = c.y_off[n_pairs];
    if (c.dev) {
        a.x = c.x;
        a.y = c.y;
        a.x_off = c.d_x_off;
        a.y_off = c.d_y_off;
        a.out = c.out;
        a.ops = c.ops;
    } else {
        size_t io_need[kBandIoBufs];
        io_need[kIoX] = std::max<uint64_t>(xb, 16);
        io_need[kIoY] = std::max<uint64_t>(yb, 16);
        io_need[kIoXOff] = io_need[kIoYOff] = (n_pairs + 1) * 8;
        io_need[kIoOut] = n_pairs * sizeof(bg_alignment_t);
        io_need[kIoOps] = c.ops ? n_pairs * stride : 16;
        for (int i = 0; i < kBandIoBufs; i++)
            if ((rc = bg_reserve(&B.io[i], &B.io_cap[i], io_need[i]))) return rc;
        a.x = (const uint8_t*)B.io[kIoX];
        a.y = (const uint8_t*)B.io[kIoY];
        a.x_off = (const uint64_t*)B.io[kIoXOff];
        a.y_off = (const uint64_t*)B.io[kIoYOff];
        a.out = (bg_alignment_t*)B.io[kIoOut];
        a.ops = c.ops ? (uint8_t*)B.io[kIoOps] : nullptr;
        BG_HIP(hipMemcpyAsync(B.io[kIoXOff], c.x_off, (n_pairs + 1) * 8, hipMemcpyHostToDevice, st));
        BG_HIP(hipMemcpyAsync(B.io[kIoYOff], c.y_off, (n_pairs + 1) * 8, hipMemcpyHostToDevice, st));
        // (the sequences follow in slices: band_upload_slices)
    }
    R.lap("h2d sequences");
    R.chunk_pairs = ctx->chunk_pairs > 0 ? (uint64_t)ctx->chunk_pairs : 16384;
    // host-buffer flavour with operations: they are compacted on the device, sub-batch by sub-batch (an operation list
    // is at most m + n + 4 bytes)
    if (compact_on_device) {
        if ((rc = bg_reserve(&B.d_cmp, &B.d_cmp_cap, xb + yb + 4 * n_pairs + 256))) return rc;
        if ((rc = bg_reserve(&B.d_cscan, &B.d_cscan_cap, bg_compact_ops_scratch(std::min<uint64_t>(n_pairs, R.chunk_pairs))))) return rc;
        BG_HIP(hipMemsetAsync(B.d_cell, 0, 8, st));  // st_tb waits for st's events before every traceback
        // the operations of a sub-batch leave for the pinned buffer as soon as they are compacted, while the next ones are
        // computed (one download of everything after the last sub-batch was 20 ms of a 490 ms call, with the device idle)
        if ((rc = pinned_reserve(&B.h_ops, &B.h_ops_cap, xb + yb + 4 * n_pairs + 256))) return rc;
    }

    R.n_slices = c.dev ? 0 : (n_pairs + R.chunk_pairs - 1) / R.chunk_pairs;
    if ((rc = band_need_seq(R, st, R.waited_fill, std::min<uint64_t>(n_pairs, R.chunk_pairs)))) return rc;  // the first slice
    // traceback + aux per scratch set (two sets): 40 GB each on an otherwise empty 288 GB part — but no more than a third of
    // what the device has free now plus what the sets already hold (a smaller or shared GPU, a torch caching allocator next
    // to the engine): a smaller budget cuts the sub-batches (`take < want` in band_collect) instead of failing bg_reserve with OOM
    R.budget = (ctx->band_budget_gb > 0 ? (uint64_t)ctx->band_budget_gb : 40ull) << 30;
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            uint64_t held = 0;
            for (auto& s : B.set) held += s.dc_tb + s.dc_aux;
            R.budget = std::min<uint64_t>(R.budget, std::max<uint64_t>(((uint64_t)free_b + held) / 3, 1ull << 30));
        }
    }
    R.grain = std::max<uint64_t>(1, std::min<uint64_t>(64, 65536 / (max_x + max_y + 1)));
    R.first_want = (n_pairs > R.chunk_pairs && n_pairs % R.chunk_pairs) ? n_pairs % R.chunk_pairs : 0;
    for (unsigned i = 0; i < 2; i++) {
        R.pass[i].parity = i;
        R.pass[i].S = &B.set[i];
        B.set[i].built_valid = false;
    }
    BG_HIP(hipMemsetAsync(B.d_started, 0, 8, st));  // [0] blocks started, [1] pairs K3p flagged
    B.started_target = 0;
    BG_HIP(hipEventRecord(B.seq_ready, st));
    BG_HIP(hipStreamWaitEvent(R.st_build, B.seq_ready, 0));
    BG_HIP(hipStreamWaitEvent(R.st_join, B.seq_ready, 0));

    // The schedule: sub-batch n + 1's band is launched (or built) right behind the kernels of sub-batch n.
    uint64_t p0 = 0, n = 0;
    if ((rc = band_build(R, 0, 0))) return rc;
    // The caller's buffers are pageable: an upload keeps this thread inside the copy call for its whole duration
    // (~30 ms per slice), and the device idle if the next launches wait behind it.  So slice c + 2 goes up right
    // after the fill of sub-batch c has been launched (44 ms of kernels to hide behind), one slice per round — not
    // all of them after the first band_build (measured: the first round took 90 ms instead of 58).
    if ((rc = band_upload_slices(R, 2))) return rc;
    for (;;) {
        BandPass& P = R.pass[n & 1];
        if ((rc = band_collect(R, P))) return rc;
        if ((rc = band_stage(R, P))) return rc;
        if ((rc = band_fill(R, P))) return rc;
        if ((rc = band_traceback(R, P))) return rc;
        if ((rc = band_download(R, P))) return rc;
        p0 += P.take;
        if (p0 >= n_pairs) break;
        if ((rc = band_upload_slices(R, n + 3))) return rc;
        n++;
        if ((rc = band_build(R, p0, n))) return rc;
    }
    return band_drain(R);
}

}  // namespace

extern "C" int bg_align_banded_batch(bg_ctx* ctx, const bg_scoring_t* sc, int mode, uint32_t k, uint32_t w,
                                     uint64_t n_pairs, const uint8_t* x, const uint64_t* x_off, const uint8_t* y,
                                     const uint64_t* y_off, bg_alignment_t* out, uint8_t* ops_buf, uint64_t ops_cap,
                                     uint64_t* ops_used, uint64_t* band_cells) {
    BandCall c;
    c.ctx = ctx, c.sc = sc, c.mode = mode, c.n_pairs = n_pairs;
    c.x = x, c.x_off = x_off, c.y = y, c.y_off = y_off;
    c.out = out, c.ops = ops_buf, c.ops_cap = ops_cap, c.ops_used = ops_used, c.band_cells = band_cells;
    c.has_kw = true, c.k = k, c.w = w;
    c.make_band = [&](uint64_t p, const bgband::ClipScores& cs, bgband::Band& band, bgband::Workspace& ws) {
        band.create(x + x_off[p], (size_t)(x_off[p + 1] - x_off[p]), y + y_off[p], (size_t)(y_off[p + 1] - y_off[p]), k, w, cs, ws);
        return true;
    };
    return band_run(c);
}

// Device-resident flavour of bg_align_banded_batch: sequences, offsets, records and operation slots are
// device pointers (records keep ops_off = (p + 1) * ops_stride - n_ops, operations right-aligned in their
// slot, as bg_align_batch_dev leaves them).  Synchronous: it drives its own streams and returns when
// the results are in place; work queued on `stream` before the call is waited for first.
extern "C" int bg_align_banded_batch_dev(bg_ctx* ctx, const bg_scoring_t* sc, int mode, uint32_t k, uint32_t w,
                                         uint64_t n_pairs, const uint8_t* d_x, const uint64_t* d_x_off, const uint8_t* d_y,
                                         const uint64_t* d_y_off, bg_alignment_t* d_out, uint8_t* d_ops, uint64_t ops_stride,
                                         uint64_t* band_cells, void* stream) {
    if (!ctx || !sc || mode < BG_MODE_CUSTOM || mode > BG_MODE_LOCAL) return BG_ERR_INVALID_ARG;
    if (n_pairs == 0) return BG_OK;
    if (!d_x_off || !d_y_off || !d_out) return BG_ERR_INVALID_ARG;
    BG_HIP(hipSetDevice(ctx->device));
    BG_HIP(hipStreamSynchronize((hipStream_t)stream));
    // the host side of the pipeline needs the lengths
    std::vector<uint64_t> x_off(n_pairs + 1), y_off(n_pairs + 1);
    BG_HIP(hipMemcpy(x_off.data(), d_x_off, (n_pairs + 1) * 8, hipMemcpyDeviceToHost));
    BG_HIP(hipMemcpy(y_off.data(), d_y_off, (n_pairs + 1) * 8, hipMemcpyDeviceToHost));
    BandCall c;
    c.ctx = ctx, c.sc = sc, c.mode = mode, c.n_pairs = n_pairs;
    c.x_off = x_off.data(), c.y_off = y_off.data();
    c.dev = true, c.x = d_x, c.y = d_y, c.d_x_off = d_x_off, c.d_y_off = d_y_off;
    c.out = d_out, c.ops = d_ops, c.ops_stride = ops_stride, c.band_cells = band_cells;
    c.has_kw = true, c.k = k, c.w = w;
    c.make_band = [&](uint64_t p, const bgband::ClipScores& cs, bgband::Band& band, bgband::Workspace& ws) {
        // a pair the device builder hands back: fetch its sequences for the host builder
        const size_t m = (size_t)(x_off[p + 1] - x_off[p]), n = (size_t)(y_off[p + 1] - y_off[p]);
        std::vector<uint8_t> hx(m + 1), hy(n + 1);
        if (m && hipMemcpy(hx.data(), d_x + x_off[p], m, hipMemcpyDeviceToHost) != hipSuccess) return false;
        if (n && hipMemcpy(hy.data(), d_y + y_off[p], n, hipMemcpyDeviceToHost) != hipSuccess) return false;
        band.create(hx.data(), m, hy.data(), n, k, w, cs, ws);
        return true;
    };
    return band_run(c);
}

// compute_alignment (banded.rs:406-869) over caller-supplied bands: n + 1 half-open row ranges per pair at
// band_off[p] — what custom_with_matches / custom_with_match_path / custom_with_expanded_matches /
// *_with_prehash (banded.rs:294-401, 938-970) reach after building their band on the host.
extern "C" int bg_align_banded_bands_batch(bg_ctx* ctx, const bg_scoring_t* sc, int mode, uint64_t n_pairs, const uint8_t* x,
                                           const uint64_t* x_off, const uint8_t* y, const uint64_t* y_off,
                                           const uint64_t* band_off, const uint32_t* band_start, const uint32_t* band_end,
                                           bg_alignment_t* out, uint8_t* ops_buf, uint64_t ops_cap, uint64_t* ops_used,
                                           uint64_t* band_cells) {
    if (n_pairs && (!band_off || !band_start || !band_end)) return BG_ERR_INVALID_ARG;
    BandCall c;
    c.ctx = ctx, c.sc = sc, c.mode = mode, c.n_pairs = n_pairs;
    c.x = x, c.x_off = x_off, c.y = y, c.y_off = y_off;
    c.out = out, c.ops = ops_buf, c.ops_cap = ops_cap, c.ops_used = ops_used, c.band_cells = band_cells;
    c.make_band = [&](uint64_t p, const bgband::ClipScores&, bgband::Band& band, bgband::Workspace&) {
        const size_t m = (size_t)(x_off[p + 1] - x_off[p]), n = (size_t)(y_off[p + 1] - y_off[p]);
        band.reset(m, n);
        for (size_t j = 0; j <= n; j++) {
            band.start[j] = band_start[band_off[p] + j];
            band.end[j] = band_end[band_off[p] + j];
            if (band.end[j] > m + 1 && band.end[j] > band.start[j]) return false;
        }
        return true;
    };
    return band_run(c);
}

namespace {
std::vector<bgband::Match> to_matches(const uint32_t* xy, uint64_t n) {
    std::vector<bgband::Match> v(n);
    for (uint64_t i = 0; i < n; i++) v[i] = {xy[2 * i], xy[2 * i + 1]};
    return v;
}
}  // namespace

// Band::create_with_matches (banded.rs:1301-1328; path == NULL) or Band::create_from_match_path
// (1330-1367) for a batch; matches of pair p are matches_xy[2*match_off[p] .. 2*match_off[p+1]).
extern "C" int bg_band_from_matches_batch(const bg_scoring_t* sc, int mode, uint32_t k, uint32_t w, uint64_t n_pairs,
                                          const uint64_t* x_off, const uint64_t* y_off, const uint32_t* matches_xy,
                                          const uint64_t* match_off, const uint32_t* path, const uint64_t* path_off,
                                          const uint64_t* band_off, uint32_t* start, uint32_t* end, uint64_t* band_cells) {
    if (!sc || !x_off || !y_off || !match_off || (n_pairs && (!band_off || !start || !end))) return BG_ERR_INVALID_ARG;
    if (path && !path_off) return BG_ERR_INVALID_ARG;
    int rc = check_scoring(sc);
    if (rc) return rc;
    const bgband::ClipScores cs = clip_scores(sc, mode);
    std::atomic<bool> bad{false};
    parallel_for(n_pairs, 4, [&](unsigned, uint64_t lo, uint64_t hi) {
        bgband::Band band;
        bgband::Workspace ws;
        for (uint64_t p = lo; p < hi; p++) {
            const uint32_t m = (uint32_t)(x_off[p + 1] - x_off[p]), n = (uint32_t)(y_off[p + 1] - y_off[p]);
            const std::vector<bgband::Match> mm = to_matches(matches_xy + 2 * match_off[p], match_off[p + 1] - match_off[p]);
            bool ok = true;
            if (path) {
                std::vector<uint32_t> pp(path + path_off[p], path + path_off[p + 1]);
                for (uint32_t idx : pp) ok = ok && idx < mm.size();
                if (!mm.empty() && pp.empty()) ok = false;  // path[0] panics in the reference
                if (ok) band.create_from_match_path(m, n, k, w, cs, pp, mm);
            } else {
                ok = band.create_with_matches(m, n, k, w, cs, mm, ws);
            }
            if (!ok) {
                bad = true;
                continue;
            }
            memcpy(start + band_off[p], band.start.data(), (size_t)(n + 1) * 4);
            memcpy(end + band_off[p], band.end.data(), (size_t)(n + 1) * 4);
            if (band_cells) band_cells[p] = band.num_cells();
        }
    });
    return bad ? BG_ERR_INVALID_ARG : BG_OK;
}

// ---- sparse.rs helpers on the host (callers of custom_with_matches / _expanded_matches need them) ----
// All take matches as (x, y) uint32 pairs; return the number of entries the result has (which may exceed
// `cap`: call again with a larger buffer), or UINT64_MAX when the reference would assert (unsorted matches).
extern "C" uint64_t bg_sparse_find_kmer_matches(const uint8_t* x, uint64_t m, const uint8_t* y, uint64_t n, uint32_t k,
                                                uint32_t* out_xy, uint64_t cap) {
    std::vector<bgband::Match> mm;
    bgband::find_kmer_matches(x, m, y, n, k, mm);
    for (uint64_t i = 0; i < mm.size() && i < cap; i++) {
        out_xy[2 * i] = mm[i].x;
        out_xy[2 * i + 1] = mm[i].y;
    }
    return mm.size();
}

extern "C" uint64_t bg_sparse_sdpkpp(const uint32_t* matches_xy, uint64_t n_matches, uint32_t k, uint32_t match_score,
                                     int32_t gap_open, int32_t gap_extend, uint32_t* path, uint64_t cap) {
    std::vector<uint32_t> pp;
    const auto mm = to_matches(matches_xy, n_matches);
    for (size_t i = 1; i < mm.size(); i++)
        if (!(mm[i - 1] < mm[i])) return UINT64_MAX;
    if (!bgband::sdpkpp_path(mm, k, match_score, gap_open, gap_extend, pp)) return UINT64_MAX;
    for (uint64_t i = 0; i < pp.size() && i < cap; i++) path[i] = pp[i];
    return pp.size();
}

extern "C" uint64_t bg_sparse_lcskpp(const uint32_t* matches_xy, uint64_t n_matches, uint32_t k, uint32_t* path, uint64_t cap,
                                     uint32_t* score) {
    std::vector<uint32_t> pp;
    if (!bgband::lcskpp_path(to_matches(matches_xy, n_matches), k, pp, score)) return UINT64_MAX;
    for (uint64_t i = 0; i < pp.size() && i < cap; i++) path[i] = pp[i];
    return pp.size();
}

extern "C" uint64_t bg_sparse_sdpkpp_union_lcskpp_path(const uint32_t* matches_xy, uint64_t n_matches, uint32_t k,
                                                       uint32_t match_score, int32_t gap_open, int32_t gap_extend,
                                                       uint32_t* path, uint64_t cap) {
    std::vector<uint32_t> pp;
    if (!bgband::sdpkpp_union_lcskpp_path(to_matches(matches_xy, n_matches), k, match_score, gap_open, gap_extend, pp))
        return UINT64_MAX;
    for (uint64_t i = 0; i < pp.size() && i < cap; i++) path[i] = pp[i];
    return pp.size();
}

extern "C" uint64_t bg_sparse_expand_kmer_matches(const uint8_t* x, uint64_t m, const uint8_t* y, uint64_t n, uint32_t k,
                                                  const uint32_t* matches_xy, uint64_t n_matches, uint32_t allowed_mismatches,
                                                  uint32_t* out_xy, uint64_t cap) {
    std::vector<bgband::Match> out;
    if (!bgband::expand_kmer_matches(x, m, y, n, k, to_matches(matches_xy, n_matches), allowed_mismatches, out)) return UINT64_MAX;
    for (uint64_t i = 0; i < out.size() && i < cap; i++) {
        out_xy[2 * i] = out[i].x;
        out_xy[2 * i + 1] = out[i].y;
    }
    return out.size();
}
