// Stand-alone CPU program for tests/test_bgzf_inflate_host_bodies.py and the GPU tests of bg_bgzf_inflate: the __host__
// __device__ bodies of csrc/bgzf_inflate_rule.h run on the host.  A file is walked member by member with bgzf_member_verdict
// (what the kernels of csrc/bgzf_inflate.hip flag candidates and name the chain's error with); a block is inflated by inf_block,
// which runs lanes 0 .. 63 in turn wherever bgzf_inflate_kernel has a barrier.  The first test builds it with
// -fsanitize=address,undefined, the GPU tests without, for the statuses the GPU must give.
// Every array of the working set is a heap allocation of its own at exactly the size bgzf_inflate_rule.h states, and every
// block's member and output range are exact-size heap allocations of their own, so a lane that reads or writes one byte
// outside any of them stops the program.
// Input: uint64 files, uint64 members; per file uint64 length and the bytes; per member uint64 length, uint64 output range and
// the bytes.
// Output: per file int64 status of the walk, uint64 n_blocks, out_bytes, first_bad; if the status is 0: n_blocks + 1 rows of
// (block_off, out_off), a status byte a block, uint64 the lowest bad block (UINT64_MAX: none), the out_bytes payload bytes (a bad
// block's range as the bodies left it, from zeros).  Per member: uint32 status and its output range.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rust-bio_amd/csrc/bgzf_inflate_rule.h"

template <typename T>
static T* make(size_t count) {
    return (T*)calloc(count ? count : 1, sizeof(T));
}
template <typename T>
static T* load(FILE* f, size_t count) {
    T* p = (T*)malloc(count * sizeof(T) ? count * sizeof(T) : 1);
    if (count && fread(p, sizeof(T), count, f) != count) exit(2);
    return p;
}

static inf_ws_t ws;
// member[0 .. size) into a fresh range of isize bytes; the member is copied to an exact-size allocation first
static uint32_t one_block(const uint8_t* member, uint32_t size, uint32_t isize, uint8_t** out) {
    uint8_t* m = (uint8_t*)malloc(size);
    memcpy(m, member, size);
    *out = make<uint8_t>(isize);
    const uint32_t st = inf_block(ws, m, size, *out, isize);
    free(m);
    return st;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint64_t* hd = load<uint64_t>(f, 2);
    const uint64_t n_files = hd[0], n_members = hd[1];
    ws.lit = make<uint16_t>(1u << INF_LROOT);
    ws.dst = make<uint16_t>(1u << INF_DROOT);
    ws.sorted = make<uint16_t>(INF_NLIT + INF_NDIST);
    ws.meta = make<uint16_t>(96);
    ws.lens = make<uint8_t>(INF_NLIT + INF_NDIST);
    ws.clens = make<uint8_t>(INF_NCODE);
    ws.q = make<uint32_t>(2 * INF_QUEUE);
    ws.T = make<uint32_t>(1024);
    ws.part = make<uint32_t>(INF_LANES);
    ws.word = make<uint32_t>(1);

    for (uint64_t k = 0; k < n_files; k++) {
        uint64_t* d = load<uint64_t>(f, 1);
        const uint64_t len = d[0];
        uint8_t* in = load<uint8_t>(f, len);
        std::vector<uint64_t> rows;  // block_off, out_off
        uint64_t at = 0, bytes = 0;
        int64_t rc = BG_OK;
        while (at < len) {
            uint32_t size, isize;
            if ((rc = bgzf_member_verdict(in, len, at, &size, &isize))) break;
            rows.push_back(at);
            rows.push_back(bytes);
            at += size;
            bytes += isize;
        }
        const uint64_t n = rows.size() / 2, head[3] = {n, bytes, rc ? n : UINT64_MAX};
        fwrite(&rc, 8, 1, o);
        fwrite(head, 8, 3, o);
        if (!rc) {
            rows.push_back(len);
            rows.push_back(bytes);
            fwrite(rows.data(), 8, rows.size(), o);
            uint8_t* status = make<uint8_t>(n);
            uint8_t* payload = make<uint8_t>(bytes);
            uint64_t first_bad = UINT64_MAX;
            for (uint64_t b = 0; b < n; b++) {
                uint8_t* out;
                const uint32_t isize = (uint32_t)(rows[2 * b + 3] - rows[2 * b + 1]);
                status[b] = (uint8_t)one_block(in + rows[2 * b], (uint32_t)(rows[2 * b + 2] - rows[2 * b]), isize, &out);
                memcpy(payload + rows[2 * b + 1], out, isize);
                if (status[b] && first_bad == UINT64_MAX) first_bad = b;
                free(out);
            }
            fwrite(status, 1, n, o);
            fwrite(&first_bad, 8, 1, o);
            fwrite(payload, 1, bytes, o);
            free(payload);
            free(status);
        }
        free(in);
        free(d);
    }
    for (uint64_t k = 0; k < n_members; k++) {
        uint64_t* d = load<uint64_t>(f, 2);
        const uint32_t size = (uint32_t)d[0], isize = (uint32_t)d[1];
        if (size < BGZF_MIN_MEMBER || isize > BGZF_MAX_ISIZE) return 2;
        uint8_t* m = load<uint8_t>(f, size);
        uint8_t* out;
        const uint32_t st = one_block(m, size, isize, &out);
        fwrite(&st, 4, 1, o);
        fwrite(out, 1, isize, o);
        free(out);
        free(m);
        free(d);
    }
    free(ws.word);
    free(ws.part);
    free(ws.T);
    free(ws.q);
    free(ws.clens);
    free(ws.lens);
    free(ws.meta);
    free(ws.sorted);
    free(ws.dst);
    free(ws.lit);
    free(hd);
    fclose(o);
    fclose(f);
    return 0;
}
