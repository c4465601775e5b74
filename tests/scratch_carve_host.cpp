// bg_carve (csrc/bg_carve.h) on the CPU, built with AddressSanitizer and UBSan: lists of pieces of 0, 1, 255, 256 and 257
// elements of 1-, 4-, 8- and 40-byte types, empty pieces first, last and next to each other.  A list is measured, exactly that
// many bytes are allocated, the list is bound to them and every piece is filled to its last byte: a total that is too small
// stops the program.  tests/test_scratch_carve_host.py builds and runs this.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bg_carve.h"

namespace {

struct S40 {
    uint8_t b[40];
};
struct Piece {
    int type;  // 0: uint8_t, 1: uint32_t, 2: uint64_t, 3: S40
    size_t n;
};
const size_t kSize[4] = {1, 4, 8, 40};
const size_t kCounts[5] = {0, 1, 255, 256, 257};

int failures = 0;
#define CHECK(cond, ...)                             \
    do {                                             \
        if (!(cond)) {                               \
            printf("FAILED %s: ", #cond);            \
            printf(__VA_ARGS__);                     \
            printf("\n");                            \
            failures++;                              \
        }                                            \
    } while (0)

// the list: one take<T>(n) a piece, as a call site writes it
std::vector<uint8_t*> run(bg_carve& cv, const std::vector<Piece>& list) {
    std::vector<uint8_t*> p;
    for (const Piece& x : list) {
        if (x.type == 0) p.push_back(cv.take<uint8_t>(x.n));
        if (x.type == 1) p.push_back((uint8_t*)cv.take<uint32_t>(x.n));
        if (x.type == 2) p.push_back((uint8_t*)cv.take<uint64_t>(x.n));
        if (x.type == 3) p.push_back((uint8_t*)cv.take<S40>(x.n));
    }
    return p;
}

void check(const char* name, const std::vector<Piece>& list) {
    bg_carve measure;
    for (uint8_t* p : run(measure, list)) CHECK(p == nullptr, "%s: measuring returned a pointer", name);
    const size_t total = measure.at;
    CHECK((total == 0) == list.empty(), "%s: total %zu", name, total);
    if (list.empty()) return;
    uint8_t* base = (uint8_t*)malloc(total);  // exactly the measured bytes: ASan guards both ends
    bg_carve bound{base};
    const std::vector<uint8_t*> p = run(bound, list);
    CHECK(bound.at == total, "%s: measured %zu, bound run ends at %zu", name, total, bound.at);
    std::vector<std::pair<size_t, size_t>> range;  // [begin, end) from the base; an empty piece counts as its one address
    for (size_t i = 0; i < list.size(); i++) {
        const size_t bytes = list[i].n * kSize[list[i].type];
        CHECK(p[i] >= base && p[i] < base + total, "%s: piece %zu starts outside the reservation", name, i);
        const size_t o = (size_t)(p[i] - base);
        CHECK(o % 256 == 0, "%s: piece %zu starts at %zu", name, i, o);
        CHECK(o + bytes <= total, "%s: piece %zu ends at %zu of %zu", name, i, o + bytes, total);
        range.push_back({o, o + std::max<size_t>(bytes, 1)});
        memset(p[i], (int)(0x21 + i), bytes);
    }
    std::sort(range.begin(), range.end());
    for (size_t i = 1; i < range.size(); i++) CHECK(range[i - 1].second <= range[i].first, "%s: pieces overlap at %zu", name, range[i].first);
    for (size_t i = 0; i < list.size(); i++) {
        const size_t bytes = list[i].n * kSize[list[i].type];
        for (size_t k = 0; k < bytes; k++)
            if (p[i][k] != (uint8_t)(0x21 + i)) {
                CHECK(false, "%s: piece %zu lost byte %zu to another piece", name, i, k);
                break;
            }
    }
    free(base);
}

}  // namespace

int main() {
    std::vector<Piece> all, rev;
    for (int t = 0; t < 4; t++)
        for (size_t n : kCounts) all.push_back({t, n});
    rev.assign(all.rbegin(), all.rend());
    check("every size of every type", all);  // (begins with an empty piece)
    check("... in reverse", rev);            // (ends with one)
    check("no piece", {});
    check("one empty piece", {{2, 0}});
    check("empty pieces only", {{0, 0}, {1, 0}, {2, 0}, {3, 0}});
    check("empty first", {{2, 0}, {1, 257}, {0, 1}});
    check("empty last", {{3, 255}, {0, 256}, {1, 0}});
    check("empty neighbours", {{2, 1}, {0, 0}, {3, 0}, {1, 0}, {0, 257}, {2, 0}, {2, 0}});
    check("empty at both ends", {{0, 0}, {0, 0}, {3, 257}, {1, 0}, {1, 0}});
    for (int t = 0; t < 4; t++)
        for (size_t n : kCounts) {
            check("alone", {{t, n}});
            check("between empty pieces", {{(t + 1) % 4, 0}, {t, n}, {(t + 2) % 4, 0}});
            for (int u = 0; u < 4; u++)
                for (size_t m : kCounts) check("pair", {{t, n}, {u, m}});
        }
    if (failures) return 1;
    printf("scratch carve ok\n");
    return 0;
}
