// bg_carve: the arrays of one device scratch buffer, listed once (bg_common.h includes this; bg_reserve_carved runs it).
// Plain host C++: nothing of HIP in here.
#ifndef BG_CARVE_H
#define BG_CARVE_H

#include <cstddef>
#include <cstdint>

// A list of arrays is a callable that calls take<T>(n) once for each.  Run on a carver without a base it measures: every
// take returns null and `at` ends as the bytes the list needs.  Run on a carver with a base it binds: every take returns
// its piece of [base, base + at).  Every piece starts on a 256-byte boundary of the buffer and has at least 256 bytes of
// its own, so a piece of no elements still has an address inside the reservation that no other piece uses.
struct bg_carve {
    uint8_t* base = nullptr;
    size_t at = 0;

    template <class T>
    T* take(size_t n) {
        const size_t o = at, bytes = n ? n * sizeof(T) : 1;
        at += (bytes + 255) & ~(size_t)255;
        return base ? (T*)(base + o) : nullptr;
    }
};

#endif
