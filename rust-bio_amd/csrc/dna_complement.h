// dna::complement (rust-bio alphabets/dna.rs) as a 256-byte table: AGCTYRWSKMDVHBN -> TCGARYWSMKHBDVN, the same in lower
// case, every other byte (N, $, ...) itself.  For bg_revcomp_batch_dev and the stranded seed-and-extend (seed_extend.hip),
// SEQ of a reverse-strand SAM record (sam_emit.hip) and the R half of a T$R$ reference (fasta_ingest.hip).  fmd_smems.hip
// builds its own in LDS inside K7's preload loop.
#ifndef BG_DNA_COMPLEMENT_H
#define BG_DNA_COMPLEMENT_H
#include "bg_common.h"

struct alignas(16) ComplementTable {
    uint8_t v[256];
};
constexpr ComplementTable make_complement() {
    ComplementTable t{};
    for (int i = 0; i < 256; i++) t.v[i] = (uint8_t)i;
    const char* a = "AGCTYRWSKMDVHBN";
    const char* b = "TCGARYWSMKHBDVN";
    for (int i = 0; a[i]; i++) {
        t.v[(uint8_t)a[i]] = (uint8_t)b[i];
        t.v[(uint8_t)a[i] + 32] = (uint8_t)(b[i] + 32);
    }
    return t;
}
namespace {  // one instance per translation unit that includes this
__constant__ ComplementTable kComplement = make_complement();
}

// the block's copy of the table (256 bytes of LDS, 4-byte aligned): 64 dwords, one per lane of the first wavefront
__device__ __forceinline__ void load_complement(uint8_t* s_comp) {
    if (threadIdx.x < 64) ((uint32_t*)s_comp)[threadIdx.x] = ((const uint32_t*)kComplement.v)[threadIdx.x];
    __syncthreads();
}

// dst[0 .. L) = revcomp(src[0 .. L)) by the 64 lanes of one wavefront
__device__ __forceinline__ void revcomp_wave(const uint8_t* s_comp, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                             uint64_t L, uint32_t lane) {
    for (uint64_t i = lane; i < L; i += 64) dst[i] = s_comp[src[L - 1 - i]];
}

#endif
