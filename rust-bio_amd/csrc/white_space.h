// char::is_whitespace (the Unicode White_Space property), shared by the FASTQ and FASTA readers: str::trim_end and the
// header split go by it.  (fasta_ingest.hip's fa_stage tests the same set on the UTF-8 bytes of a character's end.)
#ifndef BG_WHITE_SPACE_H
#define BG_WHITE_SPACE_H
#include <hip/hip_runtime.h>

#include <cstdint>

__device__ __forceinline__ bool is_ws(uint32_t cp) {  // char::is_whitespace
    return (cp >= 9 && cp <= 13) || cp == 0x20 || cp == 0x85 || cp == 0xA0 || cp == 0x1680 || (cp >= 0x2000 && cp <= 0x200A) ||
           cp == 0x2028 || cp == 0x2029 || cp == 0x202F || cp == 0x205F || cp == 0x3000;
}
#endif
