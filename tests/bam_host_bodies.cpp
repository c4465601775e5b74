// Stand-alone CPU program for tests/test_bam_host_bodies.py: the __host__ __device__ bodies of csrc/bam_rule.h — the bin, the
// base codes, integer tags in their smallest type, and a BGZF block as the 256 lanes of bgzf_frame_kernel (csrc/bgzf.hip) make
// it: the two tables, every lane's copy and raw CRC share, their XOR, the final CRC — run on the host on inputs read
// from a file; the test builds it with -fsanitize=address,undefined and compares what it writes with tests/bam_oracle.py.
// Input: 4 uint64 (bins, bases, integers, payloads); per bin int64 pos, uint64 ref_len; the bases; the integers (int64); per
// payload 3 uint64 (length, destination residue, source residue) and its bytes.
// Every payload and every block's payload area is allocated at exactly its size behind a poisoned prefix that sets its
// residue mod 16, so that a byte read or written outside one stops the program.  Exit status 3: bam_put_int wrote another
// number of bytes than bam_int_size says; 4: a constant of bam_crc_pow2 is not the square of the one before; 5: the word step
// of the CRC disagrees with four byte steps, or the far step with a multiplication by x^(8 * 4096).
// Output: uint16 per bin; a code byte per base; per integer its tag as written (3 + size bytes, under the name "XY"); per
// payload the whole block (23 bytes, payload, CRC-32, ISIZE); the 28 bytes of the end-of-file block.
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../rust-bio_amd/csrc/bam_rule.h"

template <typename T>
static T* load(FILE* f, size_t count) {
    T* p = (T*)malloc(count * sizeof(T) ? count * sizeof(T) : 1);
    if (count && fread(p, sizeof(T), count, f) != count) exit(2);
    return p;
}
// len bytes at an address = res (mod 16) that end where the allocation ends, the res bytes in front poisoned
static uint8_t* at_residue(size_t len, size_t res) {
    uint8_t* base = (uint8_t*)aligned_alloc(16, (res + len + 15) / 16 * 16);
    // (aligned_alloc wants a multiple of the alignment: what lies behind res + len is poisoned as well)
    ASAN_POISON_MEMORY_REGION(base, res);
    ASAN_POISON_MEMORY_REGION(base + res + len, (res + len + 15) / 16 * 16 - (res + len));
    return base + res;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint64_t* hd = load<uint64_t>(f, 4);
    const uint64_t n_bins = hd[0], n_bases = hd[1], n_ints = hd[2], n_payloads = hd[3];

    for (uint64_t i = 0; i < n_bins; i++) {
        int64_t* pos = load<int64_t>(f, 1);
        uint64_t* ref_len = load<uint64_t>(f, 1);
        const uint16_t bin = bam_bin(*pos, *ref_len);
        fwrite(&bin, 2, 1, o);
        free(pos);
        free(ref_len);
    }
    uint8_t* bases = load<uint8_t>(f, n_bases);
    for (uint64_t i = 0; i < n_bases; i++) fputc((int)bam_base_code(bases[i]), o);
    int64_t* ints = load<int64_t>(f, n_ints);
    for (uint64_t i = 0; i < n_ints; i++) {
        const uint32_t size = 3 + bam_int_size(ints[i]);
        uint8_t* tag = (uint8_t*)malloc(size);
        if (bam_put_int(tag, 'X', 'Y', ints[i]) != size) return 3;
        fwrite(tag, 1, size, o);
        free(tag);
    }

    for (uint32_t j = 0; j < 16; j++)
        if (bam_crc_mul(bam_crc_pow2(j), bam_crc_pow2(j)) != bam_crc_pow2(j + 1)) return 4;
    uint32_t* T = (uint32_t*)malloc(1024 * sizeof(uint32_t));
    for (uint32_t t = 0; t < 256; t++) T[t] = bam_crc_byte_entry(t);
    for (uint32_t t = 0; t < 256; t++) bam_crc_slices(T, t);
    uint32_t* K = (uint32_t*)malloc(1024 * sizeof(uint32_t));
    for (uint32_t t = 0; t < 1024; t++) K[t] = bam_crc_far_entry(t);
    for (uint32_t w = 1, c = 0x12345678u; w; w <<= 1, c = c * 2654435761u + w) {
        uint32_t b = c;
        for (int i = 0; i < 4; i++) b = bam_crc_byte(T, b, (uint8_t)(w >> (8 * i)));
        if (b != bam_crc_word(T, c, w) || bam_crc_far(K, c) != bam_crc_mul(c, bam_crc_xpow8(4096))) return 5;
    }

    for (uint64_t k = 0; k < n_payloads; k++) {
        uint64_t* d = load<uint64_t>(f, 3);
        const uint32_t len = (uint32_t)d[0];
        uint8_t* src = at_residue(len, d[2]);
        if (len && fread(src, 1, len, f) != len) return 2;
        uint8_t* dst = at_residue(len, d[1]);
        uint32_t raw = 0;
        for (uint32_t lane = 0; lane < BGZF_LANES; lane++) raw ^= bgzf_lane(T, K, src, dst, len, lane);
        uint8_t tail[8];
        bam_put32(tail, bam_crc_finish(raw, len));
        bam_put32(tail + 4, len);
        for (uint32_t i = 0; i < BGZF_HEAD; i++) fputc(bgzf_head_byte(i, len), o);
        fwrite(dst, 1, len, o);
        fwrite(tail, 1, 8, o);
        free(src - d[2]);
        free(dst - d[1]);
        free(d);
    }
    for (uint32_t i = 0; i < BGZF_EOF_BYTES; i++) fputc(bgzf_eof_byte(i), o);
    fclose(o);
    fclose(f);
    free(T);
    free(K);
    free(ints);
    free(bases);
    free(hd);
    return 0;
}
