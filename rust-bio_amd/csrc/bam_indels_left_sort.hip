// The merge sort of bg_bam_indels_left_dev (bam_indels.hip), in a translation unit of its own.  Its kernels are rocPRIM's with the
// comparator inl_cmp (bam_indels_left_rule.h): tile, shifted anchor, kind, len, then the shifted codes left to right.  It stands
// apart because of what the compiler did with it beside the sort of bg_bam_indels_dev: with both comparators instantiated in
// one file the block-sort kernel of THAT call went from 168 to 184 VGPRs and from 3 to 2 waves a SIMD (kernel-resource-usage
// report, profiles/bam_indels_left_timing.txt); alone in its file each sort is compiled as if the other did not exist.
#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "bg_common.h"
#include "bam_indels_left_rule.h"

namespace {
struct InlOrder {  // indices into raw, whose anchors are the shifted ones
    const ind_raw_t* raw;
    const uint8_t* recs;
    const uint64_t* off;
    __device__ bool operator()(uint32_t a, uint32_t b) const { return inl_cmp(raw[a], raw[b], recs, off) < 0; }
};
}  // namespace

// order[0 .. n) = 0 .. n - 1 sorted by inl_cmp; d_tmp / tmp_bytes: what rocprim::merge_sort asks for n uint32 keys
int inl_sort_raw(void* d_tmp, size_t tmp_bytes, const ind_raw_t* raw, const uint8_t* recs, const uint64_t* off, uint32_t* order, uint64_t n, hipStream_t st) {
    const rocprim::counting_iterator<uint32_t> iota(0);
    BG_HIP(rocprim::merge_sort(d_tmp, tmp_bytes, iota, order, n, InlOrder{raw, recs, off}, st));
    return BG_OK;
}
