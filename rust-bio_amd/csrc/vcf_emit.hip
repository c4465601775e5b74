// VCF text from candidate sites and indel events (bg_vcf_header, bg_vcf_emit[_dev]): THE RULE is in include/biogpu.h, its
// bodies in vcf_rule.h.  The shape is the SAM writer's (sam_emit.hip): a pass that checks and measures, scans, a pass that
// writes.
//   1. vcf_measure_kernel, a lane an element of the combined list (sites, then events): the element's check with its
//      predecessor, the smallest refused index by an unsigned atomic minimum (a value, not an order of arrival), the SNV flag
//      of a site, the length of the element's line.
//   2. bg_scan_u32 over the SNV flags compacts the sites; vcf_place_kernel, a lane an element: the line's index is the
//      element's rank in its own list plus one binary search in the other list's (region, pos) keys; the length and the
//      element's index go to the line's slot.  bg_scan_u32 over the slots gives the lines' offsets; vcf_totals_kernel puts
//      the refused index, the limit flag, the number of lines and the bytes side by side for ONE read-back.
//   3. vcf_write_kernel, kLanes lanes a line: a line of at most kStage bytes is put together in LDS at the offset inside a
//      16-byte granule that it has in the output and leaves as the SAM writer's lines do (bytes up to the first 16-byte
//      boundary of the destination, 16-byte stores between, bytes behind the last); a longer line is formatted by the same
//      body straight into global memory, the group striding over its REF / ALT bytes.
// kLanes = 8 and kStage = 256: a line of an SNV is 55 to 90 bytes, so eight 16-byte stores take its body in one trip, and the
// eight fixed pieces of a line (vcf_rule.h: VCF_ROLES) are one a lane; 32 lines a workgroup keep (256 + 16) * 32 = 8 704
// bytes of LDS plus the 256-byte fold table, which bounds nothing (160 KB a CU).  A line longer than 256 bytes holds a
// deletion of more than 150 bases or an insertion that long: rare, and bound by its reference reads wherever it is put
// together.
#include <algorithm>
#include <string>

#include "bg_common.h"
#include "vcf_rule.h"

namespace {

constexpr uint32_t kLanes = 8;                 // lanes of a line's group
constexpr uint32_t kGroups = 256 / kLanes;     // lines of a workgroup
constexpr uint32_t kStage = 256;               // bytes of a staged line
constexpr uint32_t kStageBuf = kStage + 16;    // ... plus its offset inside the 16-byte granule of the output

struct VcfResult {  // what the one read-back brings
    unsigned long long first_bad;  // the smallest refused index of the combined list, VCF_NONE if none
    unsigned long long too_large;  // a line of 2^32 bytes or more
    unsigned long long n_lines, out_bytes;
};

// pass 1: one lane an element
__global__ __launch_bounds__(256) void vcf_measure_kernel(const vcf_args_t a, uint32_t* __restrict__ snv, uint32_t* __restrict__ elem_len,
                                                          VcfResult* __restrict__ res) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n_sites + a.n_events) return;
    const bool site = e < a.n_sites;
    const bool ok = site ? vcf_site_ok(a, e) : vcf_event_ok(a, e - a.n_sites);
    const bool line = ok && (!site || a.sites[e].kind == BG_SITE_SNV);
    uint64_t len = 0;
    if (line) len = vcf_line_of(a, e).len;
    if (!ok) atomicMin(&res->first_bad, (unsigned long long)e);
    if (len >> 32) {
        atomicOr(&res->too_large, 1ull);
        len = 0;
    }
    if (site) snv[e] = line ? 1u : 0u;
    elem_len[e] = (uint32_t)len;
}

// pass 2: one lane an element; snv_off: the exclusive scan of the SNV flags.  A line's slot is below n_sites + n_events whatever
// the keys hold, so a list that is refused for its order still writes inside the scratch.
__global__ __launch_bounds__(256) void vcf_place_kernel(const vcf_args_t a, const uint32_t* __restrict__ snv, const uint64_t* __restrict__ snv_off,
                                                        const uint32_t* __restrict__ elem_len, uint32_t* __restrict__ line_len,
                                                        uint32_t* __restrict__ line_src) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n_sites + a.n_events) return;
    uint64_t slot;
    if (e < a.n_sites) {
        if (!snv[e]) return;
        slot = snv_off[e] + vcf_events_before(a.events, a.n_events, a.sites[e].region, a.sites[e].pos);
    } else {
        const bg_bam_indel_t& v = a.events[e - a.n_sites];
        slot = (e - a.n_sites) + snv_off[vcf_sites_upto(a.sites, a.n_sites, v.region, v.pos)];
    }
    line_len[slot] = elem_len[e];
    line_src[slot] = (uint32_t)e;
}

__global__ void vcf_totals_kernel(VcfResult* __restrict__ res, const uint64_t* __restrict__ snv_off, uint64_t n_sites, uint64_t n_events,
                                  const uint64_t* __restrict__ line_off) {
    res->n_lines = snv_off[n_sites] + n_events;
    res->out_bytes = line_off[n_sites + n_events];
}

// pass 3: kLanes lanes a line, kGroups lines a workgroup
__global__ __launch_bounds__(256) void vcf_write_kernel(const vcf_args_t a, uint64_t n_lines, const uint32_t* __restrict__ line_src,
                                                        const uint64_t* __restrict__ line_off, char* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) char s_stage[kGroups * kStageBuf];
    __shared__ __attribute__((aligned(4))) uint8_t s_fold[256];
    s_fold[threadIdx.x] = vcf_ref_byte((uint8_t)threadIdx.x);
    __syncthreads();
    const uint32_t g = threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
    const uint64_t l = (uint64_t)blockIdx.x * kGroups + g;
    if (l >= n_lines) return;  // (no barrier follows: a group's stage is its own, and its lanes share a wavefront)
    const vcf_line_t L = vcf_line_of(a, line_src[l]);
    char* line = out + line_off[l];
    if (L.len > kStage) {
        vcf_put_lane(a, L, s_fold, line, lane, kLanes);
        return;
    }
    const uint32_t len = (uint32_t)L.len, mis = (uint32_t)((uintptr_t)line & 15);
    char* stage = s_stage + g * kStageBuf + mis;
    vcf_put_lane(a, L, s_fold, stage, lane, kLanes);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // head up to the first 16-byte boundary and tail behind the last one byte by byte, everything between as 16-byte stores
    const uint32_t head = min(len, (16 - mis) & 15);
    const uint32_t body = (len - head) >> 4, tail = (len - head) & 15;
    for (uint32_t i = lane; i < head; i += kLanes) line[i] = stage[i];
    for (uint32_t i = lane; i < body; i += kLanes) *(uint4*)(line + head + 16 * i) = *(const uint4*)(stage + head + 16 * i);
    for (uint32_t i = lane; i < tail; i += kLanes) line[head + 16 * body + i] = stage[head + 16 * body + i];
}

// a refusal leaves the totals 0 and names no element
void vcf_clear(uint64_t* n_lines, uint64_t* out_bytes, uint64_t* first_bad) {
    if (n_lines) *n_lines = 0;
    if (out_bytes) *out_bytes = 0;
    if (first_bad) *first_bad = VCF_NONE;
}

int vcf_check(bg_ctx* ctx, const bg_vcf_params_t* prm, const void* sites, uint64_t n_sites, const void* events, uint64_t n_events, const void* seq,
              uint64_t n_seq, const void* contigs, uint64_t n_contigs, const void* names, const void* text, uint64_t n_text, const void* out,
              uint64_t out_cap, const void* line_off, const uint64_t* n_lines, const uint64_t* out_bytes, const uint64_t* first_bad) {
    if (!ctx || !prm || !n_lines || !out_bytes || !first_bad) return bg_refuse("bg_vcf_emit: a null ctx, params or result pointer");
    if (prm->flags || prm->reserved) return bg_refuse("bg_vcf_emit: flags and reserved are 0");
    if ((n_sites && !sites) || (n_events && !events) || (n_seq && !seq) || (n_contigs && (!contigs || !names)) || (n_text && !text))
        return bg_refuse("bg_vcf_emit: a null array with a count");
    if (!out && out_cap) return bg_refuse("bg_vcf_emit: a null out with a capacity");
    if (((uintptr_t)sites & 3) || ((uintptr_t)events & 7) || ((uintptr_t)line_off & 7)) return bg_refuse("bg_vcf_emit: sites, events or line_off misaligned");
    return BG_OK;
}

}  // namespace

extern "C" int bg_vcf_header(const bg_sam_contig_t* contigs, uint64_t n_contigs, const char* names, char* out, uint64_t out_cap,
                             uint64_t* out_bytes) {
    if (!out_bytes || (n_contigs && (!contigs || !names)) || (!out && out_cap)) return BG_ERR_INVALID_ARG;
    std::string s = "##fileformat=VCFv4.3\n##source=biogpu\n";
    for (uint64_t c = 0; c < n_contigs; c++) {
        s += "##contig=<ID=";
        s.append(names + contigs[c].name_off, contigs[c].name_len);
        s += ",length=" + std::to_string(contigs[c].len) + ">\n";
    }
    s += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Depth at the position or anchor\">\n"
         "##INFO=<ID=RO,Number=1,Type=Integer,Description=\"Reference observations\">\n"
         "##INFO=<ID=AO,Number=1,Type=Integer,Description=\"Alternate observations\">\n"
         "##INFO=<ID=SAF,Number=1,Type=Integer,Description=\"Alternate observations on the forward strand\">\n"
         "##INFO=<ID=SAR,Number=1,Type=Integer,Description=\"Alternate observations on the reverse strand\">\n"
         "##INFO=<ID=TYPE,Number=1,Type=String,Description=\"snp, del or ins\">\n"
         "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
    *out_bytes = s.size();
    if (!out) return BG_OK;
    if (s.size() > out_cap) return BG_ERR_OPS_CAP;
    memcpy(out, s.data(), s.size());
    return BG_OK;
}

extern "C" int bg_vcf_emit_dev(bg_ctx* ctx, const bg_vcf_params_t* prm, const bg_bam_site_t* d_sites, uint64_t n_sites,
                               const bg_bam_indel_t* d_events, uint64_t n_events, const uint8_t* d_seq, uint64_t n_seq,
                               const bg_sam_contig_t* d_contigs, uint64_t n_contigs, const char* d_names, const uint8_t* d_text, uint64_t n_text,
                               char* d_out, uint64_t out_cap, uint64_t* d_line_off, uint64_t* n_lines, uint64_t* out_bytes, uint64_t* first_bad,
                               void* stream) {
    vcf_clear(n_lines, out_bytes, first_bad);
    int rc = vcf_check(ctx, prm, d_sites, n_sites, d_events, n_events, d_seq, n_seq, d_contigs, n_contigs, d_names, d_text, n_text, d_out, out_cap,
                       d_line_off, n_lines, out_bytes, first_bad);
    if (rc) return rc;
    if (n_sites >> 32 || n_events >> 32 || (n_sites + n_events) >> 32) return BG_ERR_TOO_LARGE;
    hipStream_t st = (hipStream_t)stream;
    BG_HIP(hipSetDevice(ctx->device));
    const uint64_t n = n_sites + n_events;
    if (n == 0) {
        if (d_out && d_line_off) {
            BG_HIP(hipMemsetAsync(d_line_off, 0, 8, st));
            BG_HIP(hipStreamSynchronize(st));
        }
        return BG_OK;
    }
    bg_scratch_guard guard(ctx, st);
    uint32_t *d_snv, *d_elem_len, *d_line_len, *d_line_src;
    uint64_t *d_snv_off, *d_off, *d_sums;
    VcfResult* d_res;
    if ((rc = bg_reserve_carved(&ctx->aux, &ctx->aux_bytes, [&](bg_carve& cv) {
        d_res = cv.take<VcfResult>(1);
        d_snv = cv.take<uint32_t>(n_sites);
        d_snv_off = cv.take<uint64_t>(n_sites + 1);
        d_elem_len = cv.take<uint32_t>(n);
        d_line_len = cv.take<uint32_t>(n);
        d_line_src = cv.take<uint32_t>(n);
        d_off = cv.take<uint64_t>(n + 1);
        d_sums = cv.take<uint64_t>(bg_scan_sums_words(n));
    }))) return rc;
    const vcf_args_t a = {d_sites, n_sites, d_events, n_events, d_seq, n_seq, d_contigs, n_contigs, d_names, d_text, n_text};
    BG_HIP(hipMemsetAsync(d_res, 0, sizeof(VcfResult), st));
    BG_HIP(hipMemsetAsync(&d_res->first_bad, 0xFF, 8, st));  // VCF_NONE
    BG_HIP(hipMemsetAsync(d_line_len, 0, n * sizeof(uint32_t), st));  // the slots behind the last line count nothing
    vcf_measure_kernel<<<lanes(n), dim3(256), 0, st>>>(a, d_snv, d_elem_len, d_res);
    BG_HIP(hipGetLastError());
    if ((rc = bg_scan_u32(d_snv, n_sites, d_snv_off, d_sums, st))) return rc;
    vcf_place_kernel<<<lanes(n), dim3(256), 0, st>>>(a, d_snv, d_snv_off, d_elem_len, d_line_len, d_line_src);
    BG_HIP(hipGetLastError());
    if ((rc = bg_scan_u32(d_line_len, n, d_off, d_sums, st))) return rc;
    vcf_totals_kernel<<<dim3(1), dim3(1), 0, st>>>(d_res, d_snv_off, n_sites, n_events, d_off);
    BG_HIP(hipGetLastError());
    VcfResult res;
    BG_HIP(hipMemcpyAsync(&res, d_res, sizeof(res), hipMemcpyDeviceToHost, st));
    BG_HIP(hipStreamSynchronize(st));
    if (res.first_bad != VCF_NONE) {
        *first_bad = res.first_bad;
        return bg_refuse("bg_vcf_emit: an element is refused (first_bad)");
    }
    if (res.too_large) return BG_ERR_TOO_LARGE;
    *n_lines = res.n_lines;
    *out_bytes = res.out_bytes;
    if (!d_out && !out_cap) return BG_OK;
    if (res.out_bytes > out_cap) return BG_ERR_OPS_CAP;
    if (d_line_off) BG_HIP(hipMemcpyAsync(d_line_off, d_off, (res.n_lines + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (res.n_lines) {
        vcf_write_kernel<<<dim3((uint32_t)((res.n_lines + kGroups - 1) / kGroups)), dim3(256), 0, st>>>(a, res.n_lines, d_line_src, d_off, d_out);
        BG_HIP(hipGetLastError());
    }
    return BG_OK;
}

extern "C" int bg_vcf_emit(bg_ctx* ctx, const bg_vcf_params_t* prm, const bg_bam_site_t* sites, uint64_t n_sites, const bg_bam_indel_t* events,
                           uint64_t n_events, const uint8_t* seq, uint64_t n_seq, const bg_sam_contig_t* contigs, uint64_t n_contigs,
                           const char* names, const uint8_t* text, uint64_t n_text, char* out, uint64_t out_cap, uint64_t* line_off,
                           uint64_t* n_lines, uint64_t* out_bytes, uint64_t* first_bad) {
    vcf_clear(n_lines, out_bytes, first_bad);
    int rc = vcf_check(ctx, prm, sites, n_sites, events, n_events, seq, n_seq, contigs, n_contigs, names, text, n_text, out, out_cap, line_off,
                       n_lines, out_bytes, first_bad);
    if (rc) return rc;
    uint64_t name_bytes = 0;
    for (uint64_t c = 0; c < n_contigs; c++) name_bytes = std::max<uint64_t>(name_bytes, contigs[c].name_off + contigs[c].name_len);
    bg_stage s(ctx, ctx->stream);
    const bg_bam_site_t* d_sites = n_sites ? s.up(sites, n_sites) : nullptr;
    const bg_bam_indel_t* d_events = n_events ? s.up(events, n_events) : nullptr;
    const uint8_t* d_seq = n_seq ? s.up(seq, n_seq) : nullptr;
    const bg_sam_contig_t* d_contigs = n_contigs ? s.up(contigs, n_contigs) : nullptr;
    const char* d_names = n_contigs ? s.up(names, name_bytes) : nullptr;
    const uint8_t* d_text = n_text ? s.up(text, n_text) : nullptr;
    const bool sizing = !out && !out_cap;
    char* d_out = sizing ? nullptr : s.out<char>(out_cap);
    uint64_t* d_line_off = !sizing && line_off ? s.out<uint64_t>(n_sites + n_events + 1) : nullptr;
    if (s.rc) return s.rc;
    rc = bg_vcf_emit_dev(ctx, prm, d_sites, n_sites, d_events, n_events, d_seq, n_seq, d_contigs, n_contigs, d_names, d_text, n_text, d_out, out_cap,
                         d_line_off, n_lines, out_bytes, first_bad, s.st);
    if (rc || sizing) return rc;
    if (d_line_off) s.down(line_off, d_line_off, *n_lines + 1);
    s.down(out, d_out, *out_bytes);
    return s.sync();
}
