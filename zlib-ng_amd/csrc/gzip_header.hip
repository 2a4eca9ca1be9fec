// gzip_header.hip -- zng_rocm_gzip_headers_dev: the header FIELDS of the members of a gzip file that sits in device memory
// (inflateGetHeader, zlib-ng.h.in:1020-1055, inflate.c:556-700), and the two host calls of the writer's rules
// (zng_rocm_gzip_header_bytes / _write, deflate.c:922-1023) and of the reader's (zng_rocm_gzip_header_parse).  The rules are
// gzip_header_plan.h on top of framing_parse.h; the members table is the caller's (zng_rocm_gunzip_members_dev,
// zng_rocm_bgzf_index_dev, or the d_offsets of the writers).
//   gh_walk_kernel     one wavefront per member: wrapper_parse_rules, then the fields of an accepted header (gh_walk over
//                      WaveBytes: the terminators are searched 4 KiB per step, as far as the member reaches); lane 0 writes the
//                      row and the descriptor of the FHCRC's message
//   the FHCRC          the many-message checksum pass, one workgroup per header, as the header kernels of framing_large.hip do
//   gh_scan_kernel     one workgroup: the stored 16 bits against the pass's (gh_hcrc_bad), then text_off = the exclusive scan
//                      of the members' gather lengths in tiles of 1024, and the total
//   -> the rows come down, once
//   gh_gather_kernel   one workgroup per member moves extra, name and comment to its place in the text (bgzf_copy.h) and writes
//                      the terminators
//   -> the text comes down
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "checksum_args.h"
#include "context.h"

#include "bgzf_copy.h"
#include "compress_streams_plan.h"
#include "framing_large.h"
#include "gzip_header_plan.h"

namespace zr {

// one wavefront per member
__global__ __launch_bounds__(64)
void gh_walk_kernel(const HeadJob *__restrict__ jobs, uint32_t n, const DeviceTables *__restrict__ tabs, GhRow *__restrict__ rows,
                    StreamArgs *__restrict__ sa, FinalArgs *__restrict__ fa) {
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const HeadJob j = jobs[i];
    const GhRow r = gh_walk(WaveBytes{j.src}, j.len);
    if (threadIdx.x != 0) return;
    rows[i] = r;
    fill_check_descriptor(j.src, gh_hcrc_bytes(r), tabs, 0, 1, sa + i, fa + i);     // inflate.c:686-692
}

// one workgroup: rows[i].text_off, and *need = the bytes of the text
__global__ __launch_bounds__(1024)
void gh_scan_kernel(GhRow *__restrict__ rows, const uint32_t *__restrict__ crc2, uint32_t n, unsigned long long *__restrict__ need) {
    __shared__ unsigned long long wave_sum[16];
    __shared__ unsigned long long carry;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) carry = 0ull;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 1024u) {      // (uniform trip count: the barriers inside are reached by all)
        const uint32_t i = base + (uint32_t)t;
        const bool live = i < n;
        unsigned long long v = 0ull;
        if (live) {
            const GhRow r = rows[i];
            if (gh_hcrc_bad(r, crc2[2 * i + 1])) rows[i] = gh_row_hcrc_refused();
            else v = gh_gather_len(r);
        }
        unsigned long long incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long up = (unsigned long long)__shfl_up((long long)incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        unsigned long long before = carry;
        for (int w = 0; w < wave; ++w) before += wave_sum[w];
        if (live) rows[i].text_off = before + incl - v;
        __syncthreads();
        if (t == 1023) carry = before + incl;
        __syncthreads();
    }
    if (t == 0) *need = carry;
}

// one workgroup per member; every store lies in text[0, need)
__global__ __launch_bounds__(256)
void gh_gather_kernel(const HeadJob *__restrict__ jobs, const GhRow *__restrict__ rows, uint32_t n, uint8_t *__restrict__ text,
                      unsigned long long need) {
    const int t = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const GhRow r = rows[i];
        if (r.status != 0) continue;
        const uint8_t *src = jobs[i].src;
        unsigned long long at = r.text_off;
        bgzf_copy(text, at, need, src + r.extra_off, r.extra_len, t);
        at += r.extra_len;
        if (r.name_off) {
            bgzf_copy(text, at, need, src + r.name_off, r.name_len, t);
            at += r.name_len;
            if (t == 0 && at < need) text[at] = 0;
            ++at;
        }
        if (r.comment_off) {
            bgzf_copy(text, at, need, src + r.comment_off, r.comment_len, t);
            at += r.comment_len;
            if (t == 0 && at < need) text[at] = 0;
        }
    }
}

namespace {

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

int headers_run(const uint8_t *d_src, const zng_rocm_gzip_member *members, size_t n, zng_rocm_gzip_header_row *rows, uint8_t *text,
                size_t text_cap, size_t *text_need, hipStream_t st, Workspace *ws) {
    Context *c = ctx();
    // device: rows | need | jobs | descriptors | partials | the pass's results; pinned: jobs on their way up | rows and need
    // on their way down
    const size_t o_need = n * sizeof(GhRow), down = o_need + sizeof(unsigned long long);
    const size_t o_jobs = up16(down), o_sa = o_jobs + up16(n * sizeof(HeadJob)), o_fa = o_sa + up16(n * sizeof(StreamArgs));
    const size_t o_part = o_fa + up16(n * sizeof(FinalArgs)), o_crc = o_part + n * sizeof(Partial);
    const size_t total = o_crc + n * 2 * sizeof(uint32_t), h_down = up16(n * sizeof(HeadJob));
    uint8_t *d = nullptr, *h = nullptr;
    {
        std::lock_guard<std::mutex> use(ws->mu);
        if (int rc = scratch_reserve(ws, kScrGzipHeader, total, false, (void **)&d)) return rc;
        if (int rc = host_tables_acquire(ws)) return rc;
        if (int rc = scratch_reserve(ws, kScrGzipHeaderHost, h_down + down, true, (void **)&h)) return rc;
        HeadJob *hj = reinterpret_cast<HeadJob *>(h);
        for (size_t i = 0; i < n; ++i) hj[i] = HeadJob{d_src + members[i].src_off, members[i].src_len};
        ZR_HIP(hipMemcpyAsync(d + o_jobs, h, n * sizeof(HeadJob), hipMemcpyHostToDevice, st));
        if (int rc = host_tables_release(ws, st)) return rc;
    }
    GhRow *d_rows = reinterpret_cast<GhRow *>(d);
    unsigned long long *d_need = reinterpret_cast<unsigned long long *>(d + o_need);
    const HeadJob *d_jobs = reinterpret_cast<const HeadJob *>(d + o_jobs);
    StreamArgs *d_sa = reinterpret_cast<StreamArgs *>(d + o_sa);
    FinalArgs *d_fa = reinterpret_cast<FinalArgs *>(d + o_fa);
    uint32_t *d_crc = reinterpret_cast<uint32_t *>(d + o_crc);
    hipLaunchKernelGGL(gh_walk_kernel, dim3((unsigned)n), dim3(64), 0, st, d_jobs, (uint32_t)n, c->tables, d_rows, d_sa, d_fa);
    ZR_HIP(hipGetLastError());
    if (int rc = launch_checksum_batch_device(false, true, d_sa, d_fa, reinterpret_cast<Partial *>(d + o_part), n, d_crc, st)) return rc;
    hipLaunchKernelGGL(gh_scan_kernel, dim3(1), dim3(1024), 0, st, d_rows, d_crc, (uint32_t)n, d_need);
    ZR_HIP(hipGetLastError());
    ZR_HIP(hipMemcpyAsync(h + h_down, d, down, hipMemcpyDeviceToHost, st));
    ZR_HIP(hipStreamSynchronize(st));
    const GhRow *h_rows = reinterpret_cast<const GhRow *>(h + h_down);
    for (size_t i = 0; i < n; ++i) gh_row_public(h_rows[i], members[i].src_off, &rows[i]);
    unsigned long long need;
    memcpy(&need, h + h_down + o_need, sizeof need);
    *text_need = (size_t)need;
    if (text_cap < need) {
        set_error("zng_rocm_gzip_headers_dev: the fields take %llu bytes, text_cap is %zu", need, text_cap);
        return kCsBufError;
    }
    if (!need) return ZNG_ROCM_OK;
    uint8_t *d_text = nullptr;
    {
        std::lock_guard<std::mutex> use(ws->mu);
        if (int rc = scratch_reserve(ws, kScrGzipHeaderText, (size_t)need, false, (void **)&d_text)) return rc;
    }
    const unsigned grid = (unsigned)(n < (1u << 20) ? n : (1u << 20));
    hipLaunchKernelGGL(gh_gather_kernel, dim3(grid), dim3(256), 0, st, d_jobs, d_rows, (uint32_t)n, d_text, need);
    ZR_HIP(hipGetLastError());
    ZR_HIP(hipMemcpyAsync(text, d_text, (size_t)need, hipMemcpyDeviceToHost, st));
    ZR_HIP(hipStreamSynchronize(st));
    return ZNG_ROCM_OK;
}

}  // namespace

}  // namespace zr

using namespace zr;

extern "C" {

size_t zng_rocm_gzip_header_bytes(const zng_rocm_gzip_header *h) {
    GhLens lens;
    return gh_check(h, &lens) ? 0 : gh_bytes(h, lens);
}

size_t zng_rocm_gzip_header_write(const zng_rocm_gzip_header *h, int level, int strategy, uint8_t *buf, size_t cap) {
    GhLens lens;
    if (gh_check(h, &lens) || cs_level(level) == kCsLevelRefused || !cs_strategy_ok(strategy)) return 0;
    const size_t n = gh_bytes(h, lens);
    if (!buf || cap < n) return 0;
    gh_render(h, lens, cs_level(level), strategy, buf);
    return n;
}

int zng_rocm_gzip_header_parse(const uint8_t *src, size_t src_len, zng_rocm_gzip_header_row *row) {
    if (!row) return ZNG_ROCM_EINVAL;
    if (!src && src_len) {
        gh_row_public(gh_row_refused(ZNG_ROCM_EINVAL, kWrapNone), 0, row);
        row->msg = nullptr;
        return ZNG_ROCM_EINVAL;
    }
    gh_row_public(gh_parse_host(src, src_len), 0, row);
    return row->status;
}

int zng_rocm_gzip_headers_dev(const uint8_t *d_src, size_t src_len, const zng_rocm_gzip_member *members, size_t nmembers,
                              zng_rocm_gzip_header_row *rows, uint8_t *text, size_t text_cap, size_t *text_need, void *stream) {
    if (text_need) *text_need = 0;
    if (!text_need || (!d_src && src_len) || (nmembers && (!members || !rows)) || (!text && text_cap) || nmembers > 0x7fffffffull) {
        set_error("zng_rocm_gzip_headers_dev: a null pointer with a non-zero count, a null text_need, or more than 2^31 - 1 members");
        return ZNG_ROCM_EINVAL;
    }
    for (size_t i = 0; i < nmembers; ++i)
        if (members[i].src_off > src_len || members[i].src_len > src_len - members[i].src_off) {
            set_error("zng_rocm_gzip_headers_dev: member %zu does not lie inside the %zu bytes of the file", i, src_len);
            return ZNG_ROCM_EINVAL;
        }
    if (!nmembers) return ZNG_ROCM_OK;
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    DeviceGuard dev;
    Workspace *ws = workspace_for((hipStream_t)stream);
    if (!ws) return ZNG_ROCM_ENOMEM;
    return headers_run(d_src, members, nmembers, rows, text, text_cap, text_need, (hipStream_t)stream, ws);
}

}  // extern "C"
