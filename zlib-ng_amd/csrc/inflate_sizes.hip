// inflate_sizes.hip -- the read side of zng_rocm_compress_members_dev: many device-resident raw / zlib / gzip streams whose
// plaintext lengths nobody handed over.
//   zng_rocm_inflate_sizes_dev       one small kernel parses every header (framing_dev.hip: parse_header_kernel) -> the SIZING
//                                    kernel walks every payload and adds up what it would produce: the row the decode would
//                                    write with all the room there is, without the comparison of the check value and ISIZE
//   zng_rocm_uncompress_packed_dev   the same two kernels, the rows to scratch -> one workgroup turns the sizes into places (a
//                                    tiled scan over any njobs) -> one small kernel patches out / out_cap of the device job table
//                                    -> the existing engine, check-value pass and verify_trailer_kernel decode that table
//                                    (framing_dev.hip: uncompress_patched_device) -> one small kernel writes the final rows
// Nothing crosses PCIe between the kernels and nothing synchronises: the lengths only ever exist on the device.
//
// The sizing kernel is the stream kernel of inflate_dev.hip with everything taken out that moves a byte: one wavefront per
// stream and a symbol loop that adds a literal's 1 and a match's length to a count.  What comes in front of the symbol loop is
// the decoder's own text, included here as it is there: the 64-word fetch and bit buffer (inflate_bits_body.h), the fixed
// tables and the dynamic block header (inflate_block_tables_body.h), the table builder and the packed LDS layout
// (inflate_tables.h) -- so the same bits are consumed in front of every header fault by construction.  The loop still decodes
// every distance -- for its bits, and for "invalid distance too far back" against count + history length -- but has no window,
// no ring, no copy and no store: the history's LENGTH is all it knows of the history.  Every verdict, message and count of
// consumed bytes of the loop is the decoder's (inflate_streams_body.h), the truncation rule of kBadWide included: the two are
// held against each other stream by stream in tests/test_gpu_inflate_sizes.py.  The rules on top -- argument checks,
// saturation, the member's row, places, fit, final rows -- are inflate_sizes_plan.h's, for host and device alike.
// The kernel's body is program text of its own (inflate_sizes_body.h): the sizing kernels of LARGE streams
// (inflate_large_size.hip) include it too, with a 64-bit count; here it is included with the 32-bit saturating one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "context.h"
#include "dict_dev.h"
#include "framing_dev.h"
#include "inflate_dev.h"
#include "inflate_sizes_plan.h"
#include "inflate_tables.h"

namespace zr {

__device__ __forceinline__ IsRow load_row(const uint32_t *rows, uint32_t i) {
    return IsRow{rows[4 * i], rows[4 * i + 1], rows[4 * i + 2], rows[4 * i + 3]};
}
__device__ __forceinline__ void store_row(uint32_t *rows, uint32_t i, IsRow r) {
    rows[4 * i] = r.out_len;
    rows[4 * i + 1] = r.used;
    rows[4 * i + 2] = r.status;
    rows[4 * i + 3] = r.msg;
}

// given: the members as the caller named them; patched, head: parse_header_kernel's tables of them.  own_hist: a raw stream
// without a dictionary object counts given[job].dict_len bytes as present in front of its output (the header pass knows no
// such history); else the history is what the header's verdict gave, patched[job].dict_len.
__global__ __launch_bounds__(64)
void inflate_sizes_kernel(const InflateJobDev *__restrict__ given, const InflateJobDev *__restrict__ patched,
                          const uint32_t *__restrict__ head, uint32_t njobs, int format, int own_hist,
                          uint32_t *__restrict__ results) {
    constexpr int kLitRoot = kLitRootStream, kDistRoot = kDistRootStream;
    __shared__ SizesLds<kDistRoot, kLitRoot> L;
    const int lane = threadIdx.x;
    const uint32_t job = blockIdx.x;
    if (job >= njobs) return;
    const InflateJobDev J = patched[job];
    const uint32_t hdr = head[2 * job], hmsg = head[2 * job + 1];
    const uint64_t member_len = given[job].in_len;
    if (hmsg != kMsgNone) {                              // a refused header, another dictionary: nothing to parse
        if (lane == 0) store_row(results, job, is_sizing_row(format, hdr, hmsg, member_len, IsRow{0u, 0u, 0u, 0u}));
        return;
    }
    const ZR_GLOBAL uint8_t *const in = (const ZR_GLOBAL uint8_t *)J.in;
    const uint32_t in_len = (uint32_t)J.in_len, hist = own_hist ? given[job].dict_len : J.dict_len;

    constexpr bool WIDE = false, PARTS = false;          // 32-bit saturating count, a whole stream per wavefront
    const unsigned long long *const starts = nullptr;    // (the part form's; see inflate_sizes_body.h)
    const uint32_t jend = 0;
#include "inflate_sizes_body.h"
    if (lane == 0) {
        const unsigned long long used = (bit_pos() + 7ull) >> 3;
        const IsRow raw = {msg == kMsgStarved ? sure : count, used > in_len ? in_len : (uint32_t)used, is_status_of(msg), msg};
        store_row(results, job, is_sizing_row(format, hdr, hmsg, member_len, raw));
    }
}

// ---- packed decode: places, the patched table, the final rows -----------------------------------------------------------
// one workgroup, a tiled scan over any njobs (as cs_scan_kernel): offsets[i] = the sum of the padded rooms in front of job i,
// offsets[njobs] = the end of the last job's bytes
__global__ __launch_bounds__(1024)
void sizes_place_kernel(const uint32_t *__restrict__ sizing, uint32_t njobs, uint32_t align, unsigned long long *__restrict__ offsets) {
    __shared__ unsigned long long wave_sum[16];
    __shared__ unsigned long long carry;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) {
        carry = 0;
        if (!njobs) offsets[0] = 0;
    }
    __syncthreads();
    for (uint32_t base = 0; base < njobs; base += 1024u) {
        const uint32_t i = base + (uint32_t)t;
        const bool live = i < njobs;
        const unsigned long long room = live ? is_room(load_row(sizing, i)) : 0ull;
        const unsigned long long v = is_padded(room, align);
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
        if (live) {
            const unsigned long long off = before + incl - v;
            offsets[i] = off;
            if (i + 1u == njobs) offsets[njobs] = is_need(off, room);
        }
        __syncthreads();
        if (t == 1023) carry = before + incl;
        __syncthreads();
    }
}

__device__ __forceinline__ bool sizes_decoded(IsRow sizing, unsigned long long off, unsigned long long dst_cap) {
    return (int32_t)sizing.status == 1 && is_fits(off, is_room(sizing), dst_cap);
}

// a job that has a place and fits: out = d_dst + its offset, out_cap = its size; every other job becomes an empty job, which
// costs the engine nothing and stores nothing
__global__ __launch_bounds__(256)
void sizes_patch_kernel(const uint32_t *__restrict__ sizing, const unsigned long long *__restrict__ offsets, uint32_t njobs,
                        uint8_t *d_dst, unsigned long long dst_cap, InflateJobDev *__restrict__ patched) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= njobs) return;
    const IsRow s = load_row(sizing, i);
    InflateJobDev p = patched[i];
    if (sizes_decoded(s, offsets[i], dst_cap)) {
        p.out = d_dst + offsets[i];
        p.out_cap = s.out_len;
    } else {
        p.out = nullptr;
        p.in_len = 0;
        p.out_cap = 0;
    }
    patched[i] = p;
}

__global__ __launch_bounds__(256)
void sizes_final_kernel(const uint32_t *__restrict__ sizing, const unsigned long long *__restrict__ offsets, uint32_t njobs,
                        unsigned long long dst_cap, uint32_t *__restrict__ results) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= njobs) return;
    const IsRow s = load_row(sizing, i);
    store_row(results, i, is_final_row(s, sizes_decoded(s, offsets[i], dst_cap), load_row(results, i)));
}

// Streams per CU: the tables let 22 wavefronts share a CU's 160 KiB of LDS; held at the decoder's 16 (padded to 10 KiB in a
// build made for the measurement) the kernel measured the same within the spread, so the natural size stays.
static int launch_inflate_sizes(const InflateJobDev *d_given, const InflateJobDev *d_patched, const uint32_t *d_head, size_t njobs,
                                int format, bool own_hist, uint32_t *d_rows, hipStream_t st) {
    ZR_LAUNCH_TRACED(inflate_sizes_kernel, dim3((unsigned)njobs), dim3(64), st, d_given, d_patched, d_head, (uint32_t)njobs, format,
                     own_hist ? 1 : 0, d_rows);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

// both calls: `packed` = zng_rocm_uncompress_packed_dev.  The arguments have passed inflate_sizes_plan.h's checks.
static int sizes_body(bool packed, int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                      uint8_t *d_dst, size_t dst_cap, uint32_t align, uint64_t *d_offsets, uint32_t *d_results, hipStream_t st) {
    DeviceGuard dev;
    Workspace *ws = workspace_for(st);
    if (!ws) return ZNG_ROCM_ENOMEM;
    std::lock_guard<std::mutex> use(ws->mu);
    unsigned long long *const d_off = reinterpret_cast<unsigned long long *>(d_offsets);
    if (!njobs) {                                        // (the packed call alone gets here: an empty batch needs no room)
        hipLaunchKernelGGL(sizes_place_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t *)nullptr, 0u, align, d_off);
        ZR_HIP(hipGetLastError());
        return ZNG_ROCM_OK;
    }
    uint32_t *d_sizing = d_results;
    if (packed)
        if (int rc = scratch_reserve(ws, kScrSizes, njobs * 4 * sizeof(uint32_t), false, (void **)&d_sizing)) return rc;
    GivenJobs g;
    if (int rc = upload_given_jobs(ws, format, dict, jobs, njobs, false, packed, &g, st)) return rc;
    if (int rc = launch_inflate_sizes(g.d_given, g.d_patched, g.d_head, njobs, format, format == 0 && !dict, d_sizing, st)) return rc;
    if (!packed) return ZNG_ROCM_OK;
    const dim3 grid((unsigned)((njobs + 255) / 256)), block(256);
    hipLaunchKernelGGL(sizes_place_kernel, dim3(1), dim3(1024), 0, st, d_sizing, (uint32_t)njobs, align, d_off);
    ZR_HIP(hipGetLastError());
    hipLaunchKernelGGL(sizes_patch_kernel, grid, block, 0, st, d_sizing, d_off, (uint32_t)njobs, d_dst, (unsigned long long)dst_cap,
                       g.d_patched);
    ZR_HIP(hipGetLastError());
    if (int rc = uncompress_patched_device(format, dict, g.d_given, g.d_patched, g.d_head, g.d_checks, g.d_msg, g.d_part, njobs,
                                           d_results, st))
        return rc;
    hipLaunchKernelGGL(sizes_final_kernel, grid, block, 0, st, d_sizing, d_off, (uint32_t)njobs, (unsigned long long)dst_cap,
                       d_results);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

// the refusals in inflate_sizes_plan.h's order, then the device (the dictionary's, or the context of zng_rocm_init): 0 = go on
static int sizes_enter(bool packed, int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                       const void *d_dst, size_t dst_cap, uint32_t align, const void *d_offsets, const void *d_results) {
    const int rc = packed ? is_packed_call_check(format, dict != nullptr, jobs, njobs, d_dst, dst_cap, align, d_offsets, d_results)
                          : is_call_check(format, dict != nullptr, jobs, njobs, d_results);
    if (rc) {
        set_error(packed ? "format 0..2 (2 takes no dictionary), align 0, 1 or a power of two up to 4096, d_offsets and d_results, "
                           "and d_dst unless dst_cap is 0"
                         : "format 0..2 (2 takes no dictionary), and jobs and d_results unless njobs is 0");
        return rc;
    }
    uint64_t bad = 0;
    if (int jrc = is_jobs_check(format, dict != nullptr, jobs, njobs, packed, &bad)) {
        set_error("job %llu: null input, a stream of 2 GiB and more, flags, or a dict_len that is above 32768 or stands beside a "
                  "dictionary object, a wrapped format or a packed destination", (unsigned long long)bad);
        return jrc;
    }
    if (!packed && !njobs) return ZNG_ROCM_OK;           // (the caller returns: nothing to do needs no device)
    if (dict) return dict_usable(dict);
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    return ZNG_ROCM_OK;
}

}  // namespace zr

using namespace zr;

extern "C" {

int zng_rocm_inflate_sizes_dev(int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                               uint32_t *d_results, void *stream) {
    if (int rc = sizes_enter(false, format, dict, jobs, njobs, nullptr, 0, 0, nullptr, d_results)) return rc;
    if (!njobs) return ZNG_ROCM_OK;
    return sizes_body(false, format, dict, jobs, njobs, nullptr, 0, 0, nullptr, d_results, (hipStream_t)stream);
}

int zng_rocm_uncompress_packed_dev(int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                                   uint8_t *d_dst, size_t dst_cap, uint32_t align, uint64_t *d_offsets, uint32_t *d_results,
                                   void *stream) {
    if (int rc = sizes_enter(true, format, dict, jobs, njobs, d_dst, dst_cap, align, d_offsets, d_results)) return rc;
    return sizes_body(true, format, dict, jobs, njobs, d_dst, dst_cap, align, d_offsets, d_results, (hipStream_t)stream);
}

}  // extern "C"
