// inflate_large_size.hip -- the kernels of zng_rocm_uncompress_large_size_dev / _sizes_dev: the plaintext length of LARGE
// device-resident streams without decoding them.  Both are the sizing kernel of inflate_sizes.hip -- its text, included here as
// there (inflate_sizes_body.h): the decoder's bit reader, block headers and tables, and a symbol loop that adds a literal's 1 and
// a match's length to a count and stores nothing -- with a 64-bit count that does not saturate:
//   inflate_size_parts_kernel    one wavefront per PART of a stream, as inflate_streams_kernel<PART> (inflate_dev.hip): from bit
//                                starts[job] to the first block end that is a later start of the same stream.  It writes the
//                                part kernel's eight result words (the count's high word in r[7]: inflate_large_size_plan.h),
//                                so the chain is walked as the decode's is.  A part's output length does not depend on what
//                                lies in front of it: no slot, no window, no ring, no global store but those eight words
//   inflate_size_stream_kernel   one wavefront per whole stream: the streams the chain cannot do (short, fewer than four
//                                starts, anything irregular).  It gives the decoder's verdict, message and consumed bytes as
//                                zng_rocm_inflate_sizes_dev's row does, the truncation rule included
// The host side -- finder, starts, the launch, the walk, which streams go to the second kernel -- is pass_run's counting mode
// (inflate_large.hip) under the rules of inflate_large_size_plan.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "context.h"
#include "inflate_dev.h"
#include "inflate_sizes_plan.h"
#include "inflate_tables.h"

namespace zr {

// jobs: in / in_len the part's whole stream, dict_len the history in front of the part's first byte (the stream's first
// part: the caller's window_len; every other: 32768, so that a distance further back than that is the part's own "invalid
// distance too far back"), flags one past the last start of the part's own stream (0: njobs).  out / out_cap: not looked at.
__global__ __launch_bounds__(64)
void inflate_size_parts_kernel(const InflateJobDev *__restrict__ jobs, uint32_t njobs, const unsigned long long *__restrict__ starts,
                               uint32_t *__restrict__ results) {
    constexpr int kLitRoot = kLitRootStream, kDistRoot = kDistRootStream;
    constexpr bool WIDE = true, PARTS = true;
    __shared__ SizesLds<kDistRoot, kLitRoot> L;
    const int lane = threadIdx.x;
    const uint32_t job = blockIdx.x;
    if (job >= njobs) return;
    const InflateJobDev J = jobs[job];
    const ZR_GLOBAL uint8_t *const in = (const ZR_GLOBAL uint8_t *)J.in;
    const uint32_t in_len = (uint32_t)J.in_len, hist = J.dict_len;
    const uint32_t jend = J.flags ? J.flags : njobs;
#include "inflate_sizes_body.h"
    if (lane == 0) {
        const unsigned long long b = bit_pos();
        results[8 * job + 0] = (uint32_t)count;
        results[8 * job + 1] = (uint32_t)b;
        results[8 * job + 2] = (uint32_t)(b >> 32);
        results[8 * job + 3] = msg == kMsgNone ? (last ? 1u : 0u) : is_status_of(msg);
        results[8 * job + 4] = msg;
        results[8 * job + 5] = reach;
        results[8 * job + 6] = hit;
        results[8 * job + 7] = (uint32_t)(count >> 32);
    }
}

// jobs: in / in_len the stream, dict_len the length of the history in front of its output; results: 8 words per job, see
// ls_stream_row (inflate_large_size_plan.h)
__global__ __launch_bounds__(64)
void inflate_size_stream_kernel(const InflateJobDev *__restrict__ jobs, uint32_t njobs, uint32_t *__restrict__ results) {
    constexpr int kLitRoot = kLitRootStream, kDistRoot = kDistRootStream;
    constexpr bool WIDE = true, PARTS = false;
    __shared__ SizesLds<kDistRoot, kLitRoot> L;
    const int lane = threadIdx.x;
    const uint32_t job = blockIdx.x;
    if (job >= njobs) return;
    const InflateJobDev J = jobs[job];
    const ZR_GLOBAL uint8_t *const in = (const ZR_GLOBAL uint8_t *)J.in;
    const uint32_t in_len = (uint32_t)J.in_len, hist = J.dict_len;
    const unsigned long long *const starts = nullptr;    // (the part form's; see inflate_sizes_body.h)
    const uint32_t jend = 0;
#include "inflate_sizes_body.h"
    if (lane == 0) {
        const unsigned long long used = (bit_pos() + 7ull) >> 3, n = msg == kMsgStarved ? sure : count;
        results[8 * job + 0] = (uint32_t)n;
        results[8 * job + 1] = (uint32_t)(n >> 32);
        results[8 * job + 2] = used > in_len ? in_len : (uint32_t)used;
        results[8 * job + 3] = is_status_of(msg);
        results[8 * job + 4] = msg;
    }
}

int launch_inflate_size_parts_device(const InflateJobDev *d_jobs, size_t njobs, const unsigned long long *d_starts, uint32_t *d_results,
                                     hipStream_t st) {
    ZR_LAUNCH_TRACED(inflate_size_parts_kernel, dim3((unsigned)njobs), dim3(64), st, d_jobs, (uint32_t)njobs, d_starts, d_results);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

int launch_inflate_size_streams_device(const InflateJobDev *d_jobs, size_t njobs, uint32_t *d_results, hipStream_t st) {
    ZR_LAUNCH_TRACED(inflate_size_stream_kernel, dim3((unsigned)njobs), dim3(64), st, d_jobs, (uint32_t)njobs, d_results);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

}  // namespace zr
