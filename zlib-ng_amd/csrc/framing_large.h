// framing_large.h -- what framing_large.hip shares with gzip_members.hip: the header kernels of the wrapped large calls
// (one wavefront per member runs wrapper_parse_rules, the FHCRC through the many-message checksum pass) over a table of
// members that ALREADY sits in device memory, so that a caller whose members were found on the device runs the same
// kernels without bringing the table down first.  WaveBytes, the way a wavefront reaches a member's bytes, is here for every
// kernel that walks a header with one (gzip_header.hip's field walk as well).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "framing_parse.h"

namespace zr {

struct HeadJob {
    const uint8_t *src;
    uint64_t len;
};

#if defined(__HIPCC__)
// the member's bytes as a wavefront reaches them: every lane calls with the same arguments
struct WaveBytes {
    const uint8_t *src;
    __device__ uint32_t byte(uint64_t pos) const { return src[pos]; }
    // (forced inline: with the three call sites of gzip_header.hip's walk the compiler makes it a function with a stack in scratch)
    __device__ __forceinline__ uint64_t find_zero(uint64_t from, uint64_t n) const {
        const uint32_t lane = threadIdx.x & 63u;
        const uintptr_t base = (uintptr_t)src, lo = base + from, hi = base + n;
        // aligned 16-byte lines: the first and the last reach up to 15 bytes outside [lo, hi) inside their own line (read,
        // never used -- as the checksum kernels read around an unaligned message; include/zng_rocm.h says so to callers)
        for (uintptr_t a = lo & ~(uintptr_t)15; a < hi; a += 4u * 64u * 16u) {
            uint4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uintptr_t mine = a + ((uintptr_t)u * 64u + lane) * 16u;
                v[u] = mine < hi ? *reinterpret_cast<const uint4 *>(mine) : make_uint4(~0u, ~0u, ~0u, ~0u);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uintptr_t mine = a + ((uintptr_t)u * 64u + lane) * 16u;
                const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                uint32_t zmask = 0;                      // bit k: byte k of my line is zero and belongs to [lo, hi)
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const uintptr_t at = mine + k;
                    if (((w[k >> 2] >> (8 * (k & 3))) & 0xffu) == 0u && at >= lo && at < hi) zmask |= 1u << k;
                }
                const unsigned long long vote = __ballot(zmask != 0u);
                if (vote) {
                    const int first = __ffsll((long long)vote) - 1;
                    const uint32_t m = (uint32_t)__shfl((int)zmask, first, 64);
                    return (uint64_t)(a + ((uintptr_t)u * 64u + first) * 16u + (uint32_t)(__ffs((int)m) - 1) - base);
                }
            }
        }
        return n;
    }
};
#endif

// device bytes header_rows_device needs at `d_work` (16-byte aligned) for n members
size_t header_rows_scratch(size_t n);
// d_rows[i] = the verdict on the header of d_jobs[i] (format 1 zlib, 2 gzip with the FHCRC compared); asynchronous on `st`
int header_rows_device(int format, const HeadJob *d_jobs, size_t n, WrapperHead *d_rows, uint8_t *d_work, hipStream_t st);

}  // namespace zr
