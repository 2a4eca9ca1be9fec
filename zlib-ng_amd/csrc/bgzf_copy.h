// bgzf_copy.h -- the byte-granular mover that bgzf.hip (a payload to its byte in the file) and bgzf_read.hip (a slice of a
// decoded member to its byte in a caller's buffer) share: any source alignment, any destination alignment, nothing written
// outside the destination's bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deflate_dev.h"

namespace zr {

typedef uint32_t u32x4_line __attribute__((ext_vector_type(4)));      // a whole 16-byte line: one aligned dwordx4 store

// n bytes from src to dst[at, at + n) by the 256 lanes of a workgroup, cut at dst[cap): bytes up to the destination's next
// 16-byte line, then 16 bytes per lane (the source read at whatever alignment it has), then bytes
__device__ __forceinline__ void bgzf_copy(uint8_t *dst, unsigned long long at, unsigned long long cap, const uint8_t *src,
                                          uint32_t n, int t) {
    if (at >= cap) return;
    if (cap - at < n) n = (uint32_t)(cap - at);
    uint8_t *d = dst + at;
    uint32_t head = (uint32_t)((16u - ((uintptr_t)d & 15u)) & 15u);
    if (head > n) head = n;
    if ((uint32_t)t < head) d[t] = load_u8(src + t);
    const uint32_t lines = (n - head) >> 4;
    for (uint32_t i = (uint32_t)t; i < lines; i += 256u) {
        const u32x4_unaligned v = load_u128(src + head + 16u * i);
        *(ZR_GLOBAL u32x4_line *)(d + head + 16u * i) = v;
    }
    const uint32_t done = head + 16u * lines;
    if ((uint32_t)t < n - done) d[done + t] = load_u8(src + done + t);
}

}  // namespace zr
