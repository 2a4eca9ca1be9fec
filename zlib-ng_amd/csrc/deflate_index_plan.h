// deflate_index_plan.h -- the host rules of zng_rocm_compress2_index_dev (oneshot.hip): zng_rocm_compress2_dev that hands back a
// zng_rocm_inflate_index of the stream it writes, taken from what the compressor knows instead of from a decode.  Plain C++
// over integers, no HIP: the order in which the call refuses, the block starts of a level-0 stream in closed form, the rows
// rows_block_points_kernel (deflate_dyn.hip) leaves per block turned into the candidates index_select (inflate_index_plan.h)
// walks, and the bound on a span's length as a function that can be checked.  tests/test_deflate_index_plan_cpu.py drives
// them through tests/c/deflate_index_plan_driver.cpp without a GPU.
//
// Every block of the stream is a candidate {bit of the FILE where it begins, plaintext offset of its first byte}, in stream
// order.  Both writers end every block on a byte boundary, so the bit is 8 * (header_len + the block's byte in the deflate
// data):
//   levels 1..9   block k of the rows engine: {8 * (header_len + dst_off[k]), lo_k}; lo_k is the first byte emit_dynamic_kernel
//                 codes for it -- blo_k if a token starts there, else the next token start of the segment
//   level 0       stored block j: {8 * (header_len + 65540 * j), 65535 * j}
// THE BOUND: two neighbouring candidates are at most kDeflateIndexStep = 61440 + 257 plaintext bytes apart at levels 1..9 (a
// block takes the tokens that start in 61440 positions, and the token in front of it reaches at most 257 bytes in), exactly
// 65535 at level 0, and the last one is as close to plain_len.  index_select takes the first candidate that is span_bytes
// past the last point, so   out_off[k + 1] - out_off[k] < span_bytes + 65536   and   plain_len - out_off[last] < span_bytes + 65536.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "deflate_rows_plan.h"       // rows_deflate_bound, kSubBytes
#include "inflate_index_plan.h"      // index_span_bytes, IndexCand

namespace zr {

constexpr uint32_t kStoredBlock = 65535u;                     // MAX_STORED: plaintext per level-0 block, 5 bytes of header each
constexpr uint32_t kDeflateIndexStep = kSubBytes + 257u;      // the most between two neighbouring candidates, levels 1..9
constexpr uint64_t kDeflateIndexSlack = 65536u;               // what a span may be longer than span_bytes by: above both steps
static_assert(kDeflateIndexStep < kDeflateIndexSlack && kStoredBlock < kDeflateIndexSlack, "the span bound of the header comment");

// ---- the refusals, in the order the calls look ----------------------------------------------------------------------------------
enum Compress2Refusal {
    kC2Taken = 0,
    kC2SpanOrOut,       // zng_rocm_compress2_index_dev alone, before everything else: ZNG_ROCM_EINVAL, nothing looked at or written
    kC2NoDevice,        // ZNG_ROCM_ENODEV
    kC2Args,            // a null buffer, a format outside 0..2: ZNG_ROCM_EINVAL
    kC2Level,           // outside -1..9: Z_STREAM_ERROR
    kC2Bound            // *dst_len below zng_rocm_compress_bound(): Z_BUF_ERROR
};
inline int compress2_status(Compress2Refusal r) {
    switch (r) {
    case kC2Taken: return ZNG_ROCM_OK;
    case kC2NoDevice: return ZNG_ROCM_ENODEV;
    case kC2Level: return -2;
    case kC2Bound: return -5;
    default: return ZNG_ROCM_EINVAL;
    }
}
inline int compress2_level(int level) { return level == -1 ? 6 : level; }      // Z_DEFAULT_COMPRESSION (deflate.c:296)
// compressBound (compress.c:81-98): the raw bound + ZLIB_WRAPLEN 6 / GZIP_WRAPLEN 18 (zutil.h:68-69)
inline uint64_t compress2_bound(uint64_t src_len, int format) {
    return rows_deflate_bound(src_len) + (format == 1 ? 6u : format == 2 ? 18u : 0u);
}
// zng_rocm_compress2_dev.  null_args: d_dst or dst_len is null, or d_src is with a length; dst_len: *dst_len (when there is one)
inline Compress2Refusal compress2_check(bool have_device, bool null_args, int format, int level, uint64_t dst_len, uint64_t src_len) {
    if (!have_device) return kC2NoDevice;
    if (null_args || format < 0 || format > 2) return kC2Args;
    level = compress2_level(level);
    if (level < 0 || level > 9) return kC2Level;
    if (dst_len < compress2_bound(src_len, format)) return kC2Bound;
    return kC2Taken;
}
// zng_rocm_compress2_index_dev: its own refusal first, then that call's
inline Compress2Refusal deflate_index_check(uint64_t span_bytes, bool out_null, bool have_device, bool null_args, int format, int level,
                                            uint64_t dst_len, uint64_t src_len) {
    if (out_null || !index_span_bytes(span_bytes)) return kC2SpanOrOut;
    return compress2_check(have_device, null_args, format, level, dst_len, src_len);
}

// ---- the candidates ----------------------------------------------------------------------------------------------------------------
// level 0 (stored_kernel): a block per 65535 bytes, an empty stream is one empty block
inline uint64_t stored_blocks(uint64_t src_len) { return src_len ? (src_len + kStoredBlock - 1) / kStoredBlock : 1u; }
inline void deflate_index_stored_cands(uint64_t src_len, uint64_t header_len, std::vector<IndexCand> &cands) {
    const uint64_t n = stored_blocks(src_len);
    cands.resize((size_t)n);
    for (uint64_t j = 0; j < n; ++j) cands[(size_t)j] = IndexCand{8 * (header_len + (kStoredBlock + 5ull) * j), (uint64_t)kStoredBlock * j};
}
// levels 1..9: rows[2 * k] = dst_off[k], rows[2 * k + 1] = lo_k of block k (rows_block_points_kernel)
inline void deflate_index_rows_cands(const uint64_t *rows, size_t nblk, uint64_t header_len, std::vector<IndexCand> &cands) {
    cands.resize(nblk);
    for (size_t k = 0; k < nblk; ++k) cands[k] = IndexCand{8 * (header_len + rows[2 * k]), rows[2 * k + 1]};
}

// ---- the bound ---------------------------------------------------------------------------------------------------------------------
// every span of pts[0, n), the last one up to plain_len, is shorter than span + kDeflateIndexSlack; -1, or the first span that is not
inline int64_t deflate_index_span_bound(const zng_rocm_access_point *pts, size_t n, uint64_t plain_len, uint64_t span) {
    for (size_t k = 0; k < n; ++k) {
        const uint64_t end = k + 1 < n ? pts[k + 1].out_off : plain_len;
        if (end < pts[k].out_off || end - pts[k].out_off >= span + kDeflateIndexSlack) return (int64_t)k;
    }
    return -1;
}

}  // namespace zr
