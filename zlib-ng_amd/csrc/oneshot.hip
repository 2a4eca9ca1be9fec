// oneshot.hip -- compress2 / uncompress2 class front ends over the device paths:
// zlib (RFC 1950) and gzip (RFC 1952) framing around the raw deflate / inflate kernels, with the trailer
// checksum computed ON DEVICE by the streaming checksum kernel.
//
// Reference behaviour mirrored (zlib-ng 2.2.2):
//   compress2   compress.c:31-69      header deflate.c:868-892 (zlib) / :902-1031 (gzip), trailer :1091-1103
//   uncompress2 uncompr.c:25-76       header checks inflate.c:509-555 ("incorrect header check",
//               "unknown compression method", "invalid window size"), trailer inflate.c:1105-1147
//               ("incorrect data check", "incorrect length check"); a preset dictionary or an incomplete stream
//               is Z_DATA_ERROR for the one-shot caller (uncompr.c:70-75)
// The wrapper rules are framing_parse.h's: the canonical writer at strategy 0, wrapper_parse_whole and wrapper_trailer_verdict.
// `format`: 0 = raw (windowBits -15), 1 = zlib (windowBits 15), 2 = gzip (windowBits 31).
#include "context.h"
#include "deflate_blocks.h"
#include "deflate_index_plan.h"
#include "framing_parse.h"
#include "inflate_dev.h"

#include <vector>

extern "C" int zng_rocm_deflate_dev(int level, const uint8_t *d_in, size_t in_len, uint8_t *d_out, size_t out_cap,
                                    size_t *out_len, void *stream);
extern "C" size_t zng_rocm_deflate_bound(size_t source_len);
extern "C" int zng_rocm_inflate_raw_ex(const uint8_t *src, size_t src_len, uint8_t *d_dst, size_t dst_cap,
                                       uint64_t *out_len, size_t *in_used, void *stream);

namespace zr {

enum { Z_OK_ = 0, Z_STREAM_END_ = 1, Z_STREAM_ERROR_ = -2, Z_DATA_ERROR_ = -3, Z_MEM_ERROR_ = -4, Z_BUF_ERROR_ = -5 };

// adler32 / crc32 of a device buffer, synchronously (the one-shot front ends return a status)
static int device_checks(const uint8_t *d_buf, size_t len, hipStream_t st, uint32_t out[2]) {
    Workspace *ws = workspace_for(st);
    if (!ws) return ZNG_ROCM_ENOMEM;
    int rc = launch_checksum(true, true, 1u, 0u, d_buf, nullptr, len, ws->result, ws->result + 1, st);
    if (rc) return rc;
    ZR_HIP(hipMemcpyAsync(ws->pinned, ws->result, 8, hipMemcpyDeviceToHost, st));
    ZR_HIP(hipStreamSynchronize(st));
    out[0] = ws->pinned[0];
    out[1] = ws->pinned[1];
    return ZNG_ROCM_OK;
}

// zng_rocm_compress2_dev up to its last synchronisation: the checks (deflate_index_plan.h: compress2_check), the trailer's check
// value, the deflate data, header and trailer.  *total = the stream's bytes; *dst_len is the caller's to write.  rows (or null):
// the block rows of levels 1..9 for zng_rocm_compress2_index_dev (deflate_blocks.h: deflate_rows_points_dev); with null the
// deflate data comes from zng_rocm_deflate_dev -- the same engine behind the same checks.
static int compress2_run(uint8_t *d_dst, const size_t *dst_len, const uint8_t *d_src, size_t src_len, int level, int format, void *stream,
                         std::vector<uint64_t> *rows, size_t *total) {
    const Compress2Refusal why = compress2_check(ctx() != nullptr, !d_dst || !dst_len || (!d_src && src_len), format, level,
                                                 dst_len ? *dst_len : 0u, src_len);
    if (why == kC2NoDevice) set_error("zng_rocm_init() has not succeeded");
    else if (why == kC2Level) set_error("level %d is outside -1..9", level);           // deflateInit2: Z_STREAM_ERROR (deflate.c:318-320)
    else if (why == kC2Bound) set_error("destination smaller than zng_rocm_compress_bound()");
    if (why) return compress2_status(why);
    DeviceGuard dev;
    level = compress2_level(level);
    hipStream_t st = (hipStream_t)stream;
    const size_t head = wrapper_head_bytes(format), trail = wrapper_tail_bytes(format);
    uint32_t chk[2] = {1u, 0u};
    if (format) {
        int rc = device_checks(d_src, src_len, st, chk);
        if (rc) return rc;
    }
    size_t body = 0;
    int rc = rows ? deflate_rows_points_dev(level, d_src, src_len, d_dst + head, *dst_len - head - trail, &body, *rows, st)
                  : zng_rocm_deflate_dev(level, d_src, src_len, d_dst + head, *dst_len - head - trail, &body, stream);
    if (rc) return rc;
    uint8_t h[10], t[8];                                          // deflate.c:868-885 / :902-916 with the level's hint, :1091-1103
    for (uint32_t k = 0; k < head; ++k) h[k] = wrapper_header_byte(format, level, 0, k);
    for (uint32_t k = 0; k < trail; ++k) t[k] = wrapper_trailer_byte(format, k, chk[format == 1 ? 0 : 1], (uint32_t)src_len);
    if (head) ZR_HIP(hipMemcpyAsync(d_dst, h, head, hipMemcpyHostToDevice, st));
    if (trail) ZR_HIP(hipMemcpyAsync(d_dst + head + body, t, trail, hipMemcpyHostToDevice, st));
    ZR_HIP(hipStreamSynchronize(st));
    *total = head + body + trail;
    return Z_OK_;
}

}  // namespace zr

using namespace zr;

extern "C" {

size_t zng_rocm_compress_bound(size_t source_len, int format) {
    // compressBound (compress.c:81-98): raw bound + wrapper (ZLIB_WRAPLEN 6, GZIP_WRAPLEN 18; zutil.h:68-69)
    return zng_rocm_deflate_bound(source_len) + (format == 1 ? 6 : format == 2 ? 18 : 0);
}

int zng_rocm_compress2_dev(uint8_t *d_dst, size_t *dst_len, const uint8_t *d_src, size_t src_len, int level,
                           int format, void *stream) {
    size_t total = 0;
    if (int rc = compress2_run(d_dst, dst_len, d_src, src_len, level, format, stream, nullptr, &total)) return rc;
    *dst_len = total;
    return Z_OK_;
}

// The same stream with a zng_rocm_inflate_index of it, and no byte of it decoded (deflate_index_plan.h): every block start is a
// candidate -- the rows engine's blocks from rows_block_points_kernel's readback, level 0's in closed form -- index_select thins
// them to span_bytes, and the windows are gathered from the PLAINTEXT.
int zng_rocm_compress2_index_dev(uint8_t *d_dst, size_t *dst_len, const uint8_t *d_src, size_t src_len, int level, int format,
                                 uint64_t span_bytes, zng_rocm_inflate_index **out, void *stream) {
    if (out) *out = nullptr;
    const bool null_args = !d_dst || !dst_len || (!d_src && src_len);
    if (deflate_index_check(span_bytes, !out, ctx() != nullptr, null_args, format, level, dst_len ? *dst_len : 0u, src_len) == kC2SpanOrOut) {
        set_error("zng_rocm_compress2_index_dev: a null result pointer, or span_bytes outside 64 KiB .. 1 GiB");
        return ZNG_ROCM_EINVAL;
    }
    std::vector<uint64_t> rows;
    size_t total = 0;
    if (int rc = compress2_run(d_dst, dst_len, d_src, src_len, level, format, stream, &rows, &total)) return rc;
    const uint64_t head = wrapper_head_bytes(format);
    std::vector<IndexCand> cands;
    if (compress2_level(level) == 0) deflate_index_stored_cands(src_len, head, cands);
    else deflate_index_rows_cands(rows.data(), rows.size() / 2, head, cands);
    const IndexHead ih = {(uint32_t)format, head, (uint64_t)total, (uint64_t)src_len, index_span_bytes(span_bytes)};
    if (int rc = inflate_index_from_cands("zng_rocm_compress2_index_dev", ih, cands.data(), cands.size(), d_src, (hipStream_t)stream, out))
        return rc;
    *dst_len = total;
    return Z_OK_;
}

int zng_rocm_uncompress2_dev(uint8_t *d_dst, size_t *dst_len, const uint8_t *src, size_t *src_len, int format,
                             void *stream) {
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    DeviceGuard dev;
    if (!dst_len || !src_len || (!src && *src_len) || format < 0 || format > 2) return ZNG_ROCM_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = *src_len;
    const WholeHead w = wrapper_parse_whole(format, HostBytes{src}, n, ctx()->host_tables.byte_tab);
    if (w.msg != kMsgNone) {
        if (w.msg == kMsgStarved) set_error("input ended inside the %s header", format == 1 ? "zlib" : "gzip");
        else if (w.msg == kMsgNeedDict) set_error("preset dictionary required");     // Z_NEED_DICT -> uncompr.c:72
        else set_error("%s", wrapper_message(w.wrap_msg));                           // unknown flag bits keep their own text
        return Z_DATA_ERROR_;
    }
    const size_t pos = (size_t)w.header_len, trail = wrapper_tail_bytes(format);
    uint64_t got = 0;
    size_t used = 0;
    int rc = zng_rocm_inflate_raw_ex(src + pos, n - pos, d_dst, *dst_len, &got, &used, stream);
    if (rc == Z_BUF_ERROR_ && got > *dst_len) return Z_BUF_ERROR_;              // destination too small
    if (rc == Z_DATA_ERROR_) return Z_DATA_ERROR_;                              // message already set (strm->msg text)
    if (rc != Z_STREAM_END_) {
        if (rc == Z_OK_ || rc == Z_BUF_ERROR_) { set_error("incomplete stream"); return Z_DATA_ERROR_; }   // uncompr.c:73-74
        return rc;
    }
    if (pos + used + trail > n) { set_error("incomplete stream"); return Z_DATA_ERROR_; }
    if (format) {
        uint32_t chk[2];
        rc = device_checks(d_dst, (size_t)got, st, chk);
        if (rc) return rc;
        if (const uint32_t verdict = wrapper_trailer_verdict(format, src + pos + used, chk[0], chk[1], got)) {
            set_error("%s", wrapper_message(verdict));
            return Z_DATA_ERROR_;
        }
    }
    *dst_len = (size_t)got;
    *src_len = pos + used + trail;
    return Z_OK_;
}

}  // extern "C"
