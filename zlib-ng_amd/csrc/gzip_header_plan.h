// gzip_header_plan.h -- the gzip header FIELDS of RFC 1952 2.3 for the members the device writes and reads: deflateSetHeader
// and inflateGetHeader (zlib-ng.h.in:127-141 the zng_gz_header, :796-816, :1020-1055) for zng_rocm_compress_streams2_header_dev /
// zng_rocm_compress_members_header_dev (compress_streams.hip) and zng_rocm_gzip_headers_dev (gzip_header.hip).  Plain C++ marked
// ZR_HD, no HIP; tests/test_gzip_header_plan_cpu.py drives it through tests/c/gzip_header_plan_driver.cpp without a GPU.
//   gh_check, gh_bytes   what is refused, and the header's length without rendering it
//   gh_render            the bytes deflate.c:923-1020 writes: 1f 8b 08 | FLG | MTIME | XFL | OS | XLEN extra | name 0 | comment 0 |
//                        FHCRC.  A null header is the canonical 10 bytes of wrapper_header_byte (deflate.c:902-913).
//   gh_walk              the reader: wrapper_parse_rules(2, ...) decides -- status, message, header_len are its own, nothing is
//                        judged here -- and gh_locate then finds the fields of a header the rules accepted.  A template over
//                        the Bytes concept of framing_parse.h, so that the host walks with memchr and the device with a wavefront.
//   gh_hcrc_bad          is the stored FHCRC not the header's?  (the caller evaluates the CRC-32: the host
//                        with wrapper_host_crc32, the device with the many-message checksum pass)
//   gh_gather_len, gh_gather_layout   the fields of the accepted members, one behind the other, in `text`
// Where this differs from the reference on purpose: deflate.c:947-949 writes extra_len & 0xffff as XLEN and then copies
// extra_len bytes, so an extra_len above 65535 makes a header no reader follows; here it is refused.  zlib has no limit for name
// and comment; the 65535 bytes here are the library's own and bound a header at kGhMaxBytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/zng_rocm.h"
#include "framing_parse.h"
#include "gf2.h"      // ZR_HD

namespace zr {

constexpr uint32_t kGhFieldMax = 65535u;              // extra_len (XLEN is 16 bits); name and comment without their terminator
constexpr uint32_t kGhFixed = 10u;                    // ID1 ID2 CM FLG MTIME XFL OS
constexpr uint32_t kGhMaxBytes = kGhFixed + 2u + kGhFieldMax + 2u * (kGhFieldMax + 1u) + 2u;     // 196621
constexpr uint32_t kGhText = 1u, kGhHcrc = 2u, kGhExtra = 4u, kGhName = 8u, kGhComment = 16u;  // FLG (RFC 1952 2.3.1)

// ---- the writer ---------------------------------------------------------------------------------------------------------------
struct GhLens {                                       // of a header gh_check accepted
    uint32_t extra, name, comment;                    // name / comment without the terminator
};

// 0, or ZNG_ROCM_EINVAL: extra_len above 65535, extra_len without extra, a name or comment of more than 65535 bytes, reserved != 0
inline int gh_check(const zng_rocm_gzip_header *h, GhLens *lens) {
    GhLens l = {0u, 0u, 0u};
    if (h) {
        if (h->reserved || h->extra_len > kGhFieldMax || (!h->extra && h->extra_len)) return ZNG_ROCM_EINVAL;
        l.extra = h->extra_len;
        if (h->name && (l.name = (uint32_t)strnlen(h->name, (size_t)kGhFieldMax + 1u)) > kGhFieldMax) return ZNG_ROCM_EINVAL;
        if (h->comment && (l.comment = (uint32_t)strnlen(h->comment, (size_t)kGhFieldMax + 1u)) > kGhFieldMax) return ZNG_ROCM_EINVAL;
    }
    if (lens) *lens = l;
    return ZNG_ROCM_OK;
}

inline uint32_t gh_flg(const zng_rocm_gzip_header *h) {
    return !h ? 0u : (h->text ? kGhText : 0u) | (h->hcrc ? kGhHcrc : 0u) | (h->extra ? kGhExtra : 0u) | (h->name ? kGhName : 0u) |
                         (h->comment ? kGhComment : 0u);
}

// bytes of the header gh_render writes (h accepted by gh_check, which gave lens); a null header: the canonical 10
inline uint32_t gh_bytes(const zng_rocm_gzip_header *h, const GhLens &lens) {
    if (!h) return wrapper_head_bytes(2);
    return kGhFixed + (h->extra ? 2u + lens.extra : 0u) + (h->name ? lens.name + 1u : 0u) + (h->comment ? lens.comment + 1u : 0u) +
           (h->hcrc ? 2u : 0u);
}

// deflate.c:923-1020 into out[0, gh_bytes): level is 0..9
inline void gh_render(const zng_rocm_gzip_header *h, const GhLens &lens, int level, int strategy, uint8_t *out) {
    for (uint32_t k = 0; k < kGhFixed; ++k) out[k] = wrapper_header_byte(2, level, strategy, k);     // magic, method, XFL; a null header whole
    if (!h) return;
    out[3] = (uint8_t)gh_flg(h);
    for (uint32_t k = 0; k < 4u; ++k) out[4u + k] = (uint8_t)(h->time >> (8u * k));
    out[9] = (uint8_t)(h->os & 0xffu);
    uint32_t pos = kGhFixed;
    if (h->extra) {
        out[pos] = (uint8_t)(lens.extra & 0xffu);
        out[pos + 1u] = (uint8_t)(lens.extra >> 8);
        if (lens.extra) memcpy(out + pos + 2u, h->extra, lens.extra);
        pos += 2u + lens.extra;
    }
    if (h->name) {
        memcpy(out + pos, h->name, (size_t)lens.name + 1u);
        pos += lens.name + 1u;
    }
    if (h->comment) {
        memcpy(out + pos, h->comment, (size_t)lens.comment + 1u);
        pos += lens.comment + 1u;
    }
    if (h->hcrc) {                                    // deflate.c:1005-1016: the low 16 bits of the CRC-32 of everything in front
        const uint32_t crc = wrapper_host_crc32(out, pos);
        out[pos] = (uint8_t)(crc & 0xffu);
        out[pos + 1u] = (uint8_t)((crc >> 8) & 0xffu);
    }
}

// ---- the reader ---------------------------------------------------------------------------------------------------------------
struct GhRow {                                        // one member's header as the kernels hand it down; offsets count from the member
    uint64_t header_len;
    uint64_t extra_off, name_off, comment_off;        // 0: the field is absent
    uint64_t text_off;                                // gh_gather_layout / the scan kernel
    int32_t  status;                                  // wrapper_parse_rules': 0, -3, -5
    uint32_t msg;                                     // WrapMsg
    uint32_t flg, time, xflags, os;
    uint32_t extra_len, name_len, comment_len;
    uint32_t hcrc_stored;                             // FLG & 2: what the header stores, to be compared by the caller
};

ZR_HD GhRow gh_row_refused(int32_t status, uint32_t msg) {
    GhRow r = {0, 0, 0, 0, 0, status, msg, 0, 0, 0, 0, 0, 0, 0, 0};
    return r;
}

// the fields of a header the rules accepted (h.status == 0): nothing is judged, every byte read lies in front of h.header_len.
// The one search is for the name's terminator where a comment follows it; every other length follows from header_len.
template <class Bytes>
ZR_HD GhRow gh_locate(const Bytes &in, const WrapperHead &h) {
    GhRow r = gh_row_refused(0, kWrapNone);
    r.header_len = h.header_len;
    r.flg = in.byte(3);
    r.time = in.byte(4) | (in.byte(5) << 8) | (in.byte(6) << 16) | (in.byte(7) << 24);
    r.xflags = in.byte(8);
    r.os = in.byte(9);
    r.hcrc_stored = h.hcrc_stored;
    uint64_t pos = kGhFixed;
    const uint64_t end = h.header_len - (h.hcrc ? 2u : 0u);      // behind the last field
    if (r.flg & kGhExtra) {
        r.extra_len = in.byte(10) | (in.byte(11) << 8);
        r.extra_off = 12;
        pos = 12u + r.extra_len;
    }
    if (r.flg & kGhName) {
        r.name_off = pos;
        const uint64_t z = (r.flg & kGhComment) ? in.find_zero(pos, end) : end - 1u;
        r.name_len = (uint32_t)(z - pos);
        pos = z + 1u;
    }
    if (r.flg & kGhComment) {
        r.comment_off = pos;
        r.comment_len = (uint32_t)(end - 1u - pos);
    }
    return r;
}

// n: bytes of the member that exist.  The FHCRC is not evaluated here (gh_hcrc_bad)
template <class Bytes>
ZR_HD GhRow gh_walk(const Bytes &in, uint64_t n) {
    const WrapperHead h = wrapper_parse_rules(2, in, n);
    return h.status == 0 ? gh_locate(in, h) : gh_row_refused(h.status, h.msg);
}

// does the caller have a CRC-32 to take, and over how many bytes (inflate.c:686-692)
ZR_HD uint64_t gh_hcrc_bytes(const GhRow &r) { return r.status == 0 && (r.flg & kGhHcrc) ? r.header_len - 2u : 0u; }
// crc: the CRC-32 of the member's first gh_hcrc_bytes bytes.  true: the row becomes gh_row_hcrc_refused()
ZR_HD bool gh_hcrc_bad(const GhRow &r, uint32_t crc) { return gh_hcrc_bytes(r) && (crc & 0xffffu) != r.hcrc_stored; }
ZR_HD GhRow gh_row_hcrc_refused() { return gh_row_refused(-3, kWrapHeaderCrc); }

// the host's walk: rules, fields, FHCRC
inline GhRow gh_parse_host(const uint8_t *src, uint64_t n) {
    const GhRow r = gh_walk(HostBytes{src}, n);
    return gh_hcrc_bad(r, wrapper_host_crc32(src, (size_t)gh_hcrc_bytes(r))) ? gh_row_hcrc_refused() : r;
}

// the row callers see; member_off: the member's first byte in the file
inline void gh_row_public(const GhRow &r, uint64_t member_off, zng_rocm_gzip_header_row *out) {
    out->status = r.status;
    out->flg = r.flg;
    out->msg = r.status == -3 ? wrapper_message(r.msg) : nullptr;
    out->header_len = r.header_len;
    out->time = r.time;
    out->xflags = r.xflags;
    out->os = r.os;
    out->text = r.flg & kGhText ? 1u : 0u;
    out->hcrc = r.flg & kGhHcrc ? 1u : 0u;
    out->extra_len = r.extra_len;
    out->name_len = r.name_len;
    out->comment_len = r.comment_len;
    out->extra_off = r.extra_off ? member_off + r.extra_off : 0u;
    out->name_off = r.name_off ? member_off + r.name_off : 0u;
    out->comment_off = r.comment_off ? member_off + r.comment_off : 0u;
    out->text_off = r.text_off;
}

// ---- the gather ---------------------------------------------------------------------------------------------------------------
// what a member puts into `text`: its extra bytes, then name and a 0, then comment and a 0 -- the fields it has; a refused or cut
// member puts nothing
ZR_HD uint64_t gh_gather_len(const GhRow &r) {
    if (r.status != 0) return 0u;
    return (uint64_t)r.extra_len + (r.name_off ? (uint64_t)r.name_len + 1u : 0u) + (r.comment_off ? (uint64_t)r.comment_len + 1u : 0u);
}
// text_off of every row in member order (the running sum the scan kernel takes); returns the bytes `text` needs
inline uint64_t gh_gather_layout(GhRow *rows, uint64_t n) {
    uint64_t need = 0;
    for (uint64_t i = 0; i < n; ++i) {
        rows[i].text_off = need;
        need += gh_gather_len(rows[i]);
    }
    return need;
}

}  // namespace zr
