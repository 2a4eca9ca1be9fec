// framing_parse.h -- the rules of the zlib (RFC 1950) and gzip (RFC 1952) wrappers, ONCE, for host and device and for every
// caller: what inflate() does in its HEAD .. HCRC and DICTID states (inflate.c:509-555 zlib, :556-700 gzip, :702-715
// dictionary id) and behind the deflate data (inflate.c:1105-1147) on a member that is all in memory, and what deflate()
// writes around it (deflate.c:868-916 header, :1091-1103 trailer).  Plain C++ marked ZR_HD, no HIP.
//   wrapper_parse_rules      the header.  A template over the way the bytes are reached, so that zng_rocm_wrapper_parse walks
//                            host memory with memchr while the header kernel of framing_large.hip searches the terminators of
//                            FNAME / FCOMMENT with a whole wavefront; the ORDER of the checks and their answers are written
//                            here only.  It does not evaluate the FHCRC: it says where the stored 16 bits were and over how
//                            many bytes they are taken, and the caller compares (the large calls with the many-message
//                            checksum pass).
//   wrapper_parse_whole      the verdict of the callers that hold a whole member and no dictionary
//                            (zng_rocm_uncompress_streams_dev, zng_rocm_uncompress2_dev): the rules, the FHCRC by a table
//                            walk, and the two places where these callers answer differently from the rules
//   wrapper_trailer_verdict  check value and ISIZE: the one place where the compare order lives
//   wrapper_header_byte, wrapper_trailer_byte   the canonical header and trailer of the writers, by format, level and strategy
//   wrapper_dict_head_bytes, wrapper_dict_header_byte   the 6-byte zlib header with FDICT and the DICTID
//   wrapper_le32, wrapper_be32, wrapper_head_bytes, wrapper_tail_bytes   the 32-bit fields and the canonical sizes
//   wrapper_host_crc32       the FHCRC's CRC-32 for the host-only callers
#pragma once
#include <stdint.h>
#include <string.h>

#include "gf2.h"      // ZR_HD
#include "inflate_dev_types.h"

namespace zr {

// ---- fields and sizes ---------------------------------------------------------------------------------------------------------
// four bytes as gzip stores them (least significant first) and as zlib does (most significant first)
ZR_HD uint32_t wrapper_le32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
ZR_HD uint32_t wrapper_be32(const uint8_t *p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// the canonical wrapper (no optional field): bytes in front of and behind the deflate data.  format: 0 raw, 1 zlib, 2 gzip
ZR_HD uint32_t wrapper_head_bytes(int format) { return format == 1 ? 2u : format == 2 ? 10u : 0u; }
ZR_HD uint32_t wrapper_tail_bytes(int format) { return format == 1 ? 4u : format == 2 ? 8u : 0u; }

// ---- the writer ---------------------------------------------------------------------------------------------------------------
// FLEVEL of the zlib header (deflate.c:873-880) and XFL of the gzip header (deflate.c:911-912); level is 0 .. 9
ZR_HD uint32_t wrapper_zlib_flevel(int level, int strategy) {
    return (strategy >= 2 || level < 2) ? 0u : level < 6 ? 1u : level == 6 ? 2u : 3u;
}
ZR_HD uint32_t wrapper_gzip_xfl(int level, int strategy) { return level == 9 ? 2u : (strategy >= 2 || level < 2) ? 4u : 0u; }

// byte k (0 .. wrapper_head_bytes - 1) of the header.  window_bits: the stream's w_bits, 9..15 (deflate.c:870: CINFO = w_bits - 8;
// the writers without a window say nothing and mean 15); gzip has no window field
ZR_HD uint8_t wrapper_header_byte(int format, int level, int strategy, uint32_t k, int window_bits = 15) {
    if (format == 1) {
        uint32_t header = ((8u + ((uint32_t)(window_bits - 8) << 4)) << 8) | (wrapper_zlib_flevel(level, strategy) << 6);     // Z_DEFLATED, w_bits
        header += 31u - header % 31u;
        return (uint8_t)(header >> (k == 0u ? 8 : 0));
    }
    // gzip: ID1 ID2 CM FLG | MTIME x 4 | XFL OS
    return k == 0u ? (uint8_t)0x1fu : k == 1u ? (uint8_t)0x8bu : k == 2u ? (uint8_t)8u : k == 8u ? (uint8_t)wrapper_gzip_xfl(level, strategy)
         : k == 9u ? (uint8_t)3u : (uint8_t)0u;
}
// The zlib header of a stream with a preset dictionary (deflate.c:868-892): CMF FLG as above with FDICT set -- FCHECK makes
// the pair a multiple of 31 with the bit in it --, then the DICTID, most significant byte first.  Formats without a dictionary
// (raw: deflateSetDictionary leaves no trace in the stream; gzip has none, deflate.c:467) have no such header.
ZR_HD uint32_t wrapper_dict_head_bytes(int format) { return format == 1 ? 6u : 0u; }
// byte k (0 .. 5) of it
ZR_HD uint8_t wrapper_dict_header_byte(int level, int strategy, uint32_t dictid, uint32_t k) {
    if (k >= 2u) return (uint8_t)(dictid >> (8u * (5u - k)));
    uint32_t header = ((8u + (7u << 4)) << 8) | (wrapper_zlib_flevel(level, strategy) << 6) | 0x20u;     // PRESET_DICT
    header += 31u - header % 31u;
    return (uint8_t)(header >> (k == 0u ? 8 : 0));
}
// byte k (0 .. wrapper_tail_bytes - 1) of the trailer around n plaintext bytes whose check value (Adler-32; gzip: CRC-32) is
// `check`: zlib most significant byte first (deflate.c:1098-1101), gzip CRC-32 then ISIZE, least significant first (:1091-1096)
ZR_HD uint8_t wrapper_trailer_byte(int format, uint32_t k, uint32_t check, uint32_t n) {
    if (format == 1) return (uint8_t)(check >> (8u * (3u - k)));
    return (uint8_t)((k < 4u ? check : n) >> (8u * (k & 3u)));
}

// ---- the reader ---------------------------------------------------------------------------------------------------------------

// message ids of the wrapped large calls (texts: wrapper_message)
enum WrapMsg : uint32_t {
    kWrapNone = 0,
    kWrapHeaderCheck,       // "incorrect header check"       inflate.c:527-533
    kWrapMethod,            // "unknown compression method"   inflate.c:534-538, :561-565
    kWrapWindow,            // "invalid window size"          inflate.c:541-546
    kWrapFlags,             // "unknown header flags set"     inflate.c:565-567
    kWrapHeaderCrc,         // "header crc mismatch"          inflate.c:686-692
    kWrapDataCheck,         // "incorrect data check"         inflate.c:1132
    kWrapLengthCheck,       // "incorrect length check"       inflate.c:1146
    kWrapMsgCount
};

inline const char *wrapper_message(uint32_t id) {
    static const char *const text[kWrapMsgCount] = {nullptr, "incorrect header check", "unknown compression method",
                                                    "invalid window size", "unknown header flags set", "header crc mismatch",
                                                    "incorrect data check", "incorrect length check"};
    return id < kWrapMsgCount ? text[id] : nullptr;
}

struct WrapperHead {
    uint64_t header_len;    // status 0: bytes in front of the raw deflate payload
    int32_t  status;        // 0 accepted, -3 refused (msg), -5 the input ends inside the header
    uint32_t msg;           // WrapMsg
    uint32_t dictid;        // zlib with FDICT: the Adler-32 the dictionary must have
    uint32_t fdict;         // 1: the zlib header announces a preset dictionary
    uint32_t hcrc;          // 1: gzip FHCRC -- hcrc_stored must equal the low 16 bits of the CRC-32 of [0, header_len - 2)
    uint32_t hcrc_stored;
};

// Bytes: `uint32_t byte(uint64_t pos) const` and `uint64_t find_zero(uint64_t from, uint64_t n) const` (the position of
// the first zero byte in [from, n), or n).  format: 1 zlib, 2 gzip (0: no wrapper).  n: bytes of the member that exist.
template <class Bytes>
ZR_HD WrapperHead wrapper_parse_rules(int format, const Bytes &in, uint64_t n) {
    WrapperHead h = {0, 0, kWrapNone, 0, 0, 0, 0};
    if (format == 1) {                                   // inflate.c:509-555 with windowBits 15
        if (n < 2) { h.status = -5; return h; }
        const uint32_t cmf = in.byte(0), flg = in.byte(1);
        if (((cmf << 8) | flg) % 31u) h.msg = kWrapHeaderCheck;
        else if ((cmf & 15u) != 8u) h.msg = kWrapMethod;
        else if ((cmf >> 4) + 8u > 15u) h.msg = kWrapWindow;
        if (h.msg) { h.status = -3; return h; }
        h.header_len = 2;
        if (flg & 0x20u) {                               // DICTID, inflate.c:702-715
            if (n < 6) { h.status = -5; return h; }
            h.dictid = (in.byte(2) << 24) | (in.byte(3) << 16) | (in.byte(4) << 8) | in.byte(5);
            h.fdict = 1;
            h.header_len = 6;
        }
    } else if (format == 2) {                            // inflate.c:556-700; every field is judged as soon as it is complete
        if (n < 2) { h.status = -5; return h; }
        if (in.byte(0) != 0x1fu || in.byte(1) != 0x8bu) { h.status = -3; h.msg = kWrapHeaderCheck; return h; }
        if (n < 4) { h.status = -5; return h; }
        const uint32_t flags = in.byte(3);
        if (in.byte(2) != 8u) h.msg = kWrapMethod;
        else if (flags & 0xe0u) h.msg = kWrapFlags;
        if (h.msg) { h.status = -3; return h; }
        if (n < 10) { h.status = -5; return h; }         // MTIME, XFL, OS: any value
        uint64_t pos = 10;
        if (flags & 4u) {                                // FEXTRA: XLEN and that many bytes
            if (n < 12) { h.status = -5; return h; }
            pos = 12u + (in.byte(10) | (in.byte(11) << 8));
            if (pos > n) { h.status = -5; return h; }
        }
        for (uint32_t bit = 8; bit <= 16; bit <<= 1) {   // FNAME, FCOMMENT: zero-terminated
            if (!(flags & bit)) continue;
            const uint64_t z = in.find_zero(pos, n);
            if (z >= n) { h.status = -5; return h; }
            pos = z + 1;
        }
        if (flags & 2u) {                                // FHCRC
            if (pos + 2 > n) { h.status = -5; return h; }
            h.hcrc = 1;
            h.hcrc_stored = in.byte(pos) | (in.byte(pos + 1) << 8);
            pos += 2;
        }
        h.header_len = pos;
    }
    return h;
}

// the messages as the device calls' result rows carry them (inflate_dev_types.h).  Unknown flag bits are a header check failure
// there: zng_rocm_uncompress_streams_dev has said "incorrect header check" for them from its first day
ZR_HD uint32_t wrapper_inflate_msg(uint32_t wrap_msg) {
    switch (wrap_msg) {
    case kWrapHeaderCheck: case kWrapFlags: return kMsgHeaderCheck;
    case kWrapMethod: return kMsgMethod;
    case kWrapWindow: return kMsgWindow;
    case kWrapHeaderCrc: return kMsgHeaderCrc;
    case kWrapDataCheck: return kMsgDataCheck;
    case kWrapLengthCheck: return kMsgLengthCheck;
    default: return kMsgNone;
    }
}

// inflate.c:1105-1147: the trailer at t (wrapper_tail_bytes(format) bytes) against the check values of the out_len bytes that
// were decoded -- zlib's stored Adler-32, then gzip's CRC-32, then ISIZE against the low 32 bits of the length
ZR_HD uint32_t wrapper_trailer_verdict(int format, const uint8_t *t, uint32_t adler, uint32_t crc, uint64_t out_len) {
    if (format == 1) return wrapper_be32(t) != adler ? kWrapDataCheck : kWrapNone;
    if (format != 2) return kWrapNone;
    if (wrapper_le32(t) != crc) return kWrapDataCheck;
    return wrapper_le32(t + 4) != (uint32_t)out_len ? kWrapLengthCheck : kWrapNone;
}

// the member's bytes through a plain pointer, one lane (or the host) walking them
struct LaneBytes {
    const uint8_t *src;
    ZR_HD uint32_t byte(uint64_t pos) const { return src[pos]; }
    ZR_HD uint64_t find_zero(uint64_t from, uint64_t n) const {
        while (from < n && src[from]) ++from;
        return from < n ? from : n;
    }
};
// the member's bytes in host memory
struct HostBytes {
    const uint8_t *src;
    uint32_t byte(uint64_t pos) const { return src[pos]; }
    uint64_t find_zero(uint64_t from, uint64_t n) const {
        const void *z = from < n ? memchr(src + from, 0, (size_t)(n - from)) : nullptr;
        return z ? (uint64_t)((const uint8_t *)z - src) : n;
    }
};

// CRC-32 of a gzip header on the host, without the device context (zng_rocm_wrapper_parse and the header writer of
// gzip_header_plan.h work before zng_rocm_init)
inline uint32_t wrapper_host_crc32(const uint8_t *p, size_t n) {
    static const struct Table {
        uint32_t t[256];
        Table() {
            for (uint32_t i = 0; i < 256; ++i) {
                uint32_t c = i;
                for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
                t[i] = c;
            }
        }
    } tab;
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) c = tab.t[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return ~c;
}

// What a caller that holds the whole member and no dictionary makes of its header. msg (InflateMsg): kMsgNone -- the deflate
// data begins at header_len; kMsgStarved -- the member ends inside its header; kMsgNeedDict -- a zlib header with FDICT
// (Z_NEED_DICT, a data error for the one-shot caller, uncompr.c:70-75); else the header's fault, with the rules' own id in
// wrap_msg (zng_rocm_uncompress2_dev tells unknown flag bits apart).  byte_tab: the 256 entries of the CRC-32 byte table
// (DeviceTables::byte_tab on the device, host_tables.byte_tab on the host).
struct WholeHead {
    uint64_t header_len;
    uint32_t msg, wrap_msg;
    uint32_t fdict, dictid;
};
template <class Bytes>
ZR_HD WholeHead wrapper_parse_whole(int format, const Bytes &in, uint64_t n, const uint32_t *byte_tab) {
    WholeHead r = {0, kMsgNone, kWrapNone, 0, 0};
    // the two answers that are NOT the rules': (1) a gzip member short of 10 bytes is starved whatever its bytes are -- the rules
    // judge the magic at 2 bytes, method and flags at 4; (2) a zlib header that passes with FDICT set needs a dictionary even
    // where the DICTID is cut short -- the rules say -5 there (their only -5 for zlib with n >= 2, so the FLG read below
    // decides nothing more: it is there to name the bit this answer is about)
    if (format == 2 && n < 10) { r.msg = kMsgStarved; return r; }                                           // (1)
    WrapperHead h = wrapper_parse_rules(format, in, n);
    if (format == 1 && h.status == -5 && n >= 2 && (in.byte(1) & 0x20u)) { h.status = 0; h.fdict = 1; }     // (2)
    if (h.status == 0 && h.hcrc) {                       // FHCRC: the low 16 bits of the CRC-32 of the header in front of it
        uint32_t c = 0xffffffffu;
        for (uint64_t k = 0; k + 2 < h.header_len; ++k) c = byte_tab[(c ^ in.byte(k)) & 0xffu] ^ (c >> 8);
        if ((~c & 0xffffu) != h.hcrc_stored) { h.status = -3; h.msg = kWrapHeaderCrc; }
    }
    r.header_len = h.header_len;
    r.wrap_msg = h.msg;
    r.fdict = h.fdict;
    r.dictid = h.dictid;
    if (h.status == -5) r.msg = kMsgStarved;
    else if (h.status == -3) r.msg = wrapper_inflate_msg(h.msg);
    else if (h.fdict) r.msg = kMsgNeedDict;
    return r;
}

// BGZF (the blocked gzip of bgzip / BAM / tabix, SAM specification 4.1): every member carries the FEXTRA subfield SI1 66 'B',
// SI2 67 'C', SLEN 2 whose 16 bits are BSIZE = the member's bytes - 1, header and trailer included.  The subfields of the
// FEXTRA field (RFC 1952 2.3.1.1: SI1 SI2 SLEN and SLEN bytes, one behind the other inside the XLEN bytes at 12) are walked
// in order, for host and device alike: the first 'BC' subfield with SLEN 2 is the answer, one with any other SLEN is a
// subfield like any other, and a subfield that XLEN cuts short ends the walk with no answer.  gz_look (gzread.c.in:81-154)
// does not look into the field at all -- inflate skips it, inflate.c:599-641 -- so BSIZE is a hint to the member finder
// (gzip_members.hip) and never decides what a member is.  `n`: bytes of the member that exist; false when they end
// inside the field or the header has none.
template <class Bytes>
ZR_HD bool gzip_bgzf_bsize(const Bytes &in, uint64_t n, uint32_t *bsize) {
    if (n < 12 || !(in.byte(3) & 4u)) return false;
    const uint64_t end = 12u + (in.byte(10) | (in.byte(11) << 8));
    if (end > n) return false;
    for (uint64_t p = 12; p + 4 <= end;) {
        const uint32_t si1 = in.byte(p), si2 = in.byte(p + 1), slen = in.byte(p + 2) | (in.byte(p + 3) << 8);
        if (p + 4 + slen > end) return false;
        if (si1 == 66u && si2 == 67u && slen == 2u) {
            *bsize = in.byte(p + 4) | (in.byte(p + 5) << 8);
            return true;
        }
        p += 4u + slen;
    }
    return false;
}

}  // namespace zr
