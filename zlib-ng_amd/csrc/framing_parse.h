// framing_parse.h -- the rules of the zlib (RFC 1950) and gzip (RFC 1952) wrappers, ONCE, for host and device: what
// inflate() does in its HEAD .. HCRC and DICTID states (inflate.c:509-555 zlib, :556-700 gzip, :702-715 dictionary id) on a
// member that is all in memory.  The function is a template over the way the bytes are reached, so that
// zng_rocm_wrapper_parse walks host memory with memchr while the header kernel of framing_large.hip searches the
// terminators of FNAME / FCOMMENT with a whole wavefront; the ORDER of the checks and their answers are written here only.
// The FHCRC is not evaluated here: the function says where the stored 16 bits were and over how many bytes they are taken,
// and the caller compares (the host with a table walk, the device with the many-message checksum pass).
#pragma once
#include <stdint.h>

#include "gf2.h"

namespace zr {

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
