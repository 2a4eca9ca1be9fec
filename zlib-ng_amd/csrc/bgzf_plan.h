// bgzf_plan.h -- the host steps of zng_rocm_bgzf_compress_dev (bgzf.hip): device-resident plaintext written as a BGZF file
// (SAM specification 4.1; htslib bgzf.c), one member per piece of at most 65280 bytes.  Plain C++ over integers, no HIP: the
// cut into pieces and rounds, the bound, the argument checks, what a member weighs and when its payload is a stored block
// instead of the engine's, and the bytes of header, trailer and end-of-file block.  The rules the kernels apply as well
// (bgzf_member, the header and trailer bytes) are written once for host and device; tests/test_bgzf_plan_cpu.py drives them
// through tests/c/bgzf_plan_driver.cpp without a GPU.
//
// A member is  18 bytes of header | raw deflate payload | CRC-32 | ISIZE  and must not pass 65536 bytes, because its size
// minus one (BSIZE) is a 16-bit field of the header.  The header is the one htslib writes at every level:
//   1f 8b 08 04  00 00 00 00  00 ff  06 00  42 43 02 00  <BSIZE lo> <BSIZE hi>
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gf2.h"      // ZR_HD

namespace zr {

constexpr uint32_t kBgzfBlock = 65280u;               // htslib's BGZF_BLOCK_SIZE: the most plaintext one member takes
constexpr uint32_t kBgzfHead = 18u, kBgzfTail = 8u;
constexpr uint32_t kBgzfMaxMember = 65536u;           // BSIZE + 1 at its largest
constexpr uint32_t kBgzfMaxPayload = kBgzfMaxMember - kBgzfHead - kBgzfTail;     // 65510
constexpr uint32_t kBgzfStoredHead = 5u;              // 01 LEN NLEN (RFC 1951 3.2.4)
constexpr uint32_t kBgzfEofBytes = 28u;
constexpr uint32_t kBgzfNoEof = 1u, kBgzfQuick = 2u;  // ZNG_ROCM_BGZF_NO_EOF, ZNG_ROCM_BGZF_QUICK
constexpr uint64_t kBgzfRoundDefault = (1ull << 30) + kBgzfBlock;      // plaintext per round when the caller says 0: 1 GiB and
                                                                       // the piece that straddles its end, so 1 GiB is one round
constexpr uint32_t kBgzfForceStored = 0xffffffffu;    // the `clen` of a member no engine was asked about (level 0)

// the end-of-file block: an empty member whose payload is the empty final static block 03 00
constexpr uint8_t kBgzfEof[kBgzfEofBytes] = {0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43,
                                             0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00};

// ---- the member ---------------------------------------------------------------------------------------------------------
struct BgzfMember {
    uint32_t payload;     // bytes between header and trailer
    uint32_t stored;      // 1: the payload is one final stored block around the piece, copied from the plaintext
};

// A piece of n bytes (1 .. 65280) whose engine output is clen bytes.  The engine's bytes are kept unless they are more than
// the stored form of the piece (n + 5) or would take the member past 65536 bytes; so a member is at most n + 31 bytes and at
// most 65536 (n + 5 <= 65285 < 65510).
ZR_HD BgzfMember bgzf_member(uint32_t n, uint32_t clen) {
    BgzfMember m;
    m.stored = (clen > n + kBgzfStoredHead || clen > kBgzfMaxPayload) ? 1u : 0u;
    m.payload = m.stored ? n + kBgzfStoredHead : clen;
    return m;
}
ZR_HD uint32_t bgzf_member_bytes(const BgzfMember &m) { return kBgzfHead + m.payload + kBgzfTail; }

// byte k (0 .. 17) of the header of a member of member_bytes bytes
ZR_HD uint8_t bgzf_header_byte(uint32_t k, uint32_t member_bytes) {
    const uint32_t bsize = member_bytes - 1u;
    // the sixteen constant bytes, least significant first
    const uint64_t lo = 0x00000000'04088b1full, hi = 0x00024342'0006ff00ull;
    return k < 8u ? (uint8_t)(lo >> (8u * k)) : k < 16u ? (uint8_t)(hi >> (8u * (k - 8u))) : (uint8_t)(bsize >> (8u * (k - 16u)));
}
// byte k (0 .. 7) of the trailer: CRC-32 of the piece and its length, both least significant byte first
ZR_HD uint8_t bgzf_trailer_byte(uint32_t k, uint32_t crc, uint32_t n) {
    return (uint8_t)((k < 4u ? crc : n) >> (8u * (k & 3u)));
}
// byte k (0 .. 4) of the header of the final stored block around n bytes
ZR_HD uint8_t bgzf_stored_byte(uint32_t k, uint32_t n) {
    const uint32_t len = n & 0xffffu, nlen = ~n & 0xffffu;
    return k == 0u ? (uint8_t)1u : k < 3u ? (uint8_t)(len >> (8u * (k - 1u))) : (uint8_t)(nlen >> (8u * (k - 3u)));
}
// byte k (0 .. 27) of the end-of-file block (kBgzfEof, for code that cannot index a host table)
ZR_HD uint8_t bgzf_eof_byte(uint32_t k) {
    return k < kBgzfHead ? bgzf_header_byte(k, kBgzfEofBytes) : k == kBgzfHead ? (uint8_t)0x03u : (uint8_t)0u;
}
ZR_HD void bgzf_put_header(uint8_t *out, uint32_t member_bytes) {
    for (uint32_t k = 0; k < kBgzfHead; ++k) out[k] = bgzf_header_byte(k, member_bytes);
}
ZR_HD void bgzf_put_trailer(uint8_t *out, uint32_t crc, uint32_t n) {
    for (uint32_t k = 0; k < kBgzfTail; ++k) out[k] = bgzf_trailer_byte(k, crc, n);
}

// ---- the cut ------------------------------------------------------------------------------------------------------------
// block_bytes as the caller gives it -> the piece size, or 0 for a value the call refuses
ZR_HD uint32_t bgzf_piece_bytes(uint32_t block_bytes) {
    return block_bytes == 0u ? kBgzfBlock : block_bytes <= kBgzfBlock ? block_bytes : 0u;
}
ZR_HD uint64_t bgzf_pieces(uint64_t src_len, uint32_t piece) { return (src_len + piece - 1u) / piece; }
// bytes of piece g (0 .. pieces - 1)
ZR_HD uint32_t bgzf_piece_len(uint64_t src_len, uint32_t piece, uint64_t g) {
    const uint64_t left = src_len - g * piece;
    return left < piece ? (uint32_t)left : piece;
}

// round_bytes as the caller gives it -> pieces per round: rounded down to whole pieces, at least one
inline uint64_t bgzf_round_pieces(uint64_t round_bytes, uint32_t piece) {
    const uint64_t bytes = round_bytes ? round_bytes : kBgzfRoundDefault;
    const uint64_t per = bytes / piece;
    return per ? per : 1u;
}
inline uint64_t bgzf_rounds(uint64_t src_len, uint32_t piece, uint64_t round_bytes) {
    const uint64_t per = bgzf_round_pieces(round_bytes, piece), np = bgzf_pieces(src_len, piece);
    return (np + per - 1u) / per;
}

// src_len + 31 per member + the end-of-file block; 0 for a block_bytes the call refuses
inline uint64_t bgzf_bound(uint64_t src_len, uint32_t block_bytes) {
    const uint32_t piece = bgzf_piece_bytes(block_bytes);
    if (!piece) return 0;
    return src_len + (uint64_t)(kBgzfHead + kBgzfStoredHead + kBgzfTail) * bgzf_pieces(src_len, piece) + kBgzfEofBytes;
}

// ---- the arguments ------------------------------------------------------------------------------------------------------
// level as the caller gives it (-1 = 6) -> 0 .. 9, or -1 for a refused one
inline int bgzf_level(int level) { return level == -1 ? 6 : (level >= 0 && level <= 9 ? level : -1); }

// what the call refuses before it launches or writes anything; the pointers are looked at only for being null
inline bool bgzf_args_ok(int level, const void *d_src, uint64_t src_len, uint32_t block_bytes, const void *d_dst, uint64_t dst_cap,
                         const void *out_len, const void *members, uint64_t members_cap, const void *nmembers, uint32_t flags) {
    if (!out_len || !nmembers) return false;
    if (flags & ~(kBgzfNoEof | kBgzfQuick)) return false;
    if (bgzf_level(level) < 0) return false;
    if ((flags & kBgzfQuick) && level != 1) return false;
    if (!bgzf_piece_bytes(block_bytes)) return false;
    if ((!d_src && src_len) || (!d_dst && dst_cap) || (!members && members_cap)) return false;
    return true;
}

}  // namespace zr
