// dict_plan.h -- the rules of the shared preset dictionary of the many-stream calls (zng_rocm_dict_create_dev,
// zng_rocm_compress_streams_dict_dev, zng_rocm_uncompress_streams_dict_dev).  Plain C++ over integers and bytes, no HIP: which
// bytes of a dictionary serve as history, the primed head table of the level-1 class, the 16-byte zlib wrapper with FDICT and
// what a reader makes of a zlib header when it holds one dictionary.  The rules the kernels apply as well are written once
// for host and device; tests/test_dict_plan_cpu.py drives them through tests/c/dict_plan_driver.cpp without a GPU.
//
// The wrapper: CMF FLG | DICTID, most significant byte first | two empty stored blocks | the block | Adler-32 of the plaintext
//   78 3f  id id id id  00 00 00 ff ff  00 00 00 ff ff
// CMF / FLG are what deflate.c:868-888 writes for the fastest level with a dictionary set: level_flags 0, PRESET_DICT, and
// 0x7820 is a multiple of 31 already, so the check bits are the full 31.  The DICTID follows (deflate.c:889-892).  The two
// empty stored blocks are the padding of the 12-byte wrapper of framing_dev.hip: the block starts 4-byte aligned.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "framing_parse.h"
#include "gf2.h"      // ZR_HD
#include "inflate_dev_types.h"

namespace zr {

constexpr uint32_t kDictWindowMax = 32768u;       // the tail of a longer dictionary is its window (deflate.c:477-486)
constexpr uint32_t kDictHashBits = 12;            // the head table of the level-1 class (kQuickHashBits, deflate_stream.hip)
constexpr uint32_t kDictHeadSlots = 1u << kDictHashBits;
constexpr uint32_t kDictMinMatch = 4;             // bytes a position needs behind it to be entered (kLzMinMatch)
constexpr uint32_t kDictPad = 64u;                // zero bytes behind the window: the matcher probes 32 bytes from any position
constexpr uint32_t kDictWrapHead = 16u;
constexpr uint32_t kDictHeadParsed = 6u;          // CMF FLG DICTID: what a reader has consumed when it judges the DICTID
constexpr uint32_t kDictMismatch = 0x80000000u;   // header verdict "another dictionary": -3 with no message (inflate.c:1247-1249)

// bytes of a dictionary of dict_len bytes that serve as history, and where they begin
ZR_HD uint32_t dict_window(uint64_t dict_len) { return dict_len < kDictWindowMax ? (uint32_t)dict_len : kDictWindowMax; }
ZR_HD uint64_t dict_window_start(uint64_t dict_len) { return dict_len - dict_window(dict_len); }

// the bucket of the four bytes `first4` (least significant first): lz_hash<kDictHashBits> of deflate_lz.h
ZR_HD uint32_t dict_hash(uint32_t first4) { return (first4 * 2654435761u) >> (32u - kDictHashBits); }
ZR_HD uint32_t dict_first4(const uint8_t *w) {
    return (uint32_t)w[0] | ((uint32_t)w[1] << 8) | ((uint32_t)w[2] << 16) | ((uint32_t)w[3] << 24);
}
// positions of a window of W bytes that are entered: p + 4 <= W (the last 3 are left out, deflate.c:494-501)
ZR_HD uint32_t dict_positions(uint32_t W) { return W >= kDictMinMatch ? W - kDictMinMatch + 1u : 0u; }

// The primed head table: head[h] = 1 + the largest entered p whose four bytes fall into bucket h, else 0 -- what entering
// the positions in order leaves.  (The device builds it with one atomic max per position.)
inline void dict_head_table(const uint8_t *window, uint32_t W, uint32_t *head) {
    for (uint32_t h = 0; h < kDictHeadSlots; ++h) head[h] = 0;
    for (uint32_t p = 0; p < dict_positions(W); ++p) head[dict_hash(dict_first4(window + p))] = p + 1u;
}

// ---- the rows engine (levels 1..9 of zng_rocm_compress_streams2_dict_dev, deflate_dyn.hip) ------------------------------------
// Its search state -- the three LDS arrays pos / tag / cnt of RowShared (deflate_rows.h) -- as lz_rows_kernel's priming loop
// leaves it behind the positions [0, T) of the window, built once per dictionary and stored in this order in the object.
constexpr uint32_t kDictRowBatch = 1024u;         // kRowBatch: positions the engine enters per batch
constexpr uint32_t kDictRowsPosBytes = 3584u * 8u * 2u, kDictRowsTagBytes = 3584u * 8u, kDictRowsCntBytes = 3584u;
constexpr uint32_t kDictRowsBytes = kDictRowsPosBytes + kDictRowsTagBytes + kDictRowsCntBytes;      // 89 600
// T: the primed positions are the whole batches whose every 4-byte string lies inside the window -- the largest multiple of
// the batch with T + 3 <= W.  The positions from T on are entered per stream, with the plaintext their strings reach into.
ZR_HD uint32_t dict_rows_primed(uint32_t W) { return W < 3u ? 0u : (W - 3u) / kDictRowBatch * kDictRowBatch; }

// byte k (0 .. 15) of the wrapper's head
ZR_HD uint8_t dict_header_byte(uint32_t k, uint32_t dictid) {
    if (k < 2u) return k ? (uint8_t)0x3f : (uint8_t)0x78;
    if (k < 6u) return (uint8_t)(dictid >> (8u * (5u - k)));
    const uint32_t m = (k - 6u) % 5u;                 // 00 00 00 ff ff, twice
    return m < 3u ? (uint8_t)0x00 : (uint8_t)0xff;
}
ZR_HD void dict_put_header(uint8_t *out, uint32_t dictid) {
    for (uint32_t k = 0; k < kDictWrapHead; ++k) out[k] = dict_header_byte(k, dictid);
}
// the trailer: Adler-32 of the plaintext, most significant byte first (deflate.c:1098-1101)
ZR_HD uint8_t dict_trailer_byte(uint32_t k, uint32_t adler) { return wrapper_trailer_byte(1, k, adler, 0u); }

// What the reader makes of the first bytes of a zlib member (inflate.c:509-555 with windowBits 15, :702-715 DICTID) when it
// holds the dictionary whose id is `dictid` -- wrapper_parse_rules (framing_parse.h) with the dictionary's judgement on top:
//   msg      kMsgNone: decode from byte `pos` on; kDictMismatch: FDICT names another dictionary (pos = 6); else the header's
//            fault as zng_rocm_uncompress_streams_dev reports it -- a header that ends inside the DICTID is a short header
//   history  1: FDICT set and the ids agree, the payload is decoded with the dictionary; 0: FDICT clear, no history
struct DictHeader {
    uint32_t pos, msg, history;
};
ZR_HD DictHeader dict_parse_header(const uint8_t *in, uint64_t n, uint32_t dictid) {
    const WrapperHead h = wrapper_parse_rules(1, LaneBytes{in}, n);         // the order of the checks lives there
    DictHeader r = {n < 2u ? 0u : 2u, kMsgNone, 0u};
    if (h.status == -5) r.msg = kMsgStarved;                                // inside CMF / FLG or inside the DICTID
    else if (h.status == -3) r.msg = wrapper_inflate_msg(h.msg);
    else if (h.fdict) {
        r.pos = kDictHeadParsed;
        if (h.dictid == dictid) r.history = 1u;
        else r.msg = kDictMismatch;
    }
    return r;
}

}  // namespace zr
