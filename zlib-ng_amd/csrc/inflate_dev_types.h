// inflate_dev_types.h -- the part of inflate_dev.h that needs no HIP: the device job descriptor, the message ids of d_results,
// the block-start finder's tables and the sync kernel's work item.  inflate_large_plan.h (plain host code, compiled by a CPU
// test as well) is built on these.
#pragma once
#include <stdint.h>

namespace zr {

struct InflateJobDev {
    const uint8_t *in;
    uint8_t       *out;
    uint64_t       in_len;
    uint64_t       out_cap;
    uint32_t       dict_len;
    uint32_t       flags;
};

// the span form's table, parallel to the jobs (inflate_streams_span_kernel): where the job's own window ends, and the bit of
// its first byte the decode starts at
struct InflateSpanDev {
    const uint8_t *hist_end;
    uint32_t       start_bit;      // 0..7
    uint32_t       pad;
};

enum InflateMsg : uint32_t {
    kMsgNone = 0, kMsgBlockType, kMsgStoredLen, kMsgTooMany, kMsgCodeLengthsSet, kMsgBitRepeat, kMsgNoEob,
    kMsgLitLenSet, kMsgDistSet, kMsgLitLenCode, kMsgDistCode, kMsgTooFar, kMsgStarved, kMsgOutFull,
    // wrappers (framing_dev.hip; inflate.c:509-555 header checks, :686-692 FHCRC, :1105-1147 trailer checks)
    kMsgHeaderCheck, kMsgMethod, kMsgWindow, kMsgHeaderCrc, kMsgNeedDict, kMsgDataCheck, kMsgLengthCheck, kMsgCount
};

// The block-start finder's tables (inflate_large.hip: find_headers_table_kernel, validate_headers_table_kernel,
// first_bytes_kernel): the streams of one finder pass, and the work items -- a range of one stream each -- its scan is cut
// into.  The survivors of all streams go to ONE list, each tagged with its stream's index in the table.
struct FindStreamDev {
    const uint8_t     *src;
    unsigned long long src_len;
};
struct FindItemDev {
    unsigned long long lo, hi;    // bytes of the stream
    uint32_t           stream, pad;
};
constexpr unsigned kFindTagShift = 40;                   // a bit position takes 34 bits, the marks bits 62 and 63
constexpr unsigned long long kFindTagMask = 0x3fffffull << kFindTagShift;

// a region of the stream that starts at a block start the finder gave (one work item: at most 64 guesses, so a long region
// is several items): `n` guesses at start + (k0 + k) * spacing, k = 1 .. n, written to out_bit / out_key [first + 2 (k - 1)] (a symbol boundary B and its key, or ~0 = none) and, when the region's
// block does not have fixed codes and `fixed_too` is set, [first + 2 (k - 1) + 1] with fixed codes (a noise start inside a
// fixed-code block reads as a dynamic header or a stored block's pattern); `dynamic` = 0: no guesses with a dynamic block's
// tables
struct SubRegionDev {
    unsigned long long start, spacing;
    uint32_t           first, n, dynamic, fixed_too, k0;
    uint32_t           pad = 0;
    const uint8_t     *src = nullptr;      // a batch of streams in one launch: the region's own stream (null: the launch's)
    unsigned long long src_len = 0;
};

}  // namespace zr
