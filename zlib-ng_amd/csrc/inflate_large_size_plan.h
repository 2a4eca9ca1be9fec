// inflate_large_size_plan.h -- the rules of zng_rocm_uncompress_large_size_dev / _sizes_dev: the plaintext length of LARGE
// device-resident streams from a counting part pass (inflate_large.hip: pass_run's counting mode; the kernels are
// inflate_large_size.hip's).  Plain C++ over integers and the result tables, no HIP, as inflate_large_plan.h: the argument
// checks, the result words of the counting kernels, the chain walk over counting parts with its 64-bit total, and the row of a
// wrapped member.  tests/test_large_size_plan_cpu.py drives them through tests/c/large_size_plan_driver.cpp without a GPU.
//
// The finder, thin_starts and the part tables are inflate_large_plan.h's and unchanged.  The walk is walk_chain's stream
// mode (no sub-starts, no blocks mode, no pieces) with one difference, the reason it is written out here: a part's count is 64
// bits -- one part can expand to more than 4 GiB (4 MiB of a run) -- so nothing of it goes through PartCopy's 32-bit n.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zng_rocm.h"
#include "framing_parse.h"          // wrapper_tail_bytes
#include "inflate_dev_types.h"
#include "inflate_large_limits.h"
#include "inflate_large_plan.h"     // large_length_ok, kPieceMaxParts

namespace zr {

// ---- the checks ---------------------------------------------------------------------------------------------------------
// (flags: none -- no SUBBLOCK form, no unknown bits)
inline bool ls_round_ok(size_t round_bytes) { return !round_bytes || (round_bytes >= kRoundMin && round_bytes < kRoundEnd); }
// one stream as both calls take it: the destination is not looked at.  format 0: of the history only its LENGTH matters, a
// null pointer with a length is accepted; format 1: the dictionary's bytes are needed for the DICTID; format 2 takes none
inline bool ls_job_ok(int format, const void *d_src, uint64_t src_len, const void *d_window, uint32_t window_len) {
    if (!d_src && src_len) return false;
    if (src_len >= (1ull << 31)) return false;            // bit positions must fit the tables' words (a pieces loop: later)
    if (window_len > 32768u) return false;
    if (format == 1 && window_len && !d_window) return false;
    if (format == 2 && (d_window || window_len)) return false;
    return true;
}

// ---- result words of the counting kernels ---------------------------------------------------------------------------------
// A PART (inflate_size_parts_kernel), 8 words, those of inflate_streams_kernel<PART> (inflate_large_plan.h) with two
// differences: r[0] is the LOW word of the bytes the part would produce and r[7] -- the decoder's copy of BFINAL, which no
// walk reads -- the HIGH word.  r[1..2] the bit it ended on, r[3] = 1 when that was the end of the BFINAL block, r[4] message,
// r[5] the farthest a distance reached in front of the part, r[6] the part that starts where it ended, or ~0.
inline uint64_t ls_part_count(const uint32_t *r) { return (uint64_t)r[0] | ((uint64_t)r[7] << 32); }
// A whole STREAM by one wavefront (inflate_size_stream_kernel), 8 words: the row of zng_rocm_inflate_sizes_dev with a count
// that does not saturate -- w[0..1] plaintext bytes, w[2] input bytes consumed, w[3] status, w[4] message id
struct LsRow {
    uint64_t out_len;
    uint32_t used, status, msg;
};
inline LsRow ls_stream_row(const uint32_t *w) { return LsRow{(uint64_t)w[0] | ((uint64_t)w[1] << 32), w[2], w[3], w[4]}; }

// ---- the chain over counting parts ------------------------------------------------------------------------------------------
struct SizeChain {
    uint64_t produced = 0;
    unsigned long long end_bit = 0;
    size_t parts = 0;                                     // genuine parts: what the decode's chain would hold
    const char *reason = nullptr;                         // a failed walk: why
    size_t bad_part = ~(size_t)0;                         // ... and when it was a part's own result, which part of the stream
};
// One stream's walk from its first part: res is the launch's table, the stream's parts are [pbase, pbase + np) of it, starts
// are the stream's own.  true: the chain reached the end of the BFINAL block, c.produced bytes from c.end_bit bits.
// false = irregular (c.reason): the one-wavefront kernel sizes the stream and gives the decoder's verdict.
// A reach of exactly produced + window_len is the oldest byte there is; one more is in front of the stream.
inline bool walk_size_chain(const uint32_t *res, size_t pbase, size_t np, const unsigned long long *starts, uint32_t window_len,
                            SizeChain &c) {
    auto fail = [&](const char *reason) {
        c.reason = reason;
        return false;
    };
    c.end_bit = starts[0];
    for (size_t cur = 0;;) {
        const size_t g = pbase + cur;
        const uint32_t *r = &res[8 * g];
        const bool ended = r[3] == 1u;
        if (r[4] != kMsgNone || !(ended || r[6] != 0xffffffffu)) {                // error / truncation on the chain
            c.bad_part = cur;
            return fail("a part's message, or no end");
        }
        if ((uint64_t)r[5] > c.produced + window_len) return fail("a distance reaches in front of the stream");
        const uint64_t n = ls_part_count(r);
        if (n > ~c.produced) return fail("the parts' counts pass 64 bits");
        c.produced += n;
        ++c.parts;
        c.end_bit = (unsigned long long)r[1] | ((unsigned long long)r[2] << 32);
        if (ended) return true;
        // a part ends on a LATER start of its own stream (so a bad word cannot send the walk round in a circle)
        if (r[6] <= g || r[6] >= pbase + np) return fail("bad chain link");
        cur = r[6] - pbase;
    }
}

// ---- the row of a member ------------------------------------------------------------------------------------------------------
// is_sizing_row's last rule (inflate_sizes_plan.h) with a 64-bit count: a payload that ended (status 1) `at` bytes into a
// member of src_len bytes needs its 4 / 8 trailer bytes present; they are counted, and NOT compared -- there is no plaintext
// to check.  Sets status / in_used; the count stands either way.
inline void ls_member_tail(int format, uint64_t at, uint64_t src_len, int *status, uint64_t *in_used) {
    const uint32_t tail = wrapper_tail_bytes(format);
    if (at + tail > src_len) {
        *status = -5;
        *in_used = src_len;
    } else {
        *status = 1;
        *in_used = at + tail;
    }
}

}  // namespace zr
