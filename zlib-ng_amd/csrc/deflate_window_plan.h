// deflate_window_plan.h -- the rules of deflateInit2's windowBits on the compress side (the zng_rocm_*_window_* calls of
// deflate_dyn.hip, compress_streams.hip and hook.hip): which values are taken, the distance cap and the priming length they mean
// for the rows matcher, and the zlib header they write.  Plain C++ over integers, no HIP; tests/test_window_plan_cpu.py drives
// them through tests/c/window_plan_driver.cpp without a GPU.
//
//   windowBits   9..15 (deflate.c:317-318: MIN_WBITS 8 .. MAX_WBITS 15).  8 is taken by the zlib wrapper alone and then means 9
//                (deflate.c:319: `windowBits == 8 && wrap != 1` is Z_STREAM_ERROR; :322-323: "until 256-byte window bug fixed"),
//                so the raw calls, which have no format, and formats 0 and 2 refuse it.
//   cap          MAX_DIST(s) = w_size - MIN_LOOKAHEAD = (1 << w) - 262 (deflate.h:405-415): no match reaches further back.  A
//                reader whose window is 1 << w refuses a greater distance, so this is validity, not ratio.
//   priming      a segment enters the min(32768, 1 << w) bytes in front of itself into the rows, from a batch border: nothing
//                further back can be referenced, and every source within the cap of the segment's first byte is entered.
//   zlib header  CMF = 8 + ((w - 8) << 4), FLEVEL and FCHECK as ever (deflate.c:870-885): wrapper_header_byte of framing_parse.h
//                with its window argument -- no rule is restated here.  gzip has no window field: only the distances change.
// At 15 every rule gives what the calls without a window have always done.
#pragma once
#include <stdint.h>

#include "../../include/zng_rocm.h"
#include "framing_parse.h"
#include "gf2.h"      // ZR_HD

namespace zr {

constexpr int      kWinBitsMin = 9, kWinBitsMax = 15;
constexpr uint32_t kWinMinLookahead = 258u + 3u + 1u;        // MIN_LOOKAHEAD, deflate.h:405
constexpr uint32_t kWinPrimeMax = 32768u;                    // what a segment has always entered in front of itself
constexpr uint32_t kWinBatch = 1024u;                        // the rows matcher's batch: priming begins at a batch border

// windowBits as the caller gives it -> the window the stream is written with (9..15), or 0 = refused.  format: 0 raw, 1 zlib,
// 2 gzip; the raw calls (zng_rocm_deflate_window_block_dev, _streams_dev, the hook) pass 0
ZR_HD int win_effective(int format, int window_bits) {
    if (window_bits == 8) return format == 1 ? 9 : 0;                                    // deflate.c:319, :322-323
    return window_bits >= kWinBitsMin && window_bits <= kWinBitsMax ? window_bits : 0;   // deflate.c:317-318
}
// the verdict of a call: 0 or ZNG_ROCM_EINVAL
ZR_HD int win_check(int format, int window_bits) { return win_effective(format, window_bits) ? ZNG_ROCM_OK : ZNG_ROCM_EINVAL; }

// w is an effective window, 9..15
ZR_HD uint32_t win_size(int w) { return 1u << w; }                                       // w_size, deflate.c:345
ZR_HD uint32_t win_dist(int w) { return win_size(w) - kWinMinLookahead; }                // MAX_DIST(s), deflate.h:410-415
ZR_HD uint32_t win_prime(int w) { return win_size(w) < kWinPrimeMax ? win_size(w) : kWinPrimeMax; }
// the first position a segment that begins at seg_start enters into the rows (positions count from the first history byte)
ZR_HD uint32_t win_prime_start(uint32_t seg_start, int w) {
    const uint32_t p0 = seg_start > win_prime(w) ? seg_start - win_prime(w) : 0u;
    return p0 - p0 % kWinBatch;
}
// does the matcher run its window form?  15 stays on the kernel it has always had
ZR_HD bool win_form(int w) { return w != kWinBitsMax; }

// byte k of the member's header (wrapper_head_bytes(format) of them) at effective window w
ZR_HD uint8_t win_header_byte(int format, int level, int strategy, int w, uint32_t k) {
    return wrapper_header_byte(format, level, strategy, k, w);
}

}  // namespace zr
