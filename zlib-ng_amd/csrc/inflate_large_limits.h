// inflate_large_limits.h -- the argument ranges of the large device inflaters (inflate_large.hip), shared with the wrapped
// calls in front of them (framing_large.hip), which refuse what the raw calls refuse before anything is launched.
#pragma once
#include <stddef.h>

namespace zr {

constexpr size_t kPieceMin = 4u << 20;                  // the least piece (the hook's device threshold, hook.hip)
constexpr size_t kPieceDefault = 64u << 20;
constexpr size_t kPieceMax = 1u << 30;                  // the largest (a pass's buffer stays below inflate_large_try's 2 GiB)
constexpr size_t kRoundMin = 4u << 20;                  // zng_rocm_inflate_large_streams_dev: round_bytes in [kRoundMin, kRoundEnd)
constexpr size_t kRoundEnd = (size_t)1 << 31;
constexpr size_t kRoundDefault = 256u << 20;

}  // namespace zr
