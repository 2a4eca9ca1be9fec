// inflate_sizes_plan.h -- the rules of zng_rocm_inflate_sizes_dev and zng_rocm_uncompress_packed_dev (inflate_sizes.hip): the
// plaintext length of many device-resident streams found by a parse that stores nothing, and the same streams decoded back to
// back into one destination at offsets the device works out -- the read side of zng_rocm_compress_members_dev.  Plain C++
// over integers, no HIP: the argument checks of both calls, the saturation of a stream's count, the sizing row of a wrapped
// member, the places (alignment, which jobs get room, the fit against dst_cap, 64-bit offsets) and the final row of the packed
// call.  The rules the kernels apply as well are written once for host and device;
// tests/test_inflate_sizes_plan_cpu.py drives them through tests/c/inflate_sizes_plan_driver.cpp without a GPU.
//
// A row is the four words every stream call writes: {plaintext bytes, input bytes consumed, status, message id}.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zng_rocm.h"
#include "dict_plan.h"          // kDictMismatch
#include "framing_parse.h"      // wrapper_tail_bytes
#include "gf2.h"                // ZR_HD
#include "inflate_dev_types.h"  // message ids

namespace zr {

constexpr uint32_t kIsCountMax = 0x7fffffffu;         // the largest legal out_cap of the one-wavefront engine
constexpr uint64_t kIsInMax = 0x7fffffffull;          // in_len stays below 2 GiB
constexpr uint32_t kIsDictMax = 32768u;
constexpr uint32_t kIsAlignMax = 4096u;
constexpr uint32_t kIsBufError = (uint32_t)-5, kIsDataError = (uint32_t)-3;

struct IsRow {
    uint32_t out_len, used, status, msg;
};

// ---- the checks ---------------------------------------------------------------------------------------------------------
ZR_HD bool is_format_ok(int format) { return format >= 0 && format <= 2; }
// 0 and 1: back to back; else a power of two up to 4096
ZR_HD bool is_align_ok(uint32_t align) { return align <= kIsAlignMax && (align & (align - 1u)) == 0u; }
// the call itself, before any job is looked at; the pointers are looked at only for being null.  njobs == 0 is a call that
// does nothing, whatever `jobs` is
inline int is_call_check(int format, bool has_dict, const void *jobs, uint64_t njobs, const void *results) {
    if (!is_format_ok(format) || (format == 2 && has_dict)) return ZNG_ROCM_EINVAL;
    if (njobs > 0x7fffffffull) return ZNG_ROCM_EINVAL;
    if (njobs && (!jobs || !results)) return ZNG_ROCM_EINVAL;
    return ZNG_ROCM_OK;
}
// what the packed call asks on top: its tables are required even for an empty batch (d_offsets[0] is written then too)
inline int is_packed_call_check(int format, bool has_dict, const void *jobs, uint64_t njobs, const void *dst, uint64_t dst_cap,
                                uint32_t align, const void *offsets, const void *results) {
    if (!offsets || !results || !is_align_ok(align) || (!dst && dst_cap)) return ZNG_ROCM_EINVAL;
    return is_call_check(format, has_dict, jobs, njobs, results);
}
// one job; out and out_cap are not looked at.  A history length of the job's own belongs to a raw stream without a
// dictionary object in the sizing call alone: a packed buffer has no place for per-job history
inline int is_job_check(int format, bool has_dict, const zng_rocm_inflate_dev_job &j, bool packed) {
    if (j.in_len && !j.in) return ZNG_ROCM_EINVAL;
    if (j.in_len > kIsInMax) return ZNG_ROCM_EINVAL;
    if (j.flags) return ZNG_ROCM_EINVAL;
    if (j.dict_len > kIsDictMax) return ZNG_ROCM_EINVAL;
    if (j.dict_len && (has_dict || format != 0 || packed)) return ZNG_ROCM_EINVAL;
    return ZNG_ROCM_OK;
}
// the whole job list: the first refusal in job order, its job in *bad
inline int is_jobs_check(int format, bool has_dict, const zng_rocm_inflate_dev_job *jobs, uint64_t njobs, bool packed,
                         uint64_t *bad) {
    for (uint64_t i = 0; i < njobs; ++i)
        if (int rc = is_job_check(format, has_dict, jobs[i], packed)) {
            if (bad) *bad = i;
            return rc;
        }
    return ZNG_ROCM_OK;
}

// ---- the count of a stream ----------------------------------------------------------------------------------------------
// `n` more bytes (a literal, a match, a stored block) on a count: true when they no longer fit the largest legal out_cap --
// the count then stands at kIsCountMax and the parse stops with "output buffer too small", the decode's own end there
ZR_HD bool is_count_add(uint32_t *count, uint32_t n) {
    if (n > kIsCountMax - *count) {
        *count = kIsCountMax;
        return true;
    }
    *count += n;
    return false;
}
// the same on a 64-bit count (the sizing of large streams, inflate_large_size.hip): it never saturates
ZR_HD bool is_count_add(unsigned long long *count, uint32_t n) {
    *count += n;
    return false;
}
ZR_HD uint32_t is_status_of(uint32_t msg) {
    return msg == kMsgNone ? 1u : (msg == kMsgStarved || msg == kMsgOutFull) ? kIsBufError : kIsDataError;
}

// ---- the sizing row of a member -----------------------------------------------------------------------------------------
// `raw`: the row of the payload alone, parsed from byte `hdr` of the member on; `hdr`, `hmsg`: the header's length and
// verdict (wrapper_parse_whole, dict_parse_header; format 0: 0 and kMsgNone); `in_len`: the whole member.  The rules are the
// decode's (verify_trailer_kernel) without the comparison of the check value and ISIZE: a refused header, another
// dictionary's DICTID, the trailer's bytes present and counted.
ZR_HD IsRow is_sizing_row(int format, uint32_t hdr, uint32_t hmsg, uint64_t in_len, IsRow raw) {
    if (hmsg == kDictMismatch) return IsRow{0u, hdr, kIsDataError, kMsgNone};
    if (hmsg != kMsgNone) return IsRow{0u, 0u, hmsg == kMsgStarved ? kIsBufError : kIsDataError, hmsg};
    if ((int32_t)raw.status != 1) return IsRow{raw.out_len, raw.used + hdr, raw.status, raw.msg};
    const uint32_t tail = wrapper_tail_bytes(format);
    const uint64_t at = (uint64_t)hdr + raw.used;
    if (at + tail > in_len) return IsRow{raw.out_len, (uint32_t)in_len, kIsBufError, kMsgStarved};
    return IsRow{raw.out_len, (uint32_t)(at + tail), 1u, kMsgNone};
}

// ---- the places ---------------------------------------------------------------------------------------------------------
ZR_HD uint64_t is_align_up(uint64_t x, uint32_t align) {
    return align > 1u ? (x + align - 1u) & ~(uint64_t)(align - 1u) : x;
}
// bytes a job gets: its size when its sizing row has status 1, else none
ZR_HD uint64_t is_room(IsRow sizing) { return (int32_t)sizing.status == 1 ? sizing.out_len : 0u; }
// Job i starts at the running offset (the end of the bytes in front of it) rounded up to `align`.  Every start is a multiple
// of align, so the running rule is a prefix sum: off[i] = sum of is_padded(room[j]) over j < i -- what the scan adds up.
ZR_HD uint64_t is_padded(uint64_t room, uint32_t align) { return is_align_up(room, align); }
// the end of the batch's bytes (d_offsets[njobs]) from the last job's start and room; an empty batch needs nothing
ZR_HD uint64_t is_need(uint64_t last_off, uint64_t last_room) { return last_off + last_room; }
// a job with a place is decoded when it ends at or before dst_cap; starts never decrease, so behind a job that does not
// fit no job with a byte of its own fits either
ZR_HD bool is_fits(uint64_t off, uint64_t room, uint64_t dst_cap) { return off <= dst_cap && room <= dst_cap - off; }
// the running rule itself over a whole batch (host: the reference the driver holds the prefix-sum form against)
inline void is_places(const IsRow *sizing, uint64_t njobs, uint32_t align, uint64_t *offsets) {
    uint64_t running = 0;
    for (uint64_t i = 0; i < njobs; ++i) {
        offsets[i] = is_align_up(running, align);
        running = offsets[i] + is_room(sizing[i]);
    }
    offsets[njobs] = running;
}

// ---- the final row of the packed call -----------------------------------------------------------------------------------
// `decoded` is looked at only for a job that was decoded: its verified row (check value and ISIZE compared), out_len the
// decoded count
ZR_HD IsRow is_final_row(IsRow sizing, bool fits, IsRow decoded) {
    if ((int32_t)sizing.status != 1) return IsRow{0u, sizing.used, sizing.status, sizing.msg};
    if (!fits) return IsRow{0u, 0u, kIsBufError, kMsgOutFull};
    return decoded;
}

}  // namespace zr
