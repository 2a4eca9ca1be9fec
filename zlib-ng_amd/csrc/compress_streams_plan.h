// compress_streams_plan.h -- the rules of zng_rocm_compress_streams2_dev and zng_rocm_compress_members_dev (compress_streams.hip):
// many device-resident streams deflated at any level and strategy and wrapped as raw / zlib / gzip members, each in its own
// buffer or all back to back in one destination.  Plain C++ over integers, no HIP: the argument checks, the cut of the job list
// into rounds, the stored (level 0) sizes and block headers, and the bounds; the header and trailer bytes by format, level and
// strategy are the canonical writer of framing_parse.h.  The rules the kernels apply as well are written once for host and
// device; tests/test_compress_streams_plan_cpu.py drives them through tests/c/compress_streams_plan_driver.cpp without a GPU.
//
// A member is  header | raw deflate data | trailer:
//   format 0 raw    nothing | data | nothing
//   format 1 zlib   CMF FLG (deflate.c:868-886)             | data | Adler-32, most significant byte first (deflate.c:1098-1101)
//   format 2 gzip   1f 8b 08 00 mtime=0 XFL OS=3 (:902-913)  | data | CRC-32, ISIZE, least significant first (deflate.c:1091-1096)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zng_rocm.h"
#include "deflate_rows_plan.h" // the engine's bound, its dictionary limit, the round cut
#include "framing_parse.h"     // the wrapper's rules
#include "gf2.h"      // ZR_HD

namespace zr {

constexpr uint32_t kCsMaxStored = 65535u;             // MAX_STORED: the most one stored block holds (deflate_stored.c:22)
constexpr uint32_t kCsStoredHead = 5u;                // BFINAL/BTYPE byte, LEN, NLEN (RFC 1951 3.2.4)
constexpr uint32_t kCsDictMax = kPrime;
constexpr uint32_t kCsBlockFlags = ZNG_ROCM_BLOCK_NOT_FINAL | ZNG_ROCM_BLOCK_SYNC_FLUSH;
constexpr uint64_t kCsRoundDefault = 4ull << 30;      // plaintext per round when the caller says 0
constexpr int      kCsBufError = -5;                  // Z_BUF_ERROR
constexpr int      kCsLevelRefused = -2;              // cs_level of a level the calls refuse

// ---- the arguments ------------------------------------------------------------------------------------------------------
// level as the caller gives it (-1 = 6, deflate.c:296) -> 0 .. 9, or kCsLevelRefused
ZR_HD int cs_level(int level) { return level == -1 ? 6 : (level >= 0 && level <= 9 ? level : kCsLevelRefused); }
ZR_HD bool cs_format_ok(int format) { return format >= 0 && format <= 2; }
ZR_HD bool cs_strategy_ok(int strategy) { return strategy >= 0 && strategy <= 4; }

// ---- the wrapper --------------------------------------------------------------------------------------------------------
// the canonical writer of framing_parse.h under this plan's names: no rule is restated here
ZR_HD uint32_t cs_head_bytes(int format) { return wrapper_head_bytes(format); }
ZR_HD uint32_t cs_tail_bytes(int format) { return wrapper_tail_bytes(format); }
ZR_HD uint32_t cs_zlib_flevel(int level, int strategy) { return wrapper_zlib_flevel(level, strategy); }
ZR_HD uint32_t cs_gzip_xfl(int level, int strategy) { return wrapper_gzip_xfl(level, strategy); }
ZR_HD uint8_t cs_header_byte(int format, int level, int strategy, uint32_t k, int window_bits = 15) {
    return wrapper_header_byte(format, level, strategy, k, window_bits);
}
ZR_HD uint8_t cs_trailer_byte(int format, uint32_t k, uint32_t check, uint32_t n) { return wrapper_trailer_byte(format, k, check, n); }

// ---- level 0 ------------------------------------------------------------------------------------------------------------
// deflate_stored for a complete input and an output that holds everything (deflate_stored.c:46-95): blocks of 65535 bytes, an
// empty input is one empty block; the last block carries BFINAL unless ZNG_ROCM_BLOCK_NOT_FINAL, and behind a block that is not
// final ZNG_ROCM_BLOCK_SYNC_FLUSH adds the empty stored block 00 00 00 ff ff (deflate.c:1064-1076)
ZR_HD uint64_t cs_stored_blocks(uint64_t n) { return n ? (n + kCsMaxStored - 1u) / kCsMaxStored : 1u; }
ZR_HD bool cs_stored_marker(uint32_t flags) {
    return (flags & ZNG_ROCM_BLOCK_NOT_FINAL) && (flags & ZNG_ROCM_BLOCK_SYNC_FLUSH);
}
ZR_HD uint64_t cs_stored_bytes(uint64_t n, uint32_t flags) {
    return n + kCsStoredHead * cs_stored_blocks(n) + (cs_stored_marker(flags) ? kCsStoredHead : 0u);
}
// bytes of block b (0 .. cs_stored_blocks - 1)
ZR_HD uint32_t cs_stored_block_len(uint64_t n, uint64_t b) {
    const uint64_t left = n - b * kCsMaxStored;
    return left < kCsMaxStored ? (uint32_t)left : kCsMaxStored;
}
// byte k (0 .. 4) of the header of a stored block of len bytes
ZR_HD uint8_t cs_stored_byte(uint32_t k, uint32_t len, bool final_block) {
    const uint32_t nlen = ~len & 0xffffu;
    return k == 0u ? (uint8_t)(final_block ? 1u : 0u) : k < 3u ? (uint8_t)(len >> (8u * (k - 1u))) : (uint8_t)(nlen >> (8u * (k - 3u)));
}

// ---- the bounds ---------------------------------------------------------------------------------------------------------
// zng_rocm_deflate_bound (deflate_rows_plan.h); covers the stored form
inline uint64_t cs_deflate_bound(uint64_t n) { return rows_deflate_bound(n); }
// zng_rocm_compress_bound: + ZLIB_WRAPLEN 6 / GZIP_WRAPLEN 18 (zutil.h:68-69)
inline uint64_t cs_bound(uint64_t n, int format) { return cs_deflate_bound(n) + (format == 1 ? 6u : format == 2 ? 18u : 0u); }

// ---- the checks ---------------------------------------------------------------------------------------------------------
// what both calls refuse about the call itself, before any job is looked at: 0 or ZNG_ROCM_EINVAL.  `results` is d_results of
// streams2 or d_offsets of members; the pointers are looked at only for being null
inline int cs_call_check(int format, int level, int strategy, const void *jobs, uint64_t njobs, const void *results) {
    if (!cs_format_ok(format) || cs_level(level) == kCsLevelRefused || !cs_strategy_ok(strategy)) return ZNG_ROCM_EINVAL;
    if (njobs && (!jobs || !results)) return ZNG_ROCM_EINVAL;
    return ZNG_ROCM_OK;
}
// the one destination of members: it may be null only where it has no room
inline int cs_file_check(const void *dst, uint64_t dst_cap) { return (!dst && dst_cap) ? ZNG_ROCM_EINVAL : ZNG_ROCM_OK; }
// one job.  per_job_out: streams2, where the job's own out / out_cap take the member (members: neither is looked at)
inline int cs_job_check(int format, const zng_rocm_stream_job &j, bool per_job_out) {
    if ((j.in_len || j.dict_len) && !j.in) return ZNG_ROCM_EINVAL;
    if (j.dict_len > kCsDictMax || (j.flags & ~kCsBlockFlags)) return ZNG_ROCM_EINVAL;
    if (format != 0 && (j.dict_len || j.flags)) return ZNG_ROCM_EINVAL;
    if (cs_bound(j.in_len, format) > 0xffffffffull) return ZNG_ROCM_EINVAL;
    if (per_job_out) {
        if (!j.out) return ZNG_ROCM_EINVAL;
        if (j.out_cap < cs_bound(j.in_len, format)) return kCsBufError;
    }
    return ZNG_ROCM_OK;
}
// the whole job list: the first refusal in job order, its job in *bad
inline int cs_jobs_check(int format, const zng_rocm_stream_job *jobs, uint64_t njobs, bool per_job_out, uint64_t *bad) {
    for (uint64_t i = 0; i < njobs; ++i)
        if (int rc = cs_job_check(format, jobs[i], per_job_out)) {
            if (bad) *bad = i;
            return rc;
        }
    return ZNG_ROCM_OK;
}

// ---- the shared preset dictionary (zng_rocm_compress_streams2_dict_dev, zng_rocm_compress_members_dict_dev) --------------
// The same members with one dictionary object as every stream's history: format 0 raw (deflateSetDictionary on a raw stream),
// format 1 zlib with the 6-byte FDICT header of framing_parse.h and the Adler-32 of the plaintext alone as the trailer; gzip has
// no dictionary.  Levels 1..9 go through the dictionary form of the rows matcher, level 0 reads no dictionary byte.  Z_HUFFMAN_ONLY
// and Z_RLE have another front end (deflate_rle.h) and at most one byte of history to gain: they are refused here.
ZR_HD bool cs_dict_format_ok(int format) { return format == 0 || format == 1; }
ZR_HD bool cs_dict_strategy_ok(int strategy) { return strategy == 0 || strategy == 1 || strategy == 4; }
ZR_HD uint32_t cs_dict_head_bytes(int format) { return wrapper_dict_head_bytes(format); }
ZR_HD uint8_t cs_dict_header_byte(int level, int strategy, uint32_t dictid, uint32_t k) {
    return wrapper_dict_header_byte(level, strategy, dictid, k);
}
// zng_rocm_compress_streams2_dict_bound: the DICTID's four bytes on top of the plain bound; 0 for a refused format
inline uint64_t cs_dict_bound(uint64_t n, int format) {
    return cs_dict_format_ok(format) ? cs_bound(n, format) + (format == 1 ? 4u : 0u) : 0u;
}
// the call itself; `dict` is looked at only for being null
inline int cs_dict_call_check(int format, int level, int strategy, const void *dict, const void *jobs, uint64_t njobs,
                              const void *results) {
    if (!dict || !cs_dict_format_ok(format) || cs_level(level) == kCsLevelRefused || !cs_dict_strategy_ok(strategy)) return ZNG_ROCM_EINVAL;
    if (njobs && (!jobs || !results)) return ZNG_ROCM_EINVAL;
    return ZNG_ROCM_OK;
}
// one job: as cs_job_check, but the history is the object's -- a dict_len of the job's own is refused -- and the bound is
// cs_dict_bound
inline int cs_dict_job_check(int format, const zng_rocm_stream_job &j, bool per_job_out) {
    if (j.in_len && !j.in) return ZNG_ROCM_EINVAL;
    if (j.dict_len || (j.flags & ~kCsBlockFlags)) return ZNG_ROCM_EINVAL;
    if (format != 0 && j.flags) return ZNG_ROCM_EINVAL;
    if (cs_dict_bound(j.in_len, format) > 0xffffffffull) return ZNG_ROCM_EINVAL;
    if (per_job_out) {
        if (!j.out) return ZNG_ROCM_EINVAL;
        if (j.out_cap < cs_dict_bound(j.in_len, format)) return kCsBufError;
    }
    return ZNG_ROCM_OK;
}
inline int cs_dict_jobs_check(int format, const zng_rocm_stream_job *jobs, uint64_t njobs, bool per_job_out, uint64_t *bad) {
    for (uint64_t i = 0; i < njobs; ++i)
        if (int rc = cs_dict_job_check(format, jobs[i], per_job_out)) {
            if (bad) *bad = i;
            return rc;
        }
    return ZNG_ROCM_OK;
}

// ---- the rounds ---------------------------------------------------------------------------------------------------------
// the round that begins at job `first` ends in front of the job returned: jobs are taken while their plaintext stays within
// round_bytes (0 = 4 GiB); a job is never split, so a round has at least one job, however long
inline uint64_t cs_round_end(const zng_rocm_stream_job *jobs, uint64_t njobs, uint64_t first, uint64_t round_bytes) {
    return rows_round_end(jobs, njobs, first, round_bytes ? round_bytes : kCsRoundDefault, false);
}
inline uint64_t cs_rounds(const zng_rocm_stream_job *jobs, uint64_t njobs, uint64_t round_bytes) {
    uint64_t rounds = 0;
    for (uint64_t first = 0; first < njobs; first = cs_round_end(jobs, njobs, first, round_bytes)) ++rounds;
    return rounds;
}

}  // namespace zr
