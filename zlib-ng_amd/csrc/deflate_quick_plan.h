// deflate_quick_plan.h -- the rules of the level-1 class kernels (deflate_quick_kernel, its dictionary form and the one-wave form of
// deflate_stream.hip) that hold ONE stream to the whole range the calls accept: how the bit ring is streamed out, how the lanes'
// Adler-32 sums become the row's check word, and which jobs zng_rocm_deflate_quick_dev and launch_deflate_quick_dict take.  Plain
// C++ over integers, no HIP; tests/test_deflate_quick_plan_cpu.py drives them through tests/c/deflate_quick_plan_driver.cpp without
// a GPU, against models in Python's unbounded integers.
//
//   the bound     in_len + ceil(in_len / 8) + 13, rounded up to 16 (3 header bits, at most 9 bits per byte, 7 EOB bits, the
//                 sync-flush marker).  out_cap is 32 bits wide, so the largest stream is the largest in_len whose bound fits:
//                 kQuickMaxInLen = 3 817 748 681 (3.55 GiB).  Its output is up to 9 * in_len + 10 bits = 8 * 2^32 less a little:
//   the cursor    counts the bits placed so far MODULO 2^32 (it wraps every 512 MiB of output; up to seven times in one stream).
//                 `flushed` is the TRUE number of whole words written (< 2^30) and serves the address.  Fewer than kRingWords
//                 words are ever pending, so pending bits = cursor - 32 * flushed modulo 2^32 is exact: one shift, one subtract,
//                 one compare per batch, as many as the rule that compared cursor >> 5 with flushed and broke behind the wrap.
//   the check     a lane keeps A = sum of its bytes and B = sum of (n - p) * byte in 64 bits: below 2^63 for every n < 2^32.  The
//                 sum over a wave's 64 lanes is about byte * n^2 / 8 and passes 2^64 from 726 MiB of 0xff on, so every lane is
//                 reduced modulo 65521 BEFORE lanes are added; all later sums stay below 2^24.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zng_rocm.h"
#include "gf2.h"      // ZR_HD, kAdlerBase

namespace zr {

// The bit ring: output bit b of the stream lives in ring[(b / 32) & (kRingWords - 1u)] while it is being assembled.  A batch
// produces at most 256 nine-bit literals = 72 words; words are streamed out once 128 are complete, 32 (one 128-byte
// line) at a time, so fewer than 128 + 72 + 32 < 512 are ever pending.
constexpr uint32_t kRingWords = 512;       // 2 KiB: with the 16 KiB head table still eight workgroups per CU
constexpr uint32_t kFlushWords = 128;
constexpr uint32_t kQuickBatchBits = 256u * 9u;          // the most one batch places

// ---- the bound and the largest stream -------------------------------------------------------------------------------------------
// 3 header bits + at most 9 bits per input byte (a match of >= 4 bytes costs <= 31 bits) + 7 EOB bits,
// cf. DEFLATE_QUICK_OVERHEAD / DEFLATE_BLOCK_OVERHEAD (zutil.h:71-79, deflate.c:773-777); rounded so that
// consecutive streams stay 16-byte aligned.
constexpr uint64_t quick_bound(uint64_t source_len) {
    return (source_len + ((source_len + 7) >> 3) + 8 + 5 + 15) & ~(uint64_t)15;      // + the sync-flush terminator of a non-final block
}
constexpr uint32_t kQuickMaxInLen = 3817748681u;         // the largest in_len whose bound an out_cap can state
constexpr uint32_t kQuickMaxHistory = 32768u;            // dict_len of a job, the window of a dictionary object
static_assert(quick_bound(kQuickMaxInLen) <= 0xffffffffull && quick_bound((uint64_t)kQuickMaxInLen + 1) > 0xffffffffull,
              "kQuickMaxInLen is the last length whose bound fits 32 bits");
static_assert((uint64_t)kQuickMaxInLen + kQuickMaxHistory <= 0xffffffffull, "history + plaintext are positions of 32 bits");
static_assert(3ull + 9ull * kQuickMaxInLen + 7ull + 3ull < 8ull << 32, "the cursor wraps at most seven times");

// ---- the flush rule -------------------------------------------------------------------------------------------------------------
// cursor: bits placed so far modulo 2^32; flushed: whole words already written, true.  Bits complete in the ring and not written:
ZR_HD uint32_t quick_pending_bits(uint32_t cursor, uint32_t flushed) { return cursor - (flushed << 5); }
// How many ring words to stream out now, behind out + 4 * flushed: nothing while fewer than keep_below are complete; whole
// 128-byte lines in the batch loop (keep_below = kFlushWords), every complete word at the end of the stream (keep_below = 1).
// The kernels ask in two steps, so that a batch without a flush pays for the question alone: is a flush due at `bits` pending
// bits, and how many words does it write (never 0 when one is due).
ZR_HD bool quick_flush_due(uint32_t bits, uint32_t keep_below) { return bits >= (keep_below << 5); }
ZR_HD uint32_t quick_flush_count(uint32_t bits, uint32_t keep_below) { return keep_below > 1u ? (bits >> 5) & ~31u : bits >> 5; }
ZR_HD uint32_t quick_flush_words(uint32_t cursor, uint32_t flushed, uint32_t keep_below) {
    const uint32_t bits = quick_pending_bits(cursor, flushed);
    return quick_flush_due(bits, keep_below) ? quick_flush_count(bits, keep_below) : 0u;
}

// The end of the stream: the partial word, the end-of-block code (seven 0 bits, zng_emit_end_block, trees_emit.h:169-180), with
// `sync` the 3-bit header of an empty stored block, padding to a byte and LEN = 0, NLEN = 0xffff (deflate.c:1064-1076).
struct QuickTail {
    uint32_t word;        // the word the cursor is in (true index; == flushed once every complete word is written)
    uint32_t spill;       // 1: partial word + EOB fill that word, which is written whole at `word`
    uint32_t first;       // byte offset of the bytes written singly: 4 * (word + spill)
    uint32_t nbytes;      // how many of them carry the last bits (0..5); behind them the 4 marker bytes with `sync`
    uint32_t bytes;       // the stream's length
};
ZR_HD QuickTail quick_tail(uint32_t cursor, uint32_t flushed, bool sync) {
    QuickTail t;
    t.word = flushed + (quick_pending_bits(cursor, flushed) >> 5);
    uint32_t cbits = (cursor & 31u) + 7u;
    t.spill = cbits >= 32u ? 1u : 0u;
    cbits -= 32u * t.spill;
    if (sync) cbits += 3u;
    t.first = (t.word + t.spill) * 4u;
    t.nbytes = (cbits + 7u) / 8u;
    t.bytes = t.first + t.nbytes + (sync ? 4u : 0u);
    return t;
}

// ---- the Adler-32 fold ----------------------------------------------------------------------------------------------------------
// Linear form: over the plaintext positions p a lane visits, accA = sum of byte, accB = sum of (n - p) * byte.
// One lane's sum, reduced; these are what lanes, waves and the workgroup add up (256 * 65520 < 2^24)
ZR_HD uint32_t quick_adler_lane(unsigned long long acc) { return (uint32_t)(acc % kAdlerBase); }
// the row's second word from the sums of all lanes' reduced values and the plaintext's length
ZR_HD uint32_t quick_adler_row(unsigned long long sum_a, unsigned long long sum_b, uint32_t len) {
    const unsigned long long A = sum_a % kAdlerBase, B = sum_b % kAdlerBase;
    return (uint32_t)(((1u + A) % kAdlerBase) | ((((unsigned long long)len + B) % kAdlerBase) << 16));
}

// ---- the job check --------------------------------------------------------------------------------------------------------------
// What both entry points demand of a job; 0 or ZNG_ROCM_EINVAL.  dict_form: the history is a dictionary object's window of
// `window` bytes and the job has none of its own; else the job's dict_len bytes in front of `in` (window is not looked at).
constexpr const char *kQuickJobRule =
    "job %zu: out must be 4-byte aligned with out_cap >= zng_rocm_deflate_quick_bound(in_len), in_len at most 3817748681, "
    "known flags, and dict_len at most 32768 (0 with a dictionary object)";
ZR_HD int quick_job_check(const zng_rocm_stream_job &j, bool dict_form, uint32_t window) {
    if (!j.out || ((uintptr_t)j.out & 3u) || (j.in_len && !j.in)) return ZNG_ROCM_EINVAL;
    if (j.in_len > kQuickMaxInLen || j.out_cap < quick_bound(j.in_len)) return ZNG_ROCM_EINVAL;
    if (j.flags & ~(uint32_t)(ZNG_ROCM_BLOCK_NOT_FINAL | ZNG_ROCM_BLOCK_SYNC_FLUSH)) return ZNG_ROCM_EINVAL;
    if (dict_form ? (j.dict_len != 0u || window > kQuickMaxHistory) : (j.dict_len > kQuickMaxHistory || (j.dict_len && !j.in)))
        return ZNG_ROCM_EINVAL;
    return ZNG_ROCM_OK;
}

}  // namespace zr
