// deflate_rows_plan.h -- the host rules of the rows deflate engine (deflate_dyn.hip: zng_rocm_deflate_*_dev, and through
// deflate_blocks.h the BGZF writer, compress_streams2 / members, the dictionary and the window calls): the sizes, the argument
// checks, the cut of a job list into rounds, and the planner that cuts streams into segments and segments into blocks -- every
// offset the four kernels use.  Plain C++ over integers and the structs of zng_rocm.h, no HIP and no Workspace;
// tests/test_deflate_rows_plan_cpu.py drives it through tests/c/deflate_rows_plan_driver.cpp without a GPU.
//
//   stream    positions count from the first history byte: position q < dict names history byte q, dict + i plaintext byte i
//             (dict = the job's dict_len, or the window of the one shared dictionary object), so `in` is plaintext - dict
//   segment   seg_bytes of plaintext, [seg_start, seg_end): one workgroup of K1.  Its token scratch (bitmap, distances) begins
//             at the batch that holds seg_start: first = seg_start - seg_start % kRowsBatch
//   block     the tokens of a segment that start in [blo, bhi): borders at first + k * kSubBytes, where K1 snapshots its
//             histogram (snapshot k * kMaxSub + sub of segment k).  An empty stream is one segment of one empty block.
//   the stream's last block carries 0x80000000 in `stream` and, unless ZNG_ROCM_BLOCK_NOT_FINAL, BFINAL (is_last)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zng_rocm.h"
#include "deflate_window_plan.h"      // win_check; kWinBatch, kWinPrimeMax

namespace zr {

// ---- constants and sizes ------------------------------------------------------------------------------------------------
constexpr uint32_t kRowsBatch = kWinBatch;     // the matcher's batch (kRowBatch of deflate_rows.h; deflate_dyn.hip asserts it)
constexpr uint32_t kSegBytes = 512u << 10;     // plaintext per segment: the largest, and ...
constexpr uint32_t kSegBytesMin = 128u << 10;  // ... the smallest.  A segment is one workgroup and one CU holds one
                                               // workgroup, so a stream is cut into at least ~2 segments per CU when
                                               // it is long enough (each segment re-inserts the 32 KiB before it:
                                               // 6 % extra work at 512 KiB, 25 % at 128 KiB)
inline uint32_t segment_bytes(size_t in_len, int cus) {
    uint32_t seg = kSegBytes;
    while (seg > kSegBytesMin && in_len / seg < 2u * (size_t)cus) seg >>= 1;
    return seg;
}
constexpr uint32_t kPrime = kWinPrimeMax;      // history primed from in front of a segment; the most a dict_len may be
constexpr int      kHistWords = 320;           // 288 literal/length + 32 distance counts
// A segment is written as several BLOCKS, one per kSubBytes of positions (counted from the segment's first batch): zlib's
// blocks hold about as much (lit_bufsize 16384 symbols), the codes follow the data more closely, a block may be stored
// (<= 65535 bytes), and -- what it was done for -- every block start is a place where a parallel inflater can cut the
// stream (inflate_large.hip, inflate_threads.cpp): one block per 512 KiB segment gave a 256 MiB stream 434 parts.
constexpr uint32_t kSubBatches = 60;
constexpr uint32_t kSubBytes = kSubBatches * kRowsBatch;         // 61440
constexpr uint32_t kMaxSub = (kSegBytes + kRowsBatch + kSubBytes - 1) / kSubBytes + 1;     // histogram snapshots per segment

// scratch a segment of `bytes` plaintext bytes needs: bitmap words / distance entries (its first batch may start up to
// one batch in front of the segment)
inline size_t seg_bm_words(uint32_t bytes) { return ((size_t)bytes + 2u * kRowsBatch) / 64 + 2; }
inline size_t seg_d16_entries(uint32_t bytes) { return (((size_t)bytes + 2u * kRowsBatch) / 4 + 8) & ~(size_t)3; }
// output slot of a block of n positions: <= 9 bits per literal for an almost flat alphabet, + header (< 400 bytes) + trailer;
// 4-byte aligned
inline size_t seg_slot_bytes(uint32_t n) { return (((size_t)n * 9 + 7) / 8 + 1024 + 3) & ~(size_t)3; }

inline uint64_t rows_stream_segments(uint32_t in_len, uint32_t seg_bytes) {
    return in_len ? ((uint64_t)in_len + seg_bytes - 1) / seg_bytes : 1u;
}
// zng_rocm_deflate_bound: what the engine may write for n bytes cut into segments of kSegBytesMin, the most there can be
// (1032 bytes of block overhead per segment).  Covers level 0 too: 5 bytes per 65535 (deflate_stored) is far below n / 8
inline uint64_t rows_deflate_bound(uint64_t n) {
    const uint64_t nseg = n ? (n + kSegBytesMin - 1) / kSegBytesMin : 1;
    return n + n / 8 + nseg * 1032 + 16;
}

// ---- the tables the kernels read -------------------------------------------------------------------------------------------
// one SEGMENT (K1: the matchers of deflate_rows_body.h and deflate_rle.h).  They read in, bm_off, d16_off, seg_start and seg_end;
// the rest is left from the time one job struct served all four kernels and is zero.  The layout stays: without those fields the
// kernels need the same registers, LDS and scratch, but the compiler allocates the matchers' registers differently, and
// zng_rocm_deflate_dev then measured 0.3 % slower on MI355X (profiles/deflate_rows_plan_parity_v1.json)
struct SegJob {
    const uint8_t *in;        // stream base (position 0)
    uint8_t       *out;
    uint8_t       *dst;
    uint64_t       dst_cap;
    uint64_t       bm_off;    // this segment's token-start bitmap: u64 words from the scratch base
    uint64_t       d16_off;   // this segment's match distances: u16 entries from the scratch base
    uint32_t       seg_start, seg_end;
    uint32_t       out_cap;
    uint32_t       is_last;
    uint32_t       first_seg;
    uint32_t       stream;
};

// one BLOCK of the output (K2 .. K4): the tokens of its segment that start in [blo, bhi)
struct BlkJob {
    const uint8_t *in;        // stream base (position 0)
    uint8_t       *out;       // this block's output slot (4-byte aligned)
    uint8_t       *dst;       // the stream's output buffer (what K4 packs into)
    uint64_t       dst_cap;
    uint64_t       bm_off, d16_off;       // its segment's token scratch
    uint32_t       seg_start, seg_end;    // its segment
    uint32_t       blo, bhi;
    uint32_t       hist_idx, hist_prev;   // histogram snapshot of this block's end; 1 if the snapshot before it is the block's begin
    uint32_t       out_cap;
    uint32_t       is_last;               // the block that carries BFINAL
    uint32_t       first_seg;             // index of the first BLOCK of this block's stream
    uint32_t       stream;                // row of the per-stream result table; 0x80000000 set on the stream's last block
};
constexpr uint32_t kRowsLastBlock = 0x80000000u;

// ---- the checks -------------------------------------------------------------------------------------------------------------
constexpr uint32_t kRowsBlockFlags = ZNG_ROCM_BLOCK_NOT_FINAL | ZNG_ROCM_BLOCK_SYNC_FLUSH;
constexpr int      kRowsBufError = -5;         // Z_BUF_ERROR
constexpr int      kRowsStrategyMax = 4;       // Z_FIXED

enum RowsEntry { kRowsEntryBlock, kRowsEntryAsync, kRowsEntryStreams };    // zng_rocm_deflate_window_block_dev, _async_dev, _window_streams_dev
// what a check found, in the order the calls look: every one is ZNG_ROCM_EINVAL but the last
enum RowsRefusal { kRowsTaken = 0, kRowsStrategy, kRowsWindow, kRowsNull, kRowsLevel, kRowsDictFlags, kRowsTooLong, kRowsBound };
inline int rows_status(RowsRefusal r) { return r == kRowsTaken ? ZNG_ROCM_OK : r == kRowsBound ? kRowsBufError : ZNG_ROCM_EINVAL; }
inline const char *rows_refusal_text(RowsEntry e, RowsRefusal r) {
    switch (r) {
    case kRowsStrategy: return "strategy is outside 0..4";
    case kRowsWindow: return "window_bits is outside 9..15";
    case kRowsNull: return "null buffer";
    case kRowsLevel: return e == kRowsEntryBlock ? "level is outside 0..9" : "level is outside 1..9 (level 0: zng_rocm_deflate_block_dev per stream)";
    case kRowsDictFlags: return "dict_len above 32768 or unknown flags";
    case kRowsTooLong: return "streams of 4 GiB and more are not supported by the 32-bit position format";
    case kRowsBound: return "out_cap below zng_rocm_deflate_bound()";
    default: return "";
    }
}
// the call itself, before any job is looked at.  null_args: a pointer of the call's own (out_len, d_result, the job list, out_lens)
// is null.  A call without jobs is taken once strategy and window are in range, whatever else it says: the caller returns
// ZNG_ROCM_OK then.  (ZNG_ROCM_ENODEV, which needs the context, comes before all of this.)
inline RowsRefusal rows_call_check(RowsEntry e, int level, int strategy, int window_bits, uint64_t njobs, bool null_args) {
    if (strategy < 0 || strategy > kRowsStrategyMax) return kRowsStrategy;
    if (win_check(0, window_bits)) return kRowsWindow;
    if (!njobs) return kRowsTaken;
    if (null_args) return kRowsNull;
    if (level < (e == kRowsEntryBlock ? 0 : 1) || level > 9) return kRowsLevel;
    return kRowsTaken;
}
// one job.  in_len and out_cap are as wide as the one-stream calls take them.  (A history without plaintext needs `in` as well:
// only the streams call has ever said so.)
inline RowsRefusal rows_job_check(RowsEntry e, const void *in, const void *out, uint64_t in_len, uint32_t dict_len, uint32_t flags,
                                  uint64_t out_cap) {
    if (!out || (in_len && !in) || (e == kRowsEntryStreams && dict_len && !in)) return kRowsNull;
    if (dict_len > kPrime || (flags & ~kRowsBlockFlags)) return kRowsDictFlags;
    if (in_len + dict_len >= (1ull << 32) - kSegBytes) return kRowsTooLong;
    if (out_cap < rows_deflate_bound(in_len)) return kRowsBound;
    return kRowsTaken;
}
// what the one-stream calls (block, async) refuse
inline RowsRefusal rows_one_check(RowsEntry e, int level, int strategy, int window_bits, bool null_args, const void *in, const void *out,
                                  uint64_t in_len, uint32_t dict_len, uint32_t flags, uint64_t out_cap) {
    if (RowsRefusal r = rows_call_check(e, level, strategy, window_bits, 1, null_args)) return r;
    return rows_job_check(e, in, out, in_len, dict_len, flags, out_cap);
}
// what the streams call refuses: the call's own, then the first refusal in job order, its job in *bad
inline RowsRefusal rows_streams_check(int level, int strategy, int window_bits, const zng_rocm_stream_job *jobs, uint64_t njobs,
                                      bool null_out_lens, uint64_t *bad) {
    if (RowsRefusal r = rows_call_check(kRowsEntryStreams, level, strategy, window_bits, njobs, !jobs || null_out_lens)) return r;
    for (uint64_t i = 0; i < njobs; ++i) {
        const zng_rocm_stream_job &j = jobs[i];
        if (RowsRefusal r = rows_job_check(kRowsEntryStreams, j.in, j.out, j.in_len, j.dict_len, j.flags, j.out_cap)) {
            *bad = i;
            return r;
        }
    }
    return kRowsTaken;
}
// the job of the one-stream calls, once checked; its room does not fit out_cap: RowsPlan::cap_one carries it
inline zng_rocm_stream_job rows_one_job(const uint8_t *in, uint8_t *out, uint64_t in_len, uint32_t dict_len, uint32_t flags) {
    return zng_rocm_stream_job{in, out, (uint32_t)in_len, 0u, dict_len, flags};
}

// ---- the rounds -------------------------------------------------------------------------------------------------------------
// the round that begins at job `first` ends in front of the job returned: jobs are taken while their bytes stay within `room`;
// a job is never split, so a round has at least one job, however long.  count_dict: a job's history counts as well
// (zng_rocm_deflate_window_streams_dev; compress_streams_plan.h counts the plaintext alone)
inline uint64_t rows_round_end(const zng_rocm_stream_job *jobs, uint64_t njobs, uint64_t first, uint64_t room, bool count_dict) {
    uint64_t last = first, bytes = 0;
    while (last < njobs) {
        const uint64_t n = (uint64_t)jobs[last].in_len + (count_dict ? jobs[last].dict_len : 0u);
        if (last != first && bytes + n > room) break;
        bytes += n;
        ++last;
    }
    return last;
}
constexpr uint64_t kRowsRoundBytes = 4ull << 30;

// ---- the planner ------------------------------------------------------------------------------------------------------------
// dst_cap of a stream's blocks (what K3 holds the compressed size against, and where K4 stops)
enum RowsCapRule {
    kRowsCapJob,       // the job's own out_cap
    kRowsCapOne,       // cap_one for stream 0: a single stream whose room does not fit the job's 32 bits
    kRowsCapKeep       // none: the caller places the blocks itself
};
struct RowsPlan {
    const zng_rocm_stream_job *jobs;
    size_t                     njobs;
    uint32_t                   seg_bytes;
    uint32_t                   shared_window;     // the window of the one dictionary object behind every stream, or 0: each job's dict_len
    RowsCapRule                cap_rule;
    uint64_t                   cap_one;
};
// step 1: how many segments, how many blocks at the most, and the scratch that depends on nothing else
struct RowsCounts {
    size_t nseg, max_blk;
    size_t seg_tab;           // bytes of SegJob[nseg], rounded up to 256: BlkJob[] follows
    size_t table_bytes;       // SegJob[nseg] | BlkJob[max_blk], pinned and device
    size_t sizes_bytes;       // {compressed size, does-not-fit flag} per stream
    size_t hist_word;         // block lengths u32[max_blk], then from this word on the histogram snapshots ...
    size_t len_hist_bytes;    // ... of every segment: both
    size_t scan_bytes;        // K3: excl[nb + 1] | dst_off[nb + 1] | sizes
};
inline RowsCounts rows_plan_count(const RowsPlan &p) {
    RowsCounts c;
    c.nseg = 0;
    for (size_t s = 0; s < p.njobs; ++s) c.nseg += (size_t)rows_stream_segments(p.jobs[s].in_len, p.seg_bytes);
    c.max_blk = c.nseg * kMaxSub;
    c.seg_tab = (c.nseg * sizeof(SegJob) + 255) & ~(size_t)255;
    c.table_bytes = c.seg_tab + c.max_blk * sizeof(BlkJob);
    c.sizes_bytes = p.njobs * 2 * sizeof(unsigned long long);
    c.hist_word = (c.max_blk + 3) & ~(size_t)3;
    c.len_hist_bytes = c.max_blk * sizeof(uint32_t) + 64 + c.nseg * (size_t)kMaxSub * kHistWords * sizeof(uint32_t);
    c.scan_bytes = (2 * c.max_blk + 2 + 2 * p.njobs) * sizeof(unsigned long long);
    return c;
}
// step 2: the tables, into seg[nseg] and blk[max_blk] of the caller.  A block's `out` is its slot's OFFSET in the slot scratch
// (the caller adds the base once it has reserved slot_total bytes).
struct RowsTotals {
    size_t nb;                // blocks written
    size_t slot_total;        // bytes of all slots
    size_t bm_total;          // u64 words of all bitmaps
    size_t d16_total;         // u16 entries of all distance arrays
};
inline RowsTotals rows_plan_fill(const RowsPlan &p, SegJob *seg, BlkJob *blk) {
    RowsTotals t = {0, 0, 0, 0};
    size_t k = 0;
    for (size_t s = 0; s < p.njobs; ++s) {
        const zng_rocm_stream_job &j = p.jobs[s];
        const uint32_t dict = p.shared_window ? p.shared_window : j.dict_len;    // (behind a shared window no job has a dict_len of its own)
        const size_t n = (size_t)rows_stream_segments(j.in_len, p.seg_bytes), b0 = t.nb;
        for (size_t i = 0; i < n; ++i, ++k) {
            // positions count from the first history byte: the segments' own priming reaches into it
            const uint32_t a = dict + (uint32_t)(i * p.seg_bytes);
            const uint32_t b = dict + (uint32_t)((i + 1) * (size_t)p.seg_bytes < j.in_len ? (i + 1) * (size_t)p.seg_bytes : j.in_len);
            seg[k] = SegJob();
            seg[k].in = (const uint8_t *)((uintptr_t)j.in - dict);      // behind a shared window: never read below in + dict
            seg[k].bm_off = t.bm_total;
            seg[k].d16_off = t.d16_total;
            seg[k].seg_start = a;
            seg[k].seg_end = b;
            // The segment's blocks: one per kSubBytes of positions counted from its first batch.  None is empty but the one of
            // an empty stream: first <= a < first + kSubBytes and the last begins below b, so blo < bhi whenever a < b.
            const uint32_t first = a - a % kRowsBatch;
            const uint32_t nsub = b > first ? (b - first + kSubBytes - 1) / kSubBytes : 1u;
            for (uint32_t sub = 0; sub < nsub; ++sub) {
                const uint32_t p0 = first + sub * kSubBytes, p1 = p0 + kSubBytes;
                BlkJob &q = blk[t.nb++];
                q.in = seg[k].in;
                q.dst = j.out;
                q.dst_cap = p.cap_rule == kRowsCapKeep ? ~0ull : (p.cap_rule == kRowsCapOne && s == 0 ? p.cap_one : j.out_cap);
                q.bm_off = t.bm_total;
                q.d16_off = t.d16_total;
                q.seg_start = a;
                q.seg_end = b;
                q.blo = p0 > a ? p0 : a;
                q.bhi = p1 < b ? p1 : b;
                q.hist_idx = (uint32_t)(k * kMaxSub + sub);
                q.hist_prev = sub > 0 ? 1u : 0u;
                q.out_cap = (uint32_t)seg_slot_bytes(q.bhi - q.blo + 258u);
                q.is_last = 0;
                q.first_seg = (uint32_t)b0;
                q.stream = (uint32_t)s;
                q.out = (uint8_t *)t.slot_total;          // offset for now
                t.slot_total += q.out_cap;
            }
            t.bm_total += seg_bm_words(b - a);
            t.d16_total += seg_d16_entries(b - a);
        }
        blk[t.nb - 1].stream |= kRowsLastBlock;                                               // the stream's last block ...
        blk[t.nb - 1].is_last = (j.flags & ZNG_ROCM_BLOCK_NOT_FINAL) == 0 ? 1u : 0u;          // ... carries BFINAL
    }
    return t;
}

}  // namespace zr
