// deflate_blocks.h -- the one entry into the rows engine (deflate_dyn.hip: lz_rows_kernel, emit_dynamic_kernel,
// segments_scan_kernel; the tables and every host rule: deflate_rows_plan.h), and what it leaves on the device for a caller that
// places the blocks itself instead of having gather_segments_kernel pack them into one buffer
// per stream: the BGZF writer (bgzf.hip) and the many-stream wrapped calls (compress_streams.hip) move every block from its slot
// straight to its byte in the file or member.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/zng_rocm.h"
#include "deflate_rows_plan.h"      // BlkJob

namespace zr {

struct Workspace;

// The blocks of one round, still in their slots (scratch of the workspace: valid until the next call on the same HIP stream
// that uses the rows engine).  Block k belongs to stream blk[k].stream & 0x7fffffff, holds seg_len[k] bytes at blk[k].out and
// begins at byte in_stream[k] of its stream's deflate data; sizes[2 * s] is the whole length of stream s.  bm_base: the token-start
// bitmaps blk[k].bm_off counts from (what rows_block_points_kernel reads).
struct RowsBlocks {
    const BlkJob             *blk;
    const uint32_t           *seg_len;
    const unsigned long long *in_stream;
    const unsigned long long *sizes;
    size_t                    nblk;
    const unsigned long long *bm_base;
};

// One round through the engine, levels 1..9: the streams of `jobs` (in / in_len / dict_len / flags of each), every stream cut
// into segments of seg_bytes, all segments through ONE set of launches -- matcher, emitter, the scan that places the blocks.
// Asynchronous on `st`; the caller holds ws->mu.
enum RowsOut {
    kRowsOutHost,      // pack each stream into its job's out; {compressed size, does-not-fit flag} per stream to pinned host words
    kRowsOutDevice,    // the same, the words to d_sizes
    kRowsOutKeep       // no packing, nothing copied: the caller places the blocks itself; out and out_cap are not looked at
};
struct RowsRequest {
    int                        level;
    int                        strategy;        // 0..4, as zng_rocm_deflate_strategy_streams_dev
    int                        window_bits;     // the streams' w_bits, 9..15, already checked; below 15 the matcher runs its window form
    const zng_rocm_stream_job *jobs;
    size_t                     njobs;
    uint32_t                   seg_bytes;       // deflate_rows_segment_bytes() of the plaintext of the caller's WHOLE call, so that
                                                // the blocks of a job list do not depend on the caller or on its rounds
    const size_t              *one_cap;         // or null: the room of stream 0, a single stream of >= 4 GiB of room
    const zng_rocm_dict       *dict;            // or null: ONE shared preset dictionary (dict_dev.h) whose window is every stream's
                                                // history, through the dictionary form of the matcher -- strategies 0, 1 and 4,
                                                // window_bits 15, no job has a dict_len of its own.  The bytes are those of the
                                                // window copied in front of every plaintext with dict_len = W
    RowsOut                    out;
    unsigned long long        *d_sizes;         // kRowsOutDevice
};
struct RowsDone {
    unsigned long long *h_sizes;     // kRowsOutHost: valid once the stream has been synchronised
    RowsBlocks          blocks;      // every mode: the block table (the slots' bytes are the caller's to place only in kRowsOutKeep)
};
uint32_t deflate_rows_segment_bytes(size_t total_in);
int deflate_rows_enqueue(const RowsRequest &rq, Workspace *ws, hipStream_t st, RowsDone *done);

// zng_rocm_deflate_dev(level, ...) -- its checks, its texts, its bytes, its one synchronisation -- that also hands back, at levels
// 1..9, one row {byte of the block in the deflate data, plaintext offset of its first byte} per block (rows_block_points_kernel
// behind the engine's kernels, read back with the sizes: deflate_index_plan.h).  Level 0 leaves `rows` empty: its blocks are closed form.
int deflate_rows_points_dev(int level, const uint8_t *d_in, size_t in_len, uint8_t *d_out, size_t out_cap, size_t *out_len,
                            std::vector<uint64_t> &rows, hipStream_t st);

}  // namespace zr
