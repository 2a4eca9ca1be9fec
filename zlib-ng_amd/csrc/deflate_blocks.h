// deflate_blocks.h -- what the rows engine (deflate_dyn.hip: lz_rows_kernel, emit_dynamic_kernel, segments_scan_kernel) leaves
// on the device for a caller that places the blocks itself instead of having gather_segments_kernel pack them into one buffer
// per stream: the BGZF writer (bgzf.hip) and the many-stream wrapped calls (compress_streams.hip) move every block from its slot
// straight to its byte in the file or member.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/zng_rocm.h"

namespace zr {

struct Workspace;

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

// The blocks of one round, still in their slots (scratch of the workspace: valid until the next call on the same HIP stream
// that uses the rows engine).  Block k belongs to stream blk[k].stream & 0x7fffffff, holds seg_len[k] bytes at blk[k].out and
// begins at byte in_stream[k] of its stream's deflate data; sizes[2 * s] is the whole length of stream s.
struct RowsBlocks {
    const BlkJob             *blk;
    const uint32_t           *seg_len;
    const unsigned long long *in_stream;
    const unsigned long long *sizes;
    size_t                    nblk;
};

// Levels 1..9 over `njobs` independent streams (in / in_len / dict_len / flags of each job; out and out_cap are not looked at),
// every stream short enough for one segment: matcher, emitter and the scan, no packing, nothing copied to the host.
// Asynchronous on `st`; the caller holds ws->mu.
int deflate_rows_enqueue_blocks(int level, const zng_rocm_stream_job *sjobs, size_t njobs, Workspace *ws, hipStream_t st,
                                RowsBlocks *blocks);

// The same for streams of any length and any strategy (0..4, as zng_rocm_deflate_strategy_streams_dev): every stream is cut into
// segments of seg_bytes, and the blocks of all segments of a stream follow one another in the table, in_stream[] counting on
// through the stream.  seg_bytes is what deflate_rows_segment_bytes() gives for the plaintext of the caller's WHOLE call, so that
// the blocks are those zng_rocm_deflate_strategy_streams_dev writes for the same job list (compress_streams.hip).
// window_bits: the streams' w_bits, 9..15 (deflate_window_plan.h); below 15 the matcher runs its window form.
uint32_t deflate_rows_segment_bytes(size_t total_in);
int deflate_rows_enqueue_streams(int level, int strategy, const zng_rocm_stream_job *sjobs, size_t njobs, uint32_t seg_bytes,
                                 Workspace *ws, hipStream_t st, RowsBlocks *blocks, int window_bits = 15);
// The same behind ONE shared preset dictionary (dict_dev.h): every stream's history is the object's window, through the
// dictionary form of the matcher -- strategies 0, 1 and 4; no job has a dict_len of its own.  The bytes are those of the call
// above over the window copied in front of every plaintext with dict_len = W.
int deflate_rows_enqueue_streams_dict(int level, int strategy, const zng_rocm_dict *dict, const zng_rocm_stream_job *sjobs,
                                      size_t njobs, uint32_t seg_bytes, Workspace *ws, hipStream_t st, RowsBlocks *blocks);

}  // namespace zr
