// inflate_dev.h -- what the inflate translation units share: the device job descriptor and the message ids of d_results
// (inflate_dev_types.h; texts: zng_rocm_inflate_message), the launchers for job tables that already sit in device memory,
// and every other internal function that one of them defines and another calls.
#pragma once
#include "context.h"
#include "inflate_dev_types.h"

#include <utility>
#include <vector>

namespace zr {

// one wavefront per job; d_jobs and d_results are device memory (results: 4 words per job)
int launch_inflate_streams_device(const InflateJobDev *d_jobs, size_t njobs, uint32_t *d_results, hipStream_t stream);
// the same with every job's dict_len bytes of history taken from ONE shared window: the bytes in front of d_hist_end
// (zng_rocm_uncompress_streams_dict_dev: a job decodes with the whole window or, dict_len 0, with none)
int launch_inflate_streams_dict_device(const InflateJobDev *d_jobs, size_t njobs, uint32_t *d_results, const uint8_t *d_hist_end,
                                       hipStream_t stream);
// the same with every job's dict_len bytes of history taken from ITS OWN window, the bytes in front of d_spans[job].hist_end,
// the decode starting d_spans[job].start_bit bits into the job's first byte, and status 1 where the output reaches out_cap
// (zng_rocm_inflate_index_read_dev: a job is one span of an indexed stream)
int launch_inflate_streams_span_device(const InflateJobDev *d_jobs, size_t njobs, uint32_t *d_results, const InflateSpanDev *d_spans,
                                       hipStream_t stream);

// the parts of ONE large stream, 16-bit symbols out (inflate_large.hip); results: 8 words per part; d_marks (or null):
// (or of several streams, each stream's starts together and in order: then every job carries in `flags` the index one past
// its own stream's last start -- 0 means njobs -- and a part ends only on a start in front of that)
// 4 words per part, where its last block inside the input ended
// d_side (or null): starts inside blocks -- d_starts then holds njobs keys behind the njobs bits (0 a block start, 1 inside a
// fixed-code block, H + 2 inside the dynamic block at H), and d_side takes 8 words per part (inflate_streams_kernel<..., SUB>)
int launch_inflate_parts_device(const InflateJobDev *d_jobs, size_t njobs, uint32_t *d_results, const unsigned long long *d_starts,
                                bool many, hipStream_t stream, uint32_t *d_marks = nullptr, uint32_t *d_side = nullptr);

// the counting forms (inflate_large_size.hip): the parts of large streams, one wavefront each, no output -- d_jobs as above
// (out / out_cap not looked at), 8 result words per part; and whole streams, one wavefront each, 8 words per stream
// (inflate_large_size_plan.h: ls_part_count, ls_stream_row)
int launch_inflate_size_parts_device(const InflateJobDev *d_jobs, size_t njobs, const unsigned long long *d_starts, uint32_t *d_results,
                                     hipStream_t stream);
int launch_inflate_size_streams_device(const InflateJobDev *d_jobs, size_t njobs, uint32_t *d_results, hipStream_t stream);

// the sync kernel over a table of regions (SubRegionDev: inflate_dev_types.h)
int launch_subblock_sync(const uint8_t *d_src, size_t src_len, const SubRegionDev *d_regions, size_t nregions,
                         unsigned long long *d_bit, unsigned long long *d_key, hipStream_t stream);

// ---- inflate_resolve.hip ------------------------------------------------------------------------------------------------
// a stream of a batch laid out in symbol space (inflate_resolve_batch, inflate_resolve_symbols_batch: d_streams)
struct BatchStream {
    uint64_t       v_start;     // symbol index of the stream's first byte
    const uint8_t *d_window;    // its window_len bytes of history (device) or null
    uint64_t       window_len;
};
// symbols that are already in place (inflate_large.hip) -> bytes: the windows in front, the context chain, the translation;
// the layout of inflate_resolve_batch (context.h) without K1
int inflate_resolve_symbols_batch(const uint64_t *d_segs, size_t nsegs, uint16_t *sym, const uint64_t *d_seg_dst,
                                  const uint64_t *d_seg_end, const BatchStream *d_streams, size_t nstreams, hipStream_t st);
// the sequential decoder on the calling thread + the device resolve: what every irregular stream ends up in; *msg (when
// given) = the decoder's message of a data error (static storage), else null
int inflate_raw_window_sequential(const uint8_t *src, size_t src_len, const uint8_t *d_window, uint32_t window_len, uint8_t *d_dst,
                                  size_t dst_cap, uint64_t *out_len, size_t *in_used, hipStream_t st);
int inflate_raw_window_sequential_msg(const uint8_t *src, size_t src_len, const uint8_t *d_window, uint32_t window_len,
                                      uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, size_t *in_used, const char **msg,
                                      hipStream_t st);

// ---- inflate_large.hip (return conventions: see there) ------------------------------------------------------------------
int inflate_large_from_host(const uint8_t *src, size_t src_len, const uint8_t *d_window, uint32_t window_len, uint8_t *d_dst,
                            size_t dst_cap, uint64_t *out_len, size_t *in_used, hipStream_t st);
int inflate_large_device_only(const uint8_t *d_src, size_t src_len, const uint8_t *d_window, uint32_t window_len, uint8_t *d_dst,
                              size_t dst_cap, uint64_t *out_len, size_t *in_used, hipStream_t st);
int inflate_large_blocks_device_only(const uint8_t *d_src, size_t src_len, unsigned start_bit, const uint8_t *d_window,
                                     uint32_t window_len, uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, uint64_t *end_bit,
                                     int *final, hipStream_t st);
// the plaintext sizes of raw streams by the counting pass (zng_rocm_uncompress_large_size_dev / _sizes_dev, framing_large.hip)
int inflate_large_sizes_raw(zng_rocm_inflate_large_job *jobs, size_t njobs, size_t round_bytes, bool single, hipStream_t st);
// The block starts a pieces call meets, for zng_rocm_inflate_index_build_dev (inflate_index.hip): while the calling thread has
// a sink set, inflate_pieces_call appends {bit of its d_src, offset in its output} of every genuine part that begins at a
// block start and of every block start it establishes between pieces, and framing_large.hip notes the wrapper header's
// length.  Null outside a build call: no other caller sees a difference.
struct IndexSink {
    std::vector<std::pair<uint64_t, uint64_t>> cands;
    uint64_t header_len = 0;
};
IndexSink *inflate_index_sink();
void inflate_index_sink_set(IndexSink *sink);
// inflate_index.hip: the index of a stream whose block starts are known -- to the build above from its decode, to
// zng_rocm_compress2_index_dev (oneshot.hip) from the compressor.  cands: {bit of the file, plaintext offset} in stream order
// (inflate_index_plan.h: index_select thins them to head.span_bytes); d_plain: the plaintext the windows are gathered from.
// `who` names the call in the error text.  Returns 0 with *out set, or an error with *out untouched.
struct IndexHead;
struct IndexCand;
int inflate_index_from_cands(const char *who, const IndexHead &head, const IndexCand *cands, size_t ncands, const uint8_t *d_plain,
                             hipStream_t st, zng_rocm_inflate_index **out);
void inflate_large_forget_parts();       // the part counters of the calling thread back to 0 ("the sequential decoder did it")
void inflate_large_reset_counters();     // all of the calling thread's last_* counters: nothing ran

}  // namespace zr
