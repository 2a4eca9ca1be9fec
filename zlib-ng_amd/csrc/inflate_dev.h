// inflate_dev.h -- what inflate_dev.hip shares with framing_dev.hip: the device job descriptor, the message ids of
// d_results (texts: zng_rocm_inflate_message) and the launcher for a job table that already sits in device memory.
#pragma once
#include "context.h"
#include "inflate_dev_types.h"

namespace zr {

struct InflateJobDev {
    const uint8_t *in;
    uint8_t       *out;
    uint64_t       in_len;
    uint64_t       out_cap;
    uint32_t       dict_len;
    uint32_t       flags;
};

// one wavefront per job; d_jobs and d_results are device memory (results: 4 words per job)
int launch_inflate_streams_device(const InflateJobDev *d_jobs, size_t njobs, uint32_t *d_results, hipStream_t stream);
// the same with every job's dict_len bytes of history taken from ONE shared window: the bytes in front of d_hist_end
// (zng_rocm_uncompress_streams_dict_dev: a job decodes with the whole window or, dict_len 0, with none)
int launch_inflate_streams_dict_device(const InflateJobDev *d_jobs, size_t njobs, uint32_t *d_results, const uint8_t *d_hist_end,
                                       hipStream_t stream);

// the parts of ONE large stream, 16-bit symbols out (inflate_large.hip); results: 8 words per part; d_marks (or null):
// (or of several streams, each stream's starts together and in order: then every job carries in `flags` the index one past
// its own stream's last start -- 0 means njobs -- and a part ends only on a start in front of that)
// 4 words per part, where its last block inside the input ended
// d_side (or null): starts inside blocks -- d_starts then holds njobs keys behind the njobs bits (0 a block start, 1 inside a
// fixed-code block, H + 2 inside the dynamic block at H), and d_side takes 8 words per part (inflate_streams_kernel<..., SUB>)
int launch_inflate_parts_device(const InflateJobDev *d_jobs, size_t njobs, uint32_t *d_results, const unsigned long long *d_starts,
                                bool many, hipStream_t stream, uint32_t *d_marks = nullptr, uint32_t *d_side = nullptr);

// the sync kernel over a table of regions (SubRegionDev: inflate_dev_types.h)
int launch_subblock_sync(const uint8_t *d_src, size_t src_len, const SubRegionDev *d_regions, size_t nregions,
                         unsigned long long *d_bit, unsigned long long *d_key, hipStream_t stream);

}  // namespace zr
