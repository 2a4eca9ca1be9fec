// dict_dev.h -- the shared preset dictionary object (zng_rocm_dict, dict.hip) as the engines see it: its window, the primed
// head table of the level-1 class and the primed row tables of the rows engine in device memory, and the launchers of the
// dictionary form of the level-1 class (deflate_stream.hip) and of the row tables' kernel (deflate_dyn.hip).
#pragma once
#include "context.h"
#include "dict_plan.h"

struct zng_rocm_dict {
    uint64_t  generation;     // of the context it was made under: a zng_rocm_shutdown() retires the object
    int       device;
    uint32_t  id;             // Adler-32 of every byte of the dictionary: the DICTID
    uint32_t  window;         // W = dict_window(dict_len)
    uint32_t *d_head;         // kDictHeadSlots words: dict_head_table of the window (one allocation with d_window)
    uint8_t  *d_window;       // W bytes + kDictPad zero bytes, 16-byte aligned
    uint8_t  *d_rows;         // kDictRowsBytes: the rows engine's pos | tag | cnt behind the positions [0, dict_rows_primed(W))
};

namespace zr {

// 0, or ZNG_ROCM_ENODEV (error text set) when no context is live or the object was made under an earlier one
int dict_usable(const zng_rocm_dict *d);

// deflate_quick_kernel's dictionary form over a HOST job table (dict_len 0; out 4-byte aligned, out_cap >=
// zng_rocm_deflate_quick_bound(in_len)); d_results: 2 words per job {compressed length, Adler-32 of the plaintext}
int launch_deflate_quick_dict(const zng_rocm_stream_job *jobs, size_t njobs, uint32_t *d_results, const zng_rocm_dict *dict,
                              hipStream_t stream);

// the rows engine's primed tables of a window (deflate_dyn.hip: rows_dict_table_kernel, one workgroup) into d_tab,
// kDictRowsBytes of 16-byte aligned device memory; asynchronous on `stream`
int launch_rows_dict_table(const uint8_t *d_window, uint32_t W, void *d_tab, hipStream_t stream);

}  // namespace zr
