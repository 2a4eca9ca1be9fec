// framing_dev.h -- the uncompress pipeline of framing_dev.hip over tables that already sit in device memory, for the calls that
// fill such a table on the device themselves (inflate_sizes.hip), and the upload of the caller's jobs in front of it.
// Everything is enqueued on `stream`; nothing synchronises.
#pragma once
#include "checksum_args.h"
#include "context.h"
#include "dict_dev.h"
#include "inflate_dev.h"

namespace zr {

// parse_header_kernel: the header of every member of d_given judged (dict: by dict_parse_header), d_patched = the table of the
// payloads (in / in_len behind the header, dict_len = the history the verdict gives, an empty job for a refused header), d_head
// = 2 words per job {header bytes, verdict}
int launch_parse_header(int format, const zng_rocm_dict *dict, const InflateJobDev *d_given, size_t njobs, InflateJobDev *d_patched,
                        uint32_t *d_head, hipStream_t stream);
// the engine over d_patched (its dictionary form when dict is given), the check values of the outputs (format 1, 2) and
// verify_trailer_kernel: d_results = the verified rows of the members of d_given.  d_checks: 2 words per job; d_msg: njobs *
// (sizeof(StreamArgs) + sizeof(FinalArgs)) bytes; d_part: njobs Partial
int uncompress_patched_device(int format, const zng_rocm_dict *dict, const InflateJobDev *d_given, const InflateJobDev *d_patched,
                              const uint32_t *d_head, uint32_t *d_checks, uint8_t *d_msg, Partial *d_part, size_t njobs,
                              uint32_t *d_results, hipStream_t stream);

// The front of every uncompress and sizing call: the caller's jobs as a device table, and their headers parsed.  Reserves the
// scratch of the pipeline above (the given and the patched table, the head rows and, with `checks`, the check values' words,
// messages and partials), fills the pinned host table, copies it up and runs launch_parse_header.  with_out: the jobs carry
// out / out_cap and take neither dict_len nor flags -- a job that breaks this is refused here, ZNG_ROCM_EINVAL; else they carry
// dict_len, have no output yet, and the caller has checked them.  The caller holds ws->mu.
struct GivenJobs {
    InflateJobDev *d_given, *d_patched;
    uint32_t *d_head, *d_checks;            // d_checks, d_msg, d_part: null without `checks`
    uint8_t *d_msg;
    Partial *d_part;
};
int upload_given_jobs(Workspace *ws, int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                      bool with_out, bool checks, GivenJobs *g, hipStream_t stream);

}  // namespace zr
