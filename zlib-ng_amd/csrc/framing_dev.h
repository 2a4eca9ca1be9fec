// framing_dev.h -- the uncompress pipeline of framing_dev.hip over tables that already sit in device memory, for the calls that
// fill such a table on the device themselves (inflate_sizes.hip).  Everything is enqueued on `stream`; nothing synchronises.
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

}  // namespace zr
