// framing_large.h -- what framing_large.hip shares with gzip_members.hip: the header kernels of the wrapped large calls
// (one wavefront per member runs wrapper_parse_rules, the FHCRC through the many-message checksum pass) over a table of
// members that ALREADY sits in device memory, so that a caller whose members were found on the device runs the same
// kernels without bringing the table down first.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "framing_parse.h"

namespace zr {

struct HeadJob {
    const uint8_t *src;
    uint64_t len;
};

// device bytes header_rows_device needs at `d_work` (16-byte aligned) for n members
size_t header_rows_scratch(size_t n);
// d_rows[i] = the verdict on the header of d_jobs[i] (format 1 zlib, 2 gzip with the FHCRC compared); asynchronous on `st`
int header_rows_device(int format, const HeadJob *d_jobs, size_t n, WrapperHead *d_rows, uint8_t *d_work, hipStream_t st);

}  // namespace zr
