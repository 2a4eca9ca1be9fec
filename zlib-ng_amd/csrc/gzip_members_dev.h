// gzip_members_dev.h -- what gzip_members.hip shares with bgzf_read.hip: the first steps of discovery (scan, offsets, the
// candidates' number brought down, scatter, the header kernel on every candidate), which leave the sorted candidate positions
// and the header verdicts in device memory together with room for one row per candidate.  Each caller runs a link kernel of
// its own over them and reads its rows back once.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "context.h"
#include "framing_parse.h"

namespace zr {

struct MembersHeads {
    uint32_t n;                   // candidates; 0 when there are none, or too many for a table
    bool too_many;                // more than kMembersMaxCandidates
    const uint64_t *d_pos;        // n positions in file order
    const WrapperHead *d_heads;   // n verdicts of the header kernel (format 2, at most kMembersHeaderLook bytes shown)
    uint8_t *d_rows, *h_rows;     // device / pinned host: n rows of row_bytes each, for the caller's link kernel and readback
};

// Synchronises `st` once (four bytes: the candidates' number sizes the tables and the header kernel's grid).  `who` names the
// entry point in an error text.
int members_heads(const char *who, const uint8_t *d_src, size_t src_len, size_t row_bytes, hipStream_t st, Workspace *ws,
                  MembersHeads *out);

}  // namespace zr
