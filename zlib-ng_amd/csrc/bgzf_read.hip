// bgzf_read.hip -- random access into a BGZF file that sits in device memory (SAM specification 4.1; what bgzip, BAM and tabix
// cut into members of at most 64 KiB for): the members table without decoding, many plaintext ranges in one set of launches,
// and htslib's virtual offsets.  The host steps are bgzf_read_plan.h.
//
// zng_rocm_bgzf_index_dev
//   scan .. headers          gzip_members.hip's steps, unchanged (members_heads): every candidate, every header's verdict
//   bgzf_index_link_kernel   one lane per candidate: an accepted header with a 'BC' subfield gives {position, end = position +
//                            BSIZE + 1, header length, the CRC-32 and ISIZE words at end - 8, flags}; the flags say whether the
//                            end lies inside the file, whether header, two bytes of deflate and trailer fit, and whether 1f 8b
//                            stands at the end (what gz_look asks behind a member, gzread.c.in:122-140)
//   -> ONE readback of the table, 32 bytes per candidate; the host follows the chain from offset 0 by binary search
//   No inflate kernel runs: the rows are what the file claims.
//
// zng_rocm_bgzf_read_dev, per round of the plan
//   the slices go up; every member the round's ranges touch goes through the one-wavefront engine as a gzip member
//   (zng_rocm_uncompress_streams_dev, format 2: header, payload, CRC-32 and ISIZE verified on the device) -- an interior member
//   straight into its range's destination with exactly its row's out_len as capacity, an edge member into a 64 KiB slot
//   bgzf_slices_kernel       behind the engine on the same stream, one workgroup per slice: reads the engine's result row of
//                            the slice's member and moves the bytes (bgzf_copy.h) only if the member verified and is what its
//                            row says; a member that did not delivers no byte
//   -> ONE readback of the result rows, one synchronisation
#include "bgzf_copy.h"
#include "bgzf_read_plan.h"
#include "context.h"
#include "framing_parse.h"
#include "gzip_members_dev.h"
#include "gzip_members_plan.h"

#include <string.h>

#include <mutex>
#include <vector>

namespace zr {

struct IndexBytes {                                      // one lane reads the header it was given
    const uint8_t *src;
    __device__ uint32_t byte(uint64_t at) const { return src[at]; }
};

__global__ __launch_bounds__(256)
void bgzf_index_link_kernel(const uint8_t *__restrict__ src, uint64_t src_len, const uint64_t *__restrict__ pos,
                            const WrapperHead *__restrict__ heads, uint32_t n, BgzfIndexRow *__restrict__ rows) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const WrapperHead h = heads[i];
    const uint64_t p = pos[i];
    uint32_t bsize = 0;
    const bool bgzf = h.status == 0 && gzip_bgzf_bsize(IndexBytes{src + p}, src_len - p, &bsize);
    const uint64_t end = bgzf ? p + bsize + 1u : p;
    BgzfIndexRow r = {p, end, bgzf ? (uint32_t)h.header_len : 0u, 0u, 0u, bgzf_index_flags(bgzf, h.status == -5, p, end, h.header_len, src_len)};
    if (r.flags & kIdxTrailer) {                         // (end <= src_len and end - 8 >= p: inside the file)
        const uint8_t *t = src + end - 8;
        r.crc = wrapper_le32(t);
        r.isize = wrapper_le32(t + 4);
    }
    if ((r.flags & kIdxInside) && src_len - end >= 2 && src[end] == 0x1fu && src[end + 1] == 0x8bu) r.flags |= kIdxNextMagic;
    rows[i] = r;
}

struct BgzfSlice {
    const uint8_t *src;     // in the edge member's slot
    uint8_t       *dst;     // in the range's destination
    uint32_t len;
    uint32_t job;           // whose result row decides
    uint32_t want_used, want_out;       // the member's row: src_len, out_len
};

__global__ __launch_bounds__(256)
void bgzf_slices_kernel(const BgzfSlice *__restrict__ slices, uint32_t nslices, const uint32_t *__restrict__ results) {
    for (uint32_t w = blockIdx.x; w < nslices; w += gridDim.x) {
        const BgzfSlice s = slices[w];
        if (!bgzf_member_delivers(results + 4u * s.job, s.want_used, s.want_out)) continue;   // (the same answer in every lane)
        bgzf_copy(s.dst, 0, s.len, s.src, s.len, (int)threadIdx.x);
    }
}

namespace {

thread_local int t_read_decoded = 0, t_read_direct = 0, t_read_rounds = 0;

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

const char *index_why(uint32_t why) {
    switch (why) {
    case kIdxWhyNoHeader: return "no accepted BGZF header begins here";
    case kIdxWhyNoRoom: return "BSIZE leaves no room for header, deflate data and trailer";
    case kIdxWhyIsize: return "ISIZE is above 65536";
    case kIdxWhyCutHeader: return "the file ends inside the header";
    case kIdxWhyCutMember: return "the member's BSIZE end lies behind the end of the file";
    default: return "";
    }
}

const char *rows_why(uint32_t why) {
    switch (why) {
    case kRowsOrder: return "src_off is not ascending, or members overlap";
    case kRowsOutside: return "the member lies outside src_len";
    case kRowsDstOff: return "dst_off is not contiguous from 0";
    case kRowsNotBgzf: return "bgzf is not 1";
    case kRowsSrcLen: return "src_len is outside 28 .. 65536";
    case kRowsOutLen: return "out_len is above 65536";
    default: return "";
    }
}

}  // namespace

}  // namespace zr

using namespace zr;

extern "C" {

int zng_rocm_bgzf_read_last_decoded(void) { return t_read_decoded; }
int zng_rocm_bgzf_read_last_direct(void) { return t_read_direct; }
int zng_rocm_bgzf_read_last_rounds(void) { return t_read_rounds; }

int zng_rocm_bgzf_voffset(const zng_rocm_gzip_member *members, size_t nmembers, uint64_t uoff, uint64_t *voff) {
    if ((!members && nmembers) || !voff) return ZNG_ROCM_EINVAL;
    return bgzf_voffset(members, nmembers, uoff, voff) ? ZNG_ROCM_OK : ZNG_ROCM_EINVAL;
}

int zng_rocm_bgzf_uoffset(const zng_rocm_gzip_member *members, size_t nmembers, uint64_t voff, uint64_t *uoff) {
    if ((!members && nmembers) || !uoff) return ZNG_ROCM_EINVAL;
    return bgzf_uoffset(members, nmembers, voff, uoff) ? ZNG_ROCM_OK : ZNG_ROCM_EINVAL;
}

int zng_rocm_bgzf_index_dev(const uint8_t *d_src, size_t src_len, zng_rocm_gzip_member *members, size_t members_cap, size_t *nmembers,
                            uint64_t *plain_len, size_t *in_used, void *stream) {
    if (nmembers) *nmembers = 0;
    if (plain_len) *plain_len = 0;
    if (in_used) *in_used = 0;
    if ((!d_src && src_len) || (!members && members_cap) || !nmembers || !plain_len || !in_used) {
        set_error("zng_rocm_bgzf_index_dev: a null buffer with a length, or a null result pointer");
        return ZNG_ROCM_EINVAL;
    }
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    if (!src_len) return ZNG_ROCM_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard dev;
    Workspace *ws = workspace_for(st);
    if (!ws) return ZNG_ROCM_ENOMEM;
    MembersHeads m;
    if (int rc = members_heads("zng_rocm_bgzf_index_dev", d_src, src_len, sizeof(BgzfIndexRow), st, ws, &m)) return rc;
    if (m.too_many) {
        set_error("zng_rocm_bgzf_index_dev: more than %u candidates; zng_rocm_gunzip_members_dev reads such a file", kMembersMaxCandidates);
        return ZNG_ROCM_EINVAL;
    }
    const BgzfIndexRow *rows = nullptr;
    if (m.n) {
        BgzfIndexRow *d_rows = reinterpret_cast<BgzfIndexRow *>(m.d_rows);
        hipLaunchKernelGGL(bgzf_index_link_kernel, dim3((m.n + 255u) / 256u), dim3(256), 0, st, d_src, (uint64_t)src_len, m.d_pos, m.d_heads,
                           m.n, d_rows);
        ZR_HIP(hipGetLastError());
        ZR_HIP(hipMemcpyAsync(m.h_rows, d_rows, (size_t)m.n * sizeof(BgzfIndexRow), hipMemcpyDeviceToHost, st));
        ZR_HIP(hipStreamSynchronize(st));
        rows = reinterpret_cast<const BgzfIndexRow *>(m.h_rows);
    }
    const BgzfIndexWalk w = bgzf_index_walk(rows, m.n, src_len, kMembersHeaderLook, members, members_cap);
    *nmembers = w.nmembers;
    *plain_len = w.plain_len;
    *in_used = (size_t)w.at;
    if (w.status) set_error("zng_rocm_bgzf_index_dev: offset %llu: %s", (unsigned long long)w.at, index_why(w.why));
    return w.status;
}

int zng_rocm_bgzf_read_dev(const uint8_t *d_src, size_t src_len, const zng_rocm_gzip_member *members, size_t nmembers,
                           zng_rocm_bgzf_range *ranges, size_t nranges, size_t scratch_bytes, void *stream) {
    t_read_decoded = t_read_direct = t_read_rounds = 0;
    const uint64_t slots = bgzf_read_slots(scratch_bytes);
    if ((!d_src && src_len) || (!members && nmembers) || (!ranges && nranges) || !slots || nranges > 0xfffffffeull) {
        set_error("zng_rocm_bgzf_read_dev: a null buffer with a length, more than 2^32 - 2 ranges, or scratch_bytes outside 128 KiB .. 4 GiB");
        return ZNG_ROCM_EINVAL;
    }
    size_t bad = 0;
    if (const uint32_t why = bgzf_read_rows_check(members, nmembers, src_len, &bad)) {
        set_error("zng_rocm_bgzf_read_dev: members[%zu]: %s", bad, rows_why(why));
        return ZNG_ROCM_EINVAL;
    }
    for (size_t r = 0; r < nranges; ++r)
        if (!ranges[r].d_dst && ranges[r].len) {
            set_error("zng_rocm_bgzf_read_dev: ranges[%zu]: a null d_dst with a length", r);
            return ZNG_ROCM_EINVAL;
        }
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    std::vector<BgzfRangeIn> in(nranges);
    for (size_t r = 0; r < nranges; ++r) in[r] = BgzfRangeIn{ranges[r].uoff, ranges[r].len};
    BgzfReadPlan plan;
    bgzf_read_plan(members, nmembers, in.data(), nranges, slots, kBgzfReadRoundJobs, plan);
    // a range no round holds (empty, beyond the end) is complete as it stands; the others are written behind their round
    auto finish = [&](size_t r, const BgzfRangeOut &o) {
        ranges[r].status = o.status;
        ranges[r].out_len = o.out_len;
        ranges[r].msg = o.status != -3 ? nullptr : o.msg == kBgzfMsgRow ? "index row does not match the file" : zng_rocm_inflate_message(o.msg);
    };
    if (plan.rounds.empty()) {
        for (size_t r = 0; r < nranges; ++r) finish(r, BgzfRangeOut{1, plan.clipped[r], 0u, false});
        return ZNG_ROCM_OK;
    }
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard dev;
    Workspace *ws = workspace_for(st);
    if (!ws) return ZNG_ROCM_ENOMEM;

    // device: results | slices | slots, sized for the largest round (every part 16-byte aligned); pinned: slices | results
    size_t max_jobs = 0, max_slices = 0, max_slots = 0;
    for (const BgzfReadRound &rd : plan.rounds) {
        if (rd.job_end - rd.job_begin > max_jobs) max_jobs = rd.job_end - rd.job_begin;
        if (rd.slices > max_slices) max_slices = rd.slices;
        if (rd.slots > max_slots) max_slots = rd.slots;
    }
    const size_t o_slices = up16(max_jobs * 4 * sizeof(uint32_t)), o_slots = o_slices + up16(max_slices * sizeof(BgzfSlice));
    const size_t oh_res = up16(max_slices * sizeof(BgzfSlice));
    uint8_t *d = nullptr, *h = nullptr;
    {
        std::lock_guard<std::mutex> use(ws->mu);
        if (int rc = scratch_reserve(ws, kScrBgzfRead, o_slots + max_slots * kBgzfReadSlot, false, (void **)&d)) return rc;
        if (int rc = host_tables_acquire(ws)) return rc;
        if (int rc = scratch_reserve(ws, kScrBgzfReadHost, oh_res + max_jobs * 4 * sizeof(uint32_t), true, (void **)&h)) return rc;
    }
    uint32_t *d_res = reinterpret_cast<uint32_t *>(d);
    BgzfSlice *d_slices = reinterpret_cast<BgzfSlice *>(d + o_slices), *h_slices = reinterpret_cast<BgzfSlice *>(h);
    uint8_t *d_slots = d + o_slots;
    const uint32_t *h_res = reinterpret_cast<const uint32_t *>(h + oh_res);

    std::vector<zng_rocm_inflate_dev_job> jobs;
    std::vector<BgzfJobVerdict> verdicts(plan.jobs.size(), BgzfJobVerdict{1, 0u});
    size_t next_range = 0;
    for (const BgzfReadRound &rd : plan.rounds) {
        const size_t nj = rd.job_end - rd.job_begin;
        jobs.resize(nj);
        for (size_t k = 0; k < nj; ++k) {
            const BgzfReadJob &j = plan.jobs[rd.job_begin + k];
            const zng_rocm_gzip_member &row = members[j.member];
            const bool direct = j.slot == kBgzfReadDirect;
            jobs[k] = zng_rocm_inflate_dev_job{d_src + row.src_off, direct ? ranges[j.range].d_dst + j.at : d_slots + j.slot * kBgzfReadSlot,
                                               row.src_len, direct ? row.out_len : kBgzfReadSlot, 0u, 0u};
        }
        if (rd.slices) {
            std::lock_guard<std::mutex> use(ws->mu);
            if (int rc = host_tables_acquire(ws)) return rc;
            size_t s = 0;
            for (size_t k = rd.part_begin; k < rd.part_end; ++k) {
                const BgzfReadPart &p = plan.parts[k];
                if (!p.slice) continue;
                const BgzfReadJob &j = plan.jobs[p.job];
                const zng_rocm_gzip_member &row = members[j.member];
                h_slices[s++] = BgzfSlice{d_slots + j.slot * kBgzfReadSlot + p.off, ranges[p.range].d_dst + p.at, p.len,
                                          (uint32_t)(p.job - rd.job_begin), (uint32_t)row.src_len, (uint32_t)row.out_len};
            }
            ZR_HIP(hipMemcpyAsync(d_slices, h_slices, rd.slices * sizeof(BgzfSlice), hipMemcpyHostToDevice, st));
            if (int rc = host_tables_release(ws, st)) return rc;
        }
        if (int rc = zng_rocm_uncompress_streams_dev(2, jobs.data(), nj, d_res, st)) return rc;
        if (rd.slices) {
            const uint32_t grid = rd.slices < (1u << 20) ? rd.slices : (1u << 20);
            hipLaunchKernelGGL(bgzf_slices_kernel, dim3(grid), dim3(256), 0, st, d_slices, rd.slices, d_res);
            ZR_HIP(hipGetLastError());
        }
        ZR_HIP(hipMemcpyAsync((void *)h_res, d_res, nj * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        ZR_HIP(hipStreamSynchronize(st));
        ++t_read_rounds;
        for (size_t k = 0; k < nj; ++k) verdicts[rd.job_begin + k] = bgzf_job_verdict(h_res + 4 * k, members[plan.jobs[rd.job_begin + k].member]);
        // the ranges of this round, and the empty ones in front of it, in order; a range's parts stand together
        size_t k = rd.part_begin;
        for (; next_range < rd.range_end; ++next_range) {
            const size_t from = k;
            while (k < rd.part_end && plan.parts[k].range == next_range) ++k;
            finish(next_range, bgzf_range_result(plan.parts.data() + from, k - from, verdicts.data(), plan.clipped[next_range]));
        }
    }
    for (; next_range < nranges; ++next_range) finish(next_range, BgzfRangeOut{1, plan.clipped[next_range], 0u, false});
    t_read_decoded = (int)plan.decoded;
    t_read_direct = (int)plan.direct;
    return ZNG_ROCM_OK;
}

}  // extern "C"
