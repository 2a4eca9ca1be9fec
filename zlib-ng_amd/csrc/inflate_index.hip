// inflate_index.hip -- random access into ONE plain deflate, zlib or gzip stream that sits in device memory: what zran.c and
// indexed_gzip do on a CPU.  The host steps are inflate_index_plan.h.
//
// zng_rocm_inflate_index_build_dev
//   zng_rocm_uncompress_large_dev, unchanged, with the calling thread's sink set (inflate_dev.h): the pieces loop leaves the
//   block starts it met -- every genuine part of every pass that begins at a block start, every block start it establishes
//   between pieces, the block ends of host-decoded stretches included -- as {bit, output offset}
//   index_select             the candidates at least span_bytes apart become the access points
//   index_windows_kernel     one workgroup per point moves the min(32768, out_off) bytes in front of it out of d_dst into
//                            memory the index owns (bgzf_copy.h: d_dst has whatever alignment the caller gave it)
//   (the last two steps are inflate_index_from_cands, which zng_rocm_compress2_index_dev -- oneshot.hip -- shares: its
//   candidates come from the compressor's block table and its windows from the plaintext it compressed, nothing is decoded)
//
// zng_rocm_inflate_index_read_dev, per round of the plan
//   jobs, span table and slices go up in one copy
//   inflate_streams_span_kernel<4096>   one wavefront per span (inflate_dev.hip): from the point's bit, with the point's
//                            window as history, until out_cap bytes are there -- an interior span straight into its range's
//                            destination, an edge span into its slot, only as far as the round's ranges need it
//   index_slices_kernel      behind it on the same stream, one workgroup per slice: moves the bytes only if the slice's job
//                            ended with status 1 and produced exactly its out_cap
//   -> ONE readback of the result rows, one synchronisation
#include "bgzf_copy.h"
#include "context.h"
#include "inflate_dev.h"
#include "inflate_index_plan.h"

#include <string.h>

#include <mutex>
#include <new>
#include <vector>

struct zng_rocm_inflate_index {
    zr::IndexHead head;
    std::vector<zng_rocm_access_point> pts;
    std::vector<uint64_t> woff;           // where point k's window begins in d_windows; woff[n] = their bytes
    uint8_t *d_windows = nullptr;         // owned
};

namespace zr {

struct IndexMove {          // of index_windows_kernel and index_slices_kernel
    const uint8_t *src;
    uint8_t       *dst;
    uint32_t len;
    uint32_t job;           // slices: whose result row decides, and what it must have produced
    uint32_t want_out, pad;
};

__global__ __launch_bounds__(256)
void index_windows_kernel(const IndexMove *__restrict__ moves, uint32_t n) {
    for (uint32_t w = blockIdx.x; w < n; w += gridDim.x) {
        const IndexMove m = moves[w];
        bgzf_copy(m.dst, 0, m.len, m.src, m.len, (int)threadIdx.x);
    }
}

// (a slice is as long as its span at most: below 2 GiB, what the mover's 32-bit count takes)
__global__ __launch_bounds__(256)
void index_slices_kernel(const IndexMove *__restrict__ slices, uint32_t nslices, const uint32_t *__restrict__ results) {
    for (uint32_t w = blockIdx.x; w < nslices; w += gridDim.x) {
        const IndexMove s = slices[w];
        if (!index_job_delivers(results + 4u * s.job, s.want_out)) continue;                 // (the same answer in every lane)
        bgzf_copy(s.dst, 0, s.len, s.src, s.len, (int)threadIdx.x);
    }
}

namespace {

thread_local int t_idx_decoded = 0, t_idx_direct = 0, t_idx_rounds = 0;

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// the index object around points that are already checked; the windows' memory is allocated here and filled by the caller
int index_new(const IndexHead &head, std::vector<zng_rocm_access_point> &pts, zng_rocm_inflate_index **out) {
    zng_rocm_inflate_index *idx = new (std::nothrow) zng_rocm_inflate_index;
    if (!idx) return ZNG_ROCM_ENOMEM;
    idx->head = head;
    idx->pts.swap(pts);
    index_window_offsets(idx->pts.data(), idx->pts.size(), idx->woff);
    if (idx->woff.back() && hipMalloc((void **)&idx->d_windows, (size_t)idx->woff.back()) != hipSuccess) {
        set_error("inflate index: no device memory for %llu bytes of windows", (unsigned long long)idx->woff.back());
        delete idx;
        return ZNG_ROCM_ENOMEM;
    }
    *out = idx;
    return ZNG_ROCM_OK;
}

const char *range_msg(const IndexRangeOut &o) {
    if (o.status == 1) return nullptr;
    if (o.msg == kIndexMsgTooLong) return "span too long for the one-wavefront engine";
    if (o.status != -3) return nullptr;
    return o.msg == kIndexMsgMismatch ? "index does not match the stream" : zng_rocm_inflate_message(o.msg);
}

}  // namespace

// inflate_dev.h: candidates -> points (index_select) -> the index object -> its windows, gathered by index_windows_kernel from the
// plaintext at d_plain (bgzf_copy.h: whatever alignment the caller gave it).  Synchronises `st` when there is a window to gather.
int inflate_index_from_cands(const char *who, const IndexHead &head, const IndexCand *cands, size_t ncands, const uint8_t *d_plain,
                             hipStream_t st, zng_rocm_inflate_index **out) {
    std::vector<zng_rocm_access_point> pts;
    index_select(cands, ncands, head.span_bytes, head.plain_len, head.header_len, pts);
    DeviceGuard dev;
    zng_rocm_inflate_index *idx = nullptr;
    if (int e = index_new(head, pts, &idx)) return e;
    const size_t n = idx->pts.size();
    if (n > 1) {
        Workspace *ws = workspace_for(st);
        int e = ws ? ZNG_ROCM_OK : ZNG_ROCM_ENOMEM;
        IndexMove *d_moves = nullptr, *h_moves = nullptr;
        if (!e) {
            std::lock_guard<std::mutex> use(ws->mu);
            e = scratch_reserve(ws, kScrIndexRead, n * sizeof(IndexMove), false, (void **)&d_moves);
            if (!e) e = host_tables_acquire(ws);
            if (!e) e = scratch_reserve(ws, kScrIndexReadHost, n * sizeof(IndexMove), true, (void **)&h_moves);
            if (!e) {
                for (size_t k = 0; k < n; ++k) {
                    const zng_rocm_access_point &p = idx->pts[k];
                    h_moves[k] = IndexMove{d_plain + (p.out_off - p.window_len), idx->d_windows + idx->woff[k], p.window_len, 0u, 0u, 0u};
                }
                if (hipMemcpyAsync(d_moves, h_moves, n * sizeof(IndexMove), hipMemcpyHostToDevice, st) != hipSuccess) e = ZNG_ROCM_EHIP;
            }
            if (!e) e = host_tables_release(ws, st);
        }
        if (!e) {
            hipLaunchKernelGGL(index_windows_kernel, dim3((unsigned)(n < (1u << 20) ? n : (1u << 20))), dim3(256), 0, st, d_moves, (uint32_t)n);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) e = ZNG_ROCM_EHIP;
        }
        if (e) {
            set_error("%s: gathering the windows failed", who);
            zng_rocm_inflate_index_destroy(idx);
            return e;
        }
    }
    *out = idx;
    return ZNG_ROCM_OK;
}

}  // namespace zr

using namespace zr;

extern "C" {

int zng_rocm_inflate_index_read_last_decoded(void) { return t_idx_decoded; }
int zng_rocm_inflate_index_read_last_direct(void) { return t_idx_direct; }
int zng_rocm_inflate_index_read_last_rounds(void) { return t_idx_rounds; }

size_t zng_rocm_inflate_index_points(const zng_rocm_inflate_index *idx, zng_rocm_access_point *pts, size_t cap) {
    if (!idx) return 0;
    for (size_t k = 0; k < idx->pts.size() && k < cap && pts; ++k) pts[k] = idx->pts[k];
    return idx->pts.size();
}

uint64_t zng_rocm_inflate_index_plain_len(const zng_rocm_inflate_index *idx) { return idx ? idx->head.plain_len : 0u; }

void zng_rocm_inflate_index_destroy(zng_rocm_inflate_index *idx) {
    if (!idx) return;
    if (idx->d_windows && ctx()) {
        DeviceGuard dev;
        (void)hipFree(idx->d_windows);
    }
    delete idx;
}

int zng_rocm_inflate_index_build_dev(int format, const uint8_t *d_src, size_t src_len, uint8_t *d_dst, size_t dst_cap, uint64_t *out_len,
                                     size_t *in_used, uint64_t span_bytes, size_t piece_bytes, uint32_t flags,
                                     zng_rocm_inflate_index **out, void *stream) {
    if (out) *out = nullptr;
    const uint64_t span = index_span_bytes(span_bytes);
    if (!out || !span) {
        if (out_len) *out_len = 0;
        if (in_used) *in_used = 0;
        set_error("zng_rocm_inflate_index_build_dev: a null result pointer, or span_bytes outside 64 KiB .. 1 GiB");
        return ZNG_ROCM_EINVAL;
    }
    IndexSink sink;
    inflate_index_sink_set(&sink);
    const int rc = zng_rocm_uncompress_large_dev(format, d_src, src_len, nullptr, 0, d_dst, dst_cap, out_len, in_used, piece_bytes, flags,
                                                 stream);
    inflate_index_sink_set(nullptr);
    if (rc != 1) return rc;
    // (from here on the outputs and the last-error text are the uncompress call's: nothing below touches them on success)
    const uint64_t plain_len = *out_len;
    std::vector<IndexCand> cands(sink.cands.size());
    for (size_t i = 0; i < cands.size(); ++i) cands[i] = IndexCand{sink.cands[i].first + 8 * sink.header_len, sink.cands[i].second};
    if (int e = inflate_index_from_cands("zng_rocm_inflate_index_build_dev", IndexHead{(uint32_t)format, sink.header_len, (uint64_t)*in_used, plain_len, span},
                                         cands.data(), cands.size(), d_dst, (hipStream_t)stream, out))
        return e;
    return 1;
}

int zng_rocm_inflate_index_read_dev(const zng_rocm_inflate_index *idx, const uint8_t *d_src, size_t src_len, zng_rocm_inflate_range *ranges,
                                    size_t nranges, size_t scratch_bytes, void *stream) {
    t_idx_decoded = t_idx_direct = t_idx_rounds = 0;
    const uint64_t scratch = index_scratch_bytes(scratch_bytes);
    if (!idx || (!d_src && src_len) || (!ranges && nranges) || !scratch || nranges > 0xfffffffeull) {
        set_error("zng_rocm_inflate_index_read_dev: a null index, a null buffer with a length, more than 2^32 - 2 ranges, or "
                  "scratch_bytes outside 1 MiB .. 4 GiB");
        return ZNG_ROCM_EINVAL;
    }
    const size_t n = idx->pts.size();
    // every point has to begin inside the file: a shorter one is not the file this index was built from (a file that ends
    // behind the last point's first byte is read as far as it goes: spans it cuts report -5)
    if ((idx->pts[n - 1].in_bit >> 3) >= src_len) {
        set_error("zng_rocm_inflate_index_read_dev: src_len %zu ends in front of the index's last point (byte %llu)", src_len,
                  (unsigned long long)(idx->pts[n - 1].in_bit >> 3));
        return ZNG_ROCM_EINVAL;
    }
    for (size_t r = 0; r < nranges; ++r)
        if (!ranges[r].d_dst && ranges[r].len) {
            set_error("zng_rocm_inflate_index_read_dev: ranges[%zu]: a null d_dst with a length", r);
            return ZNG_ROCM_EINVAL;
        }
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    const zng_rocm_access_point *pts = idx->pts.data();
    std::vector<IndexRangeIn> in(nranges);
    for (size_t r = 0; r < nranges; ++r) in[r] = IndexRangeIn{ranges[r].uoff, ranges[r].len};
    IndexReadPlan plan;
    index_read_plan(pts, n, idx->head.plain_len, in.data(), nranges, scratch, kIndexRoundJobs, plan);
    auto finish = [&](size_t r, const IndexRangeOut &o) {
        ranges[r].status = o.status;
        ranges[r].out_len = o.out_len;
        ranges[r].msg = range_msg(o);
    };
    // the ranges no round holds: empty, beyond the end, or wholly on spans the engine does not take
    std::vector<IndexJobVerdict> verdicts(plan.jobs.size(), IndexJobVerdict{1, 0u});
    auto finish_upto = [&](size_t &next_range, size_t range_end, size_t &k, size_t part_end) {
        for (; next_range < range_end; ++next_range) {
            const size_t from = k;
            while (k < part_end && plan.parts[k].range == next_range) ++k;
            finish(next_range, index_range_result(plan.parts.data() + from, k - from, verdicts.data(), plan.clipped[next_range]));
        }
    };
    size_t next_range = 0, k = 0;
    if (plan.rounds.empty()) {
        finish_upto(next_range, nranges, k, plan.parts.size());
        return ZNG_ROCM_OK;
    }
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard dev;
    Workspace *ws = workspace_for(st);
    if (!ws) return ZNG_ROCM_ENOMEM;

    // device: results | jobs | span table | slices | slots, sized for the largest round (every part 16-byte aligned);
    // pinned: jobs | span table | slices (one copy up) | results
    size_t max_jobs = 0, max_slices = 0;
    uint64_t max_slots = 0;
    for (const IndexReadRound &rd : plan.rounds) {
        if (rd.job_end - rd.job_begin > max_jobs) max_jobs = rd.job_end - rd.job_begin;
        if (rd.slices > max_slices) max_slices = rd.slices;
        if (rd.slot_bytes > max_slots) max_slots = rd.slot_bytes;
    }
    const size_t b_res = up16(max_jobs * 4 * sizeof(uint32_t)), b_jobs = up16(max_jobs * sizeof(InflateJobDev)),
                 b_spans = up16(max_jobs * sizeof(InflateSpanDev)), b_slices = up16(max_slices * sizeof(IndexMove));
    const size_t o_jobs = b_res, o_spans = o_jobs + b_jobs, o_slices = o_spans + b_spans, o_slots = o_slices + b_slices;
    const size_t up_bytes = b_jobs + b_spans + b_slices;
    uint8_t *d = nullptr, *h = nullptr;
    {
        std::lock_guard<std::mutex> use(ws->mu);
        if (int rc = scratch_reserve(ws, kScrIndexRead, o_slots + (size_t)max_slots, false, (void **)&d)) return rc;
        if (int rc = host_tables_acquire(ws)) return rc;
        if (int rc = scratch_reserve(ws, kScrIndexReadHost, up_bytes + b_res, true, (void **)&h)) return rc;
    }
    uint32_t *d_res = reinterpret_cast<uint32_t *>(d);
    uint8_t *d_slots = d + o_slots;
    const uint32_t *h_res = reinterpret_cast<const uint32_t *>(h + up_bytes);

    for (const IndexReadRound &rd : plan.rounds) {
        const size_t nj = rd.job_end - rd.job_begin;
        // a round's tables are laid out for ITS counts, one behind the other, so that they go up in one copy
        const size_t r_spans = up16(nj * sizeof(InflateJobDev)), r_slices = r_spans + up16(nj * sizeof(InflateSpanDev));
        const size_t r_bytes = r_slices + rd.slices * sizeof(IndexMove);
        {
            std::lock_guard<std::mutex> use(ws->mu);
            if (int rc = host_tables_acquire(ws)) return rc;
            InflateJobDev *hj = reinterpret_cast<InflateJobDev *>(h);
            InflateSpanDev *hs = reinterpret_cast<InflateSpanDev *>(h + r_spans);
            IndexMove *hm = reinterpret_cast<IndexMove *>(h + r_slices);
            for (size_t j = 0; j < nj; ++j) {
                const IndexReadJob &job = plan.jobs[rd.job_begin + j];
                const zng_rocm_access_point &p = pts[job.span];
                const uint64_t byte = p.in_bit >> 3, room = src_len - byte;
                hj[j] = InflateJobDev{d_src + byte, job.slot == kIndexDirect ? ranges[job.range].d_dst + job.at : d_slots + job.slot,
                                      room < 0x7fffffffull ? room : 0x7fffffffull, job.out_cap, p.window_len, 0u};
                hs[j] = InflateSpanDev{idx->d_windows + idx->woff[job.span] + p.window_len, (uint32_t)(p.in_bit & 7u), 0u};
            }
            size_t s = 0;
            for (size_t q = rd.part_begin; q < rd.part_end; ++q) {
                const IndexReadPart &part = plan.parts[q];
                if (!part.slice) continue;
                const IndexReadJob &job = plan.jobs[part.job];
                hm[s++] = IndexMove{d_slots + job.slot + part.off, ranges[part.range].d_dst + part.at, (uint32_t)part.len,
                                    (uint32_t)(part.job - rd.job_begin), (uint32_t)job.out_cap, 0u};
            }
            ZR_HIP(hipMemcpyAsync(d + o_jobs, h, r_bytes, hipMemcpyHostToDevice, st));
            if (int rc = host_tables_release(ws, st)) return rc;
        }
        if (int rc = launch_inflate_streams_span_device(reinterpret_cast<const InflateJobDev *>(d + o_jobs), nj, d_res,
                                                        reinterpret_cast<const InflateSpanDev *>(d + o_jobs + r_spans), st))
            return rc;
        if (rd.slices) {
            const uint32_t grid = rd.slices < (1u << 20) ? rd.slices : (1u << 20);
            hipLaunchKernelGGL(index_slices_kernel, dim3(grid), dim3(256), 0, st, reinterpret_cast<const IndexMove *>(d + o_jobs + r_slices),
                               rd.slices, d_res);
            ZR_HIP(hipGetLastError());
        }
        ZR_HIP(hipMemcpyAsync((void *)h_res, d_res, nj * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        ZR_HIP(hipStreamSynchronize(st));
        ++t_idx_rounds;
        for (size_t j = 0; j < nj; ++j) verdicts[rd.job_begin + j] = index_job_verdict(h_res + 4 * j, (uint32_t)plan.jobs[rd.job_begin + j].out_cap);
        // the ranges of this round, and the ones without a job in front of it, in order; a range's parts stand together
        finish_upto(next_range, rd.range_end, k, rd.part_end);
    }
    finish_upto(next_range, nranges, k, plan.parts.size());
    t_idx_decoded = (int)plan.decoded;
    t_idx_direct = (int)plan.direct;
    return ZNG_ROCM_OK;
}

int zng_rocm_inflate_index_export(const zng_rocm_inflate_index *idx, uint8_t *buf, size_t cap, size_t *need, void *stream) {
    if (need) *need = 0;
    if (!idx || !need || (!buf && cap)) return ZNG_ROCM_EINVAL;
    const size_t n = idx->pts.size();
    const uint64_t total = index_blob_bytes(idx->pts.data(), n);
    *need = (size_t)total;
    if (cap < total) return -5;
    index_blob_write(idx->head, idx->pts.data(), n, buf);
    if (idx->woff.back()) {
        if (!ctx()) {
            set_error("zng_rocm_init() has not succeeded");
            return ZNG_ROCM_ENODEV;
        }
        DeviceGuard dev;
        hipStream_t st = (hipStream_t)stream;
        ZR_HIP(hipMemcpyAsync(buf + kIndexBlobHead + kIndexBlobRow * n, idx->d_windows, (size_t)idx->woff.back(), hipMemcpyDeviceToHost, st));
        ZR_HIP(hipStreamSynchronize(st));
    }
    return ZNG_ROCM_OK;
}

int zng_rocm_inflate_index_import_dev(const uint8_t *buf, size_t len, zng_rocm_inflate_index **out, void *stream) {
    if (out) *out = nullptr;
    if (!out || (!buf && len)) return ZNG_ROCM_EINVAL;
    IndexHead head;
    std::vector<zng_rocm_access_point> pts;
    if (const uint32_t why = index_blob_check(buf, len, head, pts)) {
        set_error("zng_rocm_inflate_index_import_dev: %s", index_blob_why(why));
        return ZNG_ROCM_EINVAL;
    }
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    DeviceGuard dev;
    const size_t n = pts.size();
    zng_rocm_inflate_index *idx = nullptr;
    if (int e = index_new(head, pts, &idx)) return e;
    if (idx->woff.back()) {
        hipStream_t st = (hipStream_t)stream;
        if (hipMemcpyAsync(idx->d_windows, buf + kIndexBlobHead + kIndexBlobRow * n, (size_t)idx->woff.back(), hipMemcpyHostToDevice, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            set_error("zng_rocm_inflate_index_import_dev: the copy of the windows failed");
            zng_rocm_inflate_index_destroy(idx);
            return ZNG_ROCM_EHIP;
        }
    }
    *out = idx;
    return ZNG_ROCM_OK;
}

}  // extern "C"
