// framing_large.hip -- zlib (RFC 1950) and gzip (RFC 1952) members around the LARGE device inflaters: what inflate() does
// in front of and behind the deflate data (inflate.c:509-715 header and dictionary id, :1105-1147 check value and length)
// for members that already sit in device memory, with the payload left to zng_rocm_inflate_large_streams_dev (a batch) or
// zng_rocm_inflate_large_pieces_dev (one member of any length):
//   header   one wavefront per member runs the shared rules (framing_parse.h); the terminators of FNAME / FCOMMENT are
//            searched 4 KiB per step (16 bytes per lane, four lines in flight, first zero by ballot); a gzip FHCRC goes
//            through the many-message checksum pass over descriptors filled by that kernel, a second small kernel compares
//            the 16 bits; zlib: the Adler-32 of every dictionary given in one zng_rocm_checksums_dev pass
//   ONE readback of the header table (+ the dictionaries' Adler-32), the host patches a private copy of the job array
//   payload  the raw engine, unchanged
//   check    every output cut into 512 KiB sub-messages, ALL of them through one many-message pass (one workgroup each, so a
//            round of a dozen outputs fills the chip), folded per member by one workgroup (adler32_combine_ /
//            crc32_combine_, adler32.c:32-54, crc32_braid_comb.c:16-18, in the closed form of slots.hip's combine_kernel);
//            the single call runs the full-grid checksum kernel over its one output instead
//   trailer  one lane per member compares check value and ISIZE; the rows come back with the final synchronisation
// `format`: 0 = raw (the raw call itself), 1 = zlib, 2 = gzip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "checksum_args.h"
#include "context.h"
#include "framing_large.h"
#include "framing_parse.h"
#include "inflate_dev.h"
#include "inflate_large_limits.h"
#include "inflate_large_size_plan.h"
#include "gf2.h"

namespace zr {

// One sub-message of the check pass: 32 units of 16 KiB.  One workgroup streams about 26 GB/s (derived), so a
// sub-message is its workgroup's ~20 us and a round of 100 MiB is one sub-message per CU.  4 MiB was measured first
// (profiles/uncompress_large_rate_4mib_v0.json: 0.164 ms for 111 MB, four times the single-message pass over the same
// bytes); with 512 KiB and the descriptors written on the device the same round takes 0.059 ms against 0.039 ms
// (profiles/uncompress_large_rate_v1.json).
constexpr uint64_t kSubBytes = 512ull << 10;
// the single call's full-grid pass takes its output in steps of this many bytes (launch_checksum: < 16 GiB per launch), the
// seeds chained through a device word; tests lower it (zng_rocm_debug_uncompress_large_chunk) to reach the chaining
static uint64_t g_whole_chunk = 8ull << 30;
constexpr int kCutJobs = 64;                             // messages per launch of large_cut_kernel (they travel as kernel arguments)

struct TrailJob {
    const uint8_t *src;
    uint64_t src_len;
    uint64_t at;                                         // header + what the raw call consumed: where the trailer begins
    uint64_t out_len;
};

struct TrailRow {
    uint64_t in_used;
    int32_t status;
    uint32_t msg;
};

struct FoldJob {                                         // one message of zng_rocm_checksums_cut_dev
    const uint8_t *buf;
    uint64_t total;
    uint32_t adler, crc;                                 // seeds
};

struct CutArgs {                                         // up to kCutJobs messages and the first sub-message row of each
    FoldJob jobs[kCutJobs];
    uint32_t first[kCutJobs + 1];
    uint32_t n, base;                                    // messages in this launch; index of the first one in the call
};

// one wavefront per member
__global__ __launch_bounds__(64)
void large_header_kernel(const HeadJob *__restrict__ jobs, uint32_t njobs, int format, const DeviceTables *__restrict__ tabs,
                         WrapperHead *__restrict__ rows, StreamArgs *__restrict__ sa, FinalArgs *__restrict__ fa) {
    const uint32_t i = blockIdx.x;
    if (i >= njobs) return;
    const HeadJob j = jobs[i];
    const WaveBytes in{j.src};
    const WrapperHead h = wrapper_parse_rules(format, in, j.len);
    if (threadIdx.x != 0) return;
    rows[i] = h;
    if (format == 2)                                     // the FHCRC covers the header in front of it (inflate.c:686-692)
        fill_check_descriptor(j.src, h.status == 0 && h.hcrc ? h.header_len - 2 : 0, tabs, 0, 1, sa + i, fa + i);
}

__global__ __launch_bounds__(256)
void large_hcrc_kernel(WrapperHead *__restrict__ rows, const uint32_t *__restrict__ crc2, uint32_t njobs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= njobs) return;
    if (rows[i].status == 0 && rows[i].hcrc && (crc2[2 * i + 1] & 0xffffu) != rows[i].hcrc_stored) {
        rows[i].status = -3;
        rows[i].msg = kWrapHeaderCrc;
    }
}

// One workgroup per message writes the descriptors of its sub-messages for the many-message checksum pass, and the message's
// row of the tables large_fold_kernel reads.  The messages arrive as kernel arguments: no table to copy up first.
__global__ __launch_bounds__(256)
void large_cut_kernel(const CutArgs args, int which, const DeviceTables *__restrict__ tabs, FoldJob *__restrict__ jobs,
                      uint32_t *__restrict__ first, StreamArgs *__restrict__ sa, FinalArgs *__restrict__ fa) {
    const uint32_t j = blockIdx.x, t = threadIdx.x;
    if (j >= args.n) return;
    const FoldJob job = args.jobs[j];
    const uint32_t lo = args.first[j], hi = args.first[j + 1];
    if (t == 0) {
        jobs[args.base + j] = job;
        first[args.base + j] = lo;
        if (j + 1 == args.n) first[args.base + j + 1] = hi;
    }
    for (uint32_t r = lo + t; r < hi; r += 256) {
        const uint64_t begin = (uint64_t)(r - lo) * kSubBytes;
        const uint64_t len = job.total - begin < kSubBytes ? job.total - begin : kSubBytes;
        fill_check_descriptor(job.buf + begin, len, tabs, which & 1, (which >> 1) & 1, sa + r, fa + r);
    }
}

// One workgroup per message folds the checks of its sub-messages, rows [first[j], first[j + 1]) of sub2, in order, behind
// the message's seeds.  All sub-messages but the last are kSubBytes long, so "bytes behind row r" is known without a scan.
__global__ __launch_bounds__(256)
void large_fold_kernel(const uint32_t *__restrict__ sub2, const uint32_t *__restrict__ first, const FoldJob *__restrict__ jobs,
                       int which, const DeviceTables *__restrict__ tabs, uint32_t *__restrict__ out2) {
    __shared__ unsigned long long red_a[4], red_b[4];
    __shared__ uint32_t red_c[4];
    const uint32_t j = blockIdx.x, t = threadIdx.x;
    const uint32_t lo = first[j], hi = first[j + 1];
    const uint64_t total = jobs[j].total;
    uint32_t c = 0;
    unsigned long long a = 0, b = 0;
    for (uint32_t r = lo + t; r < hi; r += 256) {
        const uint64_t begin = (uint64_t)(r - lo) * kSubBytes;
        const uint64_t end = begin + kSubBytes < total ? begin + kSubBytes : total;
        const uint64_t len = end - begin, after = total - end;
        if (which & 2) c ^= mulmod(sub2[2 * r + 1], xpow_bytes(tabs->pow_tab, after));
        if (which & 1) {                                 // linear form of the block: A = s1 - 1, B = s2 - len (seed 1 implied)
            const uint32_t chk = sub2[2 * r];
            const unsigned long long s1 = chk & 0xffffu, s2 = chk >> 16;
            const unsigned long long A = (s1 + kAdlerBase - 1) % kAdlerBase;
            const unsigned long long B = (s2 + kAdlerBase - len % kAdlerBase) % kAdlerBase;
            a += A;
            b = (b + B + A * (after % kAdlerBase)) % kAdlerBase;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        c ^= __shfl_xor(c, m, 64);
        a += __shfl_xor(a, m, 64);
        b += __shfl_xor(b, m, 64);
    }
    if ((t & 63u) == 0) {
        red_c[t >> 6] = c;
        red_a[t >> 6] = a;
        red_b[t >> 6] = b;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t cc = 0;
        unsigned long long A = 0, B = 0;
        for (int w = 0; w < 4; ++w) {
            cc ^= red_c[w];
            A += red_a[w] % kAdlerBase;
            B += red_b[w] % kAdlerBase;
        }
        if (which & 1) {                                 // from the seed (s1, s2): s1 + A, s2 + s1 * total + B
            const unsigned long long s1 = jobs[j].adler & 0xffffu, s2 = jobs[j].adler >> 16;
            const unsigned long long r1 = (s1 + A) % kAdlerBase, r2 = (s2 + s1 * (total % kAdlerBase) + B) % kAdlerBase;
            out2[2 * j] = (uint32_t)(r1 | (r2 << 16));
        }
        if (which & 2) out2[2 * j + 1] = cc ^ mulmod(jobs[j].crc, xpow_bytes(tabs->pow_tab, total));
    }
}

// inflate.c:1105-1147: the check value and gzip's ISIZE (wrapper_trailer_verdict)
__global__ __launch_bounds__(256)
void large_trailer_kernel(const TrailJob *__restrict__ jobs, const uint32_t *__restrict__ checks2, uint32_t njobs, int format,
                          TrailRow *__restrict__ rows) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= njobs) return;
    const TrailJob j = jobs[i];
    const uint32_t tail = wrapper_tail_bytes(format);
    TrailRow r = {j.at + tail, 1, kWrapNone};
    if (j.at + tail > j.src_len) {                       // the member ends inside its trailer
        r.status = -5;
        r.in_used = j.src_len;
    } else {
        const uint32_t adler = format == 1 ? checks2[2 * i] : 0u, crc = format == 2 ? checks2[2 * i + 1] : 0u;
        r.msg = wrapper_trailer_verdict(format, j.src + j.at, adler, crc, j.out_len);
        if (r.msg != kWrapNone) r.status = -3;
    }
    rows[i] = r;
}

namespace {

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

// framing_large.h: the header kernels over jobs that already sit in device memory
size_t header_rows_scratch(size_t n) {
    return up16(n * sizeof(StreamArgs)) + up16(n * sizeof(FinalArgs)) + n * sizeof(Partial) + n * 2 * sizeof(uint32_t);
}

int header_rows_device(int format, const HeadJob *d_jobs, size_t n, WrapperHead *d_rows, uint8_t *d_work, hipStream_t st) {
    Context *c = ctx();
    const size_t o_fa = up16(n * sizeof(StreamArgs)), o_part = o_fa + up16(n * sizeof(FinalArgs)), o_crc = o_part + n * sizeof(Partial);
    StreamArgs *d_sa = reinterpret_cast<StreamArgs *>(d_work);
    FinalArgs *d_fa = reinterpret_cast<FinalArgs *>(d_work + o_fa);
    hipLaunchKernelGGL(large_header_kernel, dim3((unsigned)n), dim3(64), 0, st, d_jobs, (uint32_t)n, format, c->tables, d_rows, d_sa, d_fa);
    ZR_HIP(hipGetLastError());
    if (format == 2) {
        uint32_t *d_crc = reinterpret_cast<uint32_t *>(d_work + o_crc);
        if (int rc = launch_checksum_batch_device(false, true, d_sa, d_fa, reinterpret_cast<Partial *>(d_work + o_part), n, d_crc, st))
            return rc;
        hipLaunchKernelGGL(large_hcrc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_rows, d_crc, (uint32_t)n);
        ZR_HIP(hipGetLastError());
    }
    return ZNG_ROCM_OK;
}

namespace {

// Every header parsed on the device and, for zlib, the Adler-32 of every dictionary given; one readback.
int header_phase(int format, const zng_rocm_inflate_large_job *jobs, size_t n, Workspace *ws, hipStream_t st,
                 std::vector<WrapperHead> &rows, std::vector<uint32_t> &dict_adler) {
    std::vector<zng_rocm_check_job> dj;
    std::vector<size_t> dj_of;
    if (format == 1)
        for (size_t i = 0; i < n; ++i)
            if (jobs[i].window_len) {
                dj.push_back(zng_rocm_check_job{jobs[i].d_window, jobs[i].window_len, 1u, 0u});
                dj_of.push_back(i);
            }
    const size_t nd = dj.size();
    const size_t o_dict = n * sizeof(WrapperHead), down = o_dict + nd * 2 * sizeof(uint32_t);
    const size_t o_jobs = up16(down), o_work = up16(o_jobs + n * sizeof(HeadJob));
    const size_t total = o_work + header_rows_scratch(n), h_down = up16(n * sizeof(HeadJob));
    uint8_t *d = nullptr, *h = nullptr;
    {
        std::lock_guard<std::mutex> use(ws->mu);
        if (int rc = scratch_reserve(ws, kScrFrameLarge, total, false, (void **)&d)) return rc;
        if (int rc = host_tables_acquire(ws)) return rc;
        if (int rc = scratch_reserve(ws, kScrFrameLargeHost, h_down + down, true, (void **)&h)) return rc;
        HeadJob *hj = reinterpret_cast<HeadJob *>(h);
        for (size_t i = 0; i < n; ++i) hj[i] = HeadJob{jobs[i].d_src, jobs[i].src_len};
        ZR_HIP(hipMemcpyAsync(d + o_jobs, h, n * sizeof(HeadJob), hipMemcpyHostToDevice, st));
        if (int rc = host_tables_release(ws, st)) return rc;
        if (int rc = header_rows_device(format, reinterpret_cast<const HeadJob *>(d + o_jobs), n, reinterpret_cast<WrapperHead *>(d),
                                        d + o_work, st))
            return rc;
    }
    if (nd)                                              // takes the stream's workspace itself
        if (int rc = zng_rocm_checksums_dev(1, dj.data(), nd, reinterpret_cast<uint32_t *>(d + o_dict), st)) return rc;
    std::lock_guard<std::mutex> use(ws->mu);
    ZR_HIP(hipMemcpyAsync(h + h_down, d, down, hipMemcpyDeviceToHost, st));
    ZR_HIP(hipStreamSynchronize(st));
    rows.resize(n);
    memcpy(rows.data(), h + h_down, n * sizeof(WrapperHead));
    dict_adler.assign(n, 0u);
    const uint32_t *da = reinterpret_cast<const uint32_t *>(h + h_down + o_dict);
    for (size_t k = 0; k < nd; ++k) dict_adler[dj_of[k]] = da[2 * k];
    return ZNG_ROCM_OK;
}

// what the header says about member i before any payload is decoded; true: the payload goes to the raw engine with
// `*window_len` bytes of dictionary
bool header_verdict(const WrapperHead &h, const zng_rocm_inflate_large_job &given, uint32_t dict_adler, zng_rocm_inflate_large_job *out,
                    uint32_t *window_len) {
    out->out_len = 0;
    out->in_used = 0;
    out->msg = nullptr;
    out->parts = out->subparts = 0;
    *window_len = 0;
    if (h.status == -3) {
        out->status = -3;
        out->msg = wrapper_message(h.msg);
        return false;
    }
    if (h.status == -5) {
        out->status = -5;
        out->in_used = given.src_len;
        return false;
    }
    if (h.fdict) {                                       // inflate.c:702-715, inflateSetDictionary inflate.c:1214-1261
        if (!given.window_len) {
            out->status = 2;                             // Z_NEED_DICT
            out->in_used = 6;
            return false;
        }
        if (dict_adler != h.dictid) {
            out->status = -3;
            return false;
        }
        *window_len = given.window_len;
    }
    return true;                                         // FDICT clear: a dictionary is only taken in state DICT, so none here
}

// zng_rocm_checksums_cut_dev: every message cut into sub-messages of kSubBytes whose descriptors are written on the
// device, ALL of them through one many-message pass (one workgroup each), one workgroup per message folds.  Nothing is
// copied up and nothing is waited for.  Asynchronous on `st`.
int checks_cut(int which, const zng_rocm_check_job *jobs, size_t m, uint32_t *d_out2, Workspace *ws, hipStream_t st) {
    Context *c = ctx();
    std::vector<uint32_t> first(m + 1, 0u);
    uint64_t ns = 0;
    for (size_t k = 0; k < m; ++k) {
        ns += (jobs[k].len + kSubBytes - 1) / kSubBytes;
        if (ns > 0x7fffffffull) {
            set_error("more than 2^31 sub-messages of %llu bytes in one call", (unsigned long long)kSubBytes);
            return ZNG_ROCM_EINVAL;
        }
        first[k + 1] = (uint32_t)ns;
    }
    const size_t o_first = m * sizeof(FoldJob), o_sa = up16(o_first + (m + 1) * sizeof(uint32_t));
    const size_t o_fa = up16(o_sa + ns * sizeof(StreamArgs)), o_part = up16(o_fa + ns * sizeof(FinalArgs));
    const size_t o_sub = o_part + ns * sizeof(Partial);
    uint8_t *d = nullptr;
    {
        std::lock_guard<std::mutex> use(ws->mu);
        if (int rc = scratch_reserve(ws, kScrCheckCut, o_sub + ns * 2 * sizeof(uint32_t), false, (void **)&d)) return rc;
    }
    FoldJob *d_jobs = reinterpret_cast<FoldJob *>(d);
    uint32_t *d_first = reinterpret_cast<uint32_t *>(d + o_first), *d_sub = reinterpret_cast<uint32_t *>(d + o_sub);
    StreamArgs *d_sa = reinterpret_cast<StreamArgs *>(d + o_sa);
    FinalArgs *d_fa = reinterpret_cast<FinalArgs *>(d + o_fa);
    for (size_t base = 0; base < m; base += kCutJobs) {
        CutArgs args;
        args.n = (uint32_t)(m - base < (size_t)kCutJobs ? m - base : (size_t)kCutJobs);
        args.base = (uint32_t)base;
        for (uint32_t k = 0; k < args.n; ++k) {
            const zng_rocm_check_job &j = jobs[base + k];
            args.jobs[k] = FoldJob{(const uint8_t *)j.buf, j.len, j.adler, j.crc};
            args.first[k] = first[base + k];
        }
        for (uint32_t k = args.n; k < (uint32_t)kCutJobs; ++k) args.jobs[k] = FoldJob{nullptr, 0, 0, 0};
        for (uint32_t k = args.n; k <= (uint32_t)kCutJobs; ++k) args.first[k] = first[base + args.n];
        hipLaunchKernelGGL(large_cut_kernel, dim3(args.n), dim3(256), 0, st, args, which, c->tables, d_jobs, d_first, d_sa, d_fa);
        ZR_HIP(hipGetLastError());
    }
    if (int rc = launch_checksum_batch_device((which & 1) != 0, (which & 2) != 0, d_sa, d_fa, reinterpret_cast<Partial *>(d + o_part),
                                              (size_t)ns, d_sub, st))
        return rc;
    hipLaunchKernelGGL(large_fold_kernel, dim3((unsigned)m), dim3(256), 0, st, d_sub, d_first, d_jobs, which, c->tables, d_out2);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

// Check values of the outputs at dst[k] (tj[k].out_len bytes) and the trailer compare.  `whole`: one member, the
// full-grid checksum kernel over its output; else checks_cut.
int check_phase(int format, bool whole, const std::vector<TrailJob> &tj, const std::vector<const uint8_t *> &dst, Workspace *ws,
                hipStream_t st, std::vector<TrailRow> &out) {
    const size_t m = tj.size();
    out.clear();
    if (!m) return ZNG_ROCM_OK;
    const size_t o_jobs = up16(m * sizeof(TrailRow)), o_checks = o_jobs + m * sizeof(TrailJob);
    const size_t total = o_checks + (m + 1) * 2 * sizeof(uint32_t), h_down = m * sizeof(TrailJob);
    uint8_t *d = nullptr, *h = nullptr;
    {
        std::lock_guard<std::mutex> use(ws->mu);
        if (int rc = scratch_reserve(ws, kScrFrameLarge, total, false, (void **)&d)) return rc;
        if (int rc = host_tables_acquire(ws)) return rc;
        if (int rc = scratch_reserve(ws, kScrFrameLargeHost, h_down + m * sizeof(TrailRow), true, (void **)&h)) return rc;
        memcpy(h, tj.data(), m * sizeof(TrailJob));
        ZR_HIP(hipMemcpyAsync(d + o_jobs, h, m * sizeof(TrailJob), hipMemcpyHostToDevice, st));
        if (int rc = host_tables_release(ws, st)) return rc;
    }
    const TrailJob *d_jobs = reinterpret_cast<const TrailJob *>(d + o_jobs);
    uint32_t *d_checks = reinterpret_cast<uint32_t *>(d + o_checks);
    if (whole) {                                         // one message; launch_checksum takes < 16 GiB at a time, seeds chained on the device
        const uint64_t kChunk = g_whole_chunk;
        const bool adler = format == 1;
        uint32_t *res = d_checks;
        uint64_t at = 0;
        do {
            const uint64_t len = tj[0].out_len - at < kChunk ? tj[0].out_len - at : kChunk;
            uint32_t *next = at ? (res == d_checks ? d_checks + 2 : d_checks) : d_checks;
            if (int rc = launch_checksum(adler, !adler, 1u, 0u, dst[0] + at, nullptr, (size_t)len, next, next + 1, st,
                                         at && adler ? res : nullptr, at && !adler ? res + 1 : nullptr))
                return rc;
            res = next;
            at += len;
        } while (at < tj[0].out_len);
        d_checks = res;
    } else {
        std::vector<zng_rocm_check_job> cj(m);
        for (size_t k = 0; k < m; ++k) cj[k] = zng_rocm_check_job{dst[k], tj[k].out_len, 1u, 0u};
        if (int rc = checks_cut(format == 1 ? 1 : 2, cj.data(), m, d_checks, ws, st)) return rc;
    }
    TrailRow *d_rows = reinterpret_cast<TrailRow *>(d);
    hipLaunchKernelGGL(large_trailer_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, d_jobs, d_checks, (uint32_t)m, format,
                       d_rows);
    ZR_HIP(hipGetLastError());
    std::lock_guard<std::mutex> use(ws->mu);
    ZR_HIP(hipMemcpyAsync(h + h_down, d_rows, m * sizeof(TrailRow), hipMemcpyDeviceToHost, st));
    ZR_HIP(hipStreamSynchronize(st));
    out.resize(m);
    memcpy(out.data(), h + h_down, m * sizeof(TrailRow));
    return ZNG_ROCM_OK;
}


// the wrapped member `given` through header verdict, raw engine and trailer; `single`: piece_bytes and the pieces call
int uncompress_large(int format, zng_rocm_inflate_large_job *jobs, size_t njobs, bool single, size_t bytes, uint32_t flags,
                     hipStream_t st) {
    DeviceGuard dev;
    Workspace *ws = workspace_for(st);
    if (!ws) return ZNG_ROCM_ENOMEM;
    std::vector<WrapperHead> heads;
    std::vector<uint32_t> dict_adler;
    if (int rc = header_phase(format, jobs, njobs, ws, st, heads, dict_adler)) return rc;
    std::vector<zng_rocm_inflate_large_job> inner;
    std::vector<size_t> inner_of;
    for (size_t i = 0; i < njobs; ++i) {
        uint32_t wl = 0;
        if (!header_verdict(heads[i], jobs[i], dict_adler[i], &jobs[i], &wl)) continue;
        zng_rocm_inflate_large_job p = jobs[i];
        p.d_src = jobs[i].d_src + heads[i].header_len;
        p.src_len = jobs[i].src_len - (size_t)heads[i].header_len;
        p.d_window = wl ? jobs[i].d_window : nullptr;
        p.window_len = wl;
        inner.push_back(p);
        inner_of.push_back(i);
    }
    int rc = ZNG_ROCM_OK;
    if (single) {
        if (!inner.empty()) {
            zng_rocm_inflate_large_job &p = inner[0];
            if (IndexSink *sink = inflate_index_sink()) sink->header_len = heads[inner_of[0]].header_len;
            p.status = zng_rocm_inflate_large_pieces_dev(p.d_src, p.src_len, p.d_window, p.window_len, p.d_dst, p.dst_cap, &p.out_len,
                                                         &p.in_used, bytes, flags, st);
            p.msg = nullptr;                             // the text of a data error is in zng_rocm_last_error() already
            if (p.status == ZNG_ROCM_EHIP || p.status == ZNG_ROCM_ENOMEM || p.status == ZNG_ROCM_ENODEV) rc = p.status;
        }
    } else {
        rc = zng_rocm_inflate_large_streams_dev(inner.data(), inner.size(), bytes, flags, st);
    }
    std::vector<TrailJob> tj;
    std::vector<const uint8_t *> dst;
    std::vector<size_t> tj_of;
    for (size_t k = 0; k < inner.size(); ++k) {
        const zng_rocm_inflate_large_job &p = inner[k];
        zng_rocm_inflate_large_job &j = jobs[inner_of[k]];
        const uint64_t hl = heads[inner_of[k]].header_len;
        j.status = p.status;
        j.out_len = p.out_len;
        j.in_used = p.in_used + (p.status == 1 || p.status == -3 || p.status == -5 ? (size_t)hl : 0);
        j.msg = p.msg;
        j.parts = p.parts;
        j.subparts = p.subparts;
        if (p.status == 1) {
            tj.push_back(TrailJob{j.d_src, j.src_len, hl + p.in_used, p.out_len});
            dst.push_back(j.d_dst);
            tj_of.push_back(inner_of[k]);
        }
    }
    if (rc != ZNG_ROCM_OK) return rc;
    std::vector<TrailRow> rows;
    if (int e = check_phase(format, single, tj, dst, ws, st, rows)) return e;
    for (size_t k = 0; k < rows.size(); ++k) {
        zng_rocm_inflate_large_job &j = jobs[tj_of[k]];
        j.status = rows[k].status;
        j.in_used = (size_t)rows[k].in_used;
        j.msg = wrapper_message(rows[k].msg);
    }
    return ZNG_ROCM_OK;
}

// The plaintext SIZES of the members `jobs` (zng_rocm_uncompress_large_size_dev / _sizes_dev): header phase and verdicts as
// uncompress_large, the counting pass of inflate_large.hip on the payloads, and the trailer's 4 / 8 bytes present and counted
// but not compared (ls_member_tail) -- there is no plaintext whose check value could be taken.
int uncompress_large_sizes(int format, zng_rocm_inflate_large_job *jobs, size_t njobs, size_t round_bytes, bool single, hipStream_t st) {
    if (format == 0) return inflate_large_sizes_raw(jobs, njobs, round_bytes, single, st);
    DeviceGuard dev;
    Workspace *ws = workspace_for(st);
    if (!ws) return ZNG_ROCM_ENOMEM;
    std::vector<WrapperHead> heads;
    std::vector<uint32_t> dict_adler;
    inflate_large_reset_counters();
    if (int rc = header_phase(format, jobs, njobs, ws, st, heads, dict_adler)) return rc;
    std::vector<zng_rocm_inflate_large_job> inner;
    std::vector<size_t> inner_of;
    for (size_t i = 0; i < njobs; ++i) {
        uint32_t wl = 0;
        if (!header_verdict(heads[i], jobs[i], dict_adler[i], &jobs[i], &wl)) continue;
        zng_rocm_inflate_large_job p = jobs[i];
        p.d_src = jobs[i].d_src + heads[i].header_len;
        p.src_len = jobs[i].src_len - (size_t)heads[i].header_len;
        p.d_window = wl ? jobs[i].d_window : nullptr;
        p.window_len = wl;
        inner.push_back(p);
        inner_of.push_back(i);
    }
    const int rc = inflate_large_sizes_raw(inner.data(), inner.size(), round_bytes, single, st);
    for (size_t k = 0; k < inner.size(); ++k) {
        const zng_rocm_inflate_large_job &p = inner[k];
        zng_rocm_inflate_large_job &j = jobs[inner_of[k]];
        const uint64_t hl = heads[inner_of[k]].header_len;
        j.status = p.status;
        j.out_len = p.out_len;
        j.in_used = p.in_used + (p.status == 1 || p.status == -3 || p.status == -5 ? (size_t)hl : 0);
        j.msg = p.msg;
        j.parts = p.parts;
        j.subparts = 0;
        if (p.status == 1) {
            uint64_t used = 0;
            ls_member_tail(format, hl + p.in_used, j.src_len, &j.status, &used);
            j.in_used = (size_t)used;
        }
    }
    return rc;
}

// the refusals of both sizing calls that no job is looked at for: 0 = go on
int sizes_call_check(const char *who, int format, uint32_t flags, size_t round_bytes) {
    if (format < 0 || format > 2) {
        set_error("%s: format %d is none of 0 (raw), 1 (zlib), 2 (gzip)", who, format);
        return ZNG_ROCM_EINVAL;
    }
    if (flags) {
        set_error("%s: flag bits 0x%x (the counting pass has no SUBBLOCK form and takes no flags)", who, flags);
        return ZNG_ROCM_EINVAL;
    }
    if (!ls_round_ok(round_bytes)) {
        set_error("%s: round_bytes %zu outside %zu .. 2 GiB", who, round_bytes, kRoundMin);
        return ZNG_ROCM_EINVAL;
    }
    return ZNG_ROCM_OK;
}

}  // namespace

}  // namespace zr

using namespace zr;

extern "C" {

int zng_rocm_wrapper_parse(int format, const uint8_t *src, size_t src_len, zng_rocm_wrapper_info *info, const char **msg) {
    if (msg) *msg = nullptr;
    if (format < 0 || format > 2 || (!src && src_len) || !info) return ZNG_ROCM_EINVAL;
    WrapperHead h = wrapper_parse_rules(format, HostBytes{src}, src_len);
    if (h.status == 0 && h.hcrc && (wrapper_host_crc32(src, (size_t)h.header_len - 2) & 0xffffu) != h.hcrc_stored) {
        h.status = -3;
        h.msg = kWrapHeaderCrc;
    }
    info->header_len = h.status == 0 ? h.header_len : 0;
    info->dictid = h.status == 0 ? h.dictid : 0;
    info->fdict = h.status == 0 ? h.fdict : 0;
    if (h.status == -3 && msg) *msg = wrapper_message(h.msg);
    return h.status == 0 && h.fdict ? 2 : h.status;
}

// test hook, not part of the ABI (not declared in zng_rocm.h): the step of the single call's check pass; 0 restores 8 GiB
uint64_t zng_rocm_debug_uncompress_large_chunk(uint64_t bytes) {
    const uint64_t was = g_whole_chunk;
    g_whole_chunk = bytes && bytes < (16ull << 30) ? bytes : 8ull << 30;
    return was;
}

int zng_rocm_checksums_cut_dev(int which, const zng_rocm_check_job *jobs, size_t njobs, uint32_t *d_out2, void *stream) {
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    if (!njobs) return ZNG_ROCM_OK;
    if (which < 1 || which > 3 || !jobs || !d_out2 || njobs > 0x7fffffffull) return ZNG_ROCM_EINVAL;
    for (size_t i = 0; i < njobs; ++i)
        if ((!jobs[i].buf && jobs[i].len) || (jobs[i].len >> 34)) {
            set_error("job %zu: null buffer or more than 16 GiB", i);
            return ZNG_ROCM_EINVAL;
        }
    DeviceGuard dev;
    Workspace *ws = workspace_for((hipStream_t)stream);
    if (!ws) return ZNG_ROCM_ENOMEM;
    return checks_cut(which, jobs, njobs, d_out2, ws, (hipStream_t)stream);
}

int zng_rocm_uncompress_large_streams_dev(int format, zng_rocm_inflate_large_job *jobs, size_t njobs, size_t round_bytes,
                                          uint32_t flags, void *stream) {
    if (format < 0 || format > 2) {
        set_error("zng_rocm_uncompress_large_streams_dev: format %d is none of 0 (raw), 1 (zlib), 2 (gzip)", format);
        return ZNG_ROCM_EINVAL;
    }
    if (format == 0) return zng_rocm_inflate_large_streams_dev(jobs, njobs, round_bytes, flags, stream);
    inflate_large_reset_counters();
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    if (flags & ~ZNG_ROCM_INFLATE_SUBBLOCK) {
        set_error("zng_rocm_uncompress_large_streams_dev: unknown flag bits 0x%x", flags & ~ZNG_ROCM_INFLATE_SUBBLOCK);
        return ZNG_ROCM_EINVAL;
    }
    if (round_bytes && (round_bytes < kRoundMin || round_bytes >= kRoundEnd)) {
        set_error("zng_rocm_uncompress_large_streams_dev: round_bytes %zu outside %zu .. 2 GiB", round_bytes, kRoundMin);
        return ZNG_ROCM_EINVAL;
    }
    if ((njobs && !jobs) || njobs > 0x7fffffffull) return ZNG_ROCM_EINVAL;
    for (size_t i = 0; i < njobs; ++i) {
        const zng_rocm_inflate_large_job &j = jobs[i];
        if ((!j.d_src && j.src_len) || j.window_len > 32768u || (j.window_len && !j.d_window) || (!j.d_dst && j.dst_cap)) {
            set_error("zng_rocm_uncompress_large_streams_dev: job %zu: a null buffer with a length, or window_len above 32768", i);
            return ZNG_ROCM_EINVAL;
        }
        if (format == 2 && (j.d_window || j.window_len)) {
            set_error("zng_rocm_uncompress_large_streams_dev: job %zu: a gzip member takes no dictionary", i);
            return ZNG_ROCM_EINVAL;
        }
    }
    if (!njobs) return ZNG_ROCM_OK;
    return uncompress_large(format, jobs, njobs, false, round_bytes, flags, (hipStream_t)stream);
}

int zng_rocm_uncompress_large_sizes_dev(int format, zng_rocm_inflate_large_job *jobs, size_t njobs, size_t round_bytes,
                                        uint32_t flags, void *stream) {
    static const char who[] = "zng_rocm_uncompress_large_sizes_dev";
    if (int rc = sizes_call_check(who, format, flags, round_bytes)) return rc;
    if ((njobs && !jobs) || njobs > 0x7fffffffull) return ZNG_ROCM_EINVAL;
    for (size_t i = 0; i < njobs; ++i)
        if (!ls_job_ok(format, jobs[i].d_src, jobs[i].src_len, jobs[i].d_window, jobs[i].window_len)) {
            set_error("%s: job %zu: a null d_src with a length, a stream of 2 GiB and more, window_len above 32768, a zlib "
                      "dictionary without its bytes, or a gzip member with a dictionary", who, i);
            return ZNG_ROCM_EINVAL;
        }
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    if (!njobs) return ZNG_ROCM_OK;
    return uncompress_large_sizes(format, jobs, njobs, round_bytes, false, (hipStream_t)stream);
}

int zng_rocm_uncompress_large_size_dev(int format, const uint8_t *d_src, size_t src_len, const uint8_t *d_dict, uint32_t dict_len,
                                       uint64_t *out_len, size_t *in_used, uint32_t flags, void *stream) {
    static const char who[] = "zng_rocm_uncompress_large_size_dev";
    if (int rc = sizes_call_check(who, format, flags, 0)) return rc;
    if (!out_len || !in_used || !ls_job_ok(format, d_src, src_len, d_dict, dict_len)) {
        set_error("%s: a null out_len or in_used, a null d_src with a length, a stream of 2 GiB and more, dict_len above 32768, a "
                  "zlib dictionary without its bytes, or a gzip member with a dictionary", who);
        return ZNG_ROCM_EINVAL;
    }
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    zng_rocm_inflate_large_job job = {d_src, src_len, d_dict, dict_len, nullptr, 0, 0, 0, 0, nullptr, 0, 0};
    const int rc = uncompress_large_sizes(format, &job, 1, 0, true, (hipStream_t)stream);
    if (rc != ZNG_ROCM_OK) return rc;
    *out_len = job.out_len;
    *in_used = job.in_used;
    if (job.status == -3 && job.msg) set_error("%s", job.msg);
    return job.status;
}

int zng_rocm_uncompress_large_dev(int format, const uint8_t *d_src, size_t src_len, const uint8_t *d_dict, uint32_t dict_len,
                                  uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, size_t *in_used, size_t piece_bytes,
                                  uint32_t flags, void *stream) {
    if (format < 0 || format > 2) {
        set_error("zng_rocm_uncompress_large_dev: format %d is none of 0 (raw), 1 (zlib), 2 (gzip)", format);
        return ZNG_ROCM_EINVAL;
    }
    if (format == 0)
        return zng_rocm_inflate_large_pieces_dev(d_src, src_len, d_dict, dict_len, d_dst, dst_cap, out_len, in_used, piece_bytes, flags,
                                                 stream);
    inflate_large_reset_counters();
    if (out_len) *out_len = 0;
    if (in_used) *in_used = 0;
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    if (flags & ~ZNG_ROCM_INFLATE_SUBBLOCK) {
        set_error("zng_rocm_uncompress_large_dev: unknown flag bits 0x%x", flags & ~ZNG_ROCM_INFLATE_SUBBLOCK);
        return ZNG_ROCM_EINVAL;
    }
    if (piece_bytes && (piece_bytes < kPieceMin || piece_bytes > kPieceMax)) {
        set_error("zng_rocm_uncompress_large_dev: piece_bytes %zu outside %zu .. %zu", piece_bytes, kPieceMin, kPieceMax);
        return ZNG_ROCM_EINVAL;
    }
    if ((!d_src && src_len) || dict_len > 32768u || (dict_len && !d_dict) || (!d_dst && dst_cap) || !out_len || !in_used)
        return ZNG_ROCM_EINVAL;
    if (format == 2 && (d_dict || dict_len)) {
        set_error("zng_rocm_uncompress_large_dev: a gzip member takes no dictionary");
        return ZNG_ROCM_EINVAL;
    }
    zng_rocm_inflate_large_job job = {d_src, src_len, d_dict, dict_len, d_dst, dst_cap, 0, 0, 0, nullptr, 0, 0};
    const int rc = uncompress_large(format, &job, 1, true, piece_bytes, flags, (hipStream_t)stream);
    if (rc != ZNG_ROCM_OK) return rc;
    *out_len = job.out_len;
    *in_used = job.in_used;
    if (job.status == -3 && job.msg) set_error("%s", job.msg);
    return job.status;
}

}  // extern "C"
