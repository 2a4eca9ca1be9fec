// framing_dev.hip -- zlib (RFC 1950) and gzip (RFC 1952) framing for MANY device-resident streams: the compress2 /
// uncompress2 class front ends (compress.c:31-69, uncompr.c:25-76) in the shape of the reference's many-stream model
// (test/pigz/CMakeLists.txt:123-200), with nothing on the host between the kernels:
//   compress    zng_rocm_deflate_quick_dev (level-1 class) -> [CRC-32 of every plaintext in one pass, gzip only]
//               -> one small kernel writes every header and trailer (deflate.c:868-892 / :902-1031, :1091-1103)
//   uncompress  one small kernel parses every header (inflate.c:509-555 zlib, :556-700 gzip incl. FHCRC) and patches
//               the job table -> inflate_streams_kernel -> the checksum descriptors of the outputs are filled ON THE
//               DEVICE (only it knows the lengths) -> many-message checksum pass -> one small kernel compares the
//               trailers (inflate.c:1105-1147: "incorrect data check", "incorrect length check")
// `format`: 0 = raw, 1 = zlib, 2 = gzip (as oneshot.hip).
//
// The level-1 class writes its block at a 4-byte aligned address, so both headers are 12 bytes long: gzip declares an
// empty FEXTRA field (XLEN = 0), zlib puts two empty stored blocks (the 5-byte Z_SYNC_FLUSH marker, deflate.c:1064-1076,
// twice) between its 2-byte header and the block -- valid RFC 1951 that every inflater skips.
//
// The *_dict calls are the same two pipelines for raw and zlib streams that share ONE preset dictionary (zng_rocm_dict,
// dict.hip; deflateSetDictionary / inflateSetDictionary, deflate.c:456-512, inflate.c:1234-1260): the level-1 class and the
// inflater in their dictionary forms, and a 16-byte zlib wrapper with FDICT and the DICTID (dict_plan.h).  The same three
// wrapper kernels and the same two host bodies serve both; with a dictionary the header is judged by dict_parse_header.
//
// The rules of the wrappers -- the order of the header checks, the FHCRC, the trailer's compare order, the trailer bytes -- are
// framing_parse.h's; nothing of them is restated here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "checksum_args.h"
#include "context.h"
#include "dict_dev.h"
#include "framing_dev.h"
#include "framing_parse.h"
#include "gf2.h"
#include "inflate_dev.h"

extern "C" size_t zng_rocm_deflate_quick_bound(size_t source_len);
extern "C" int zng_rocm_deflate_quick_dev(const zng_rocm_stream_job *jobs, size_t njobs, uint32_t *d_results, void *stream);
extern "C" int zng_rocm_checksums_dev(int which, const zng_rocm_check_job *jobs, size_t njobs, uint32_t *d_out2, void *stream);

namespace zr {

constexpr uint32_t kWrapHead = 12;                       // both wrapped formats (see above)

struct FrameJob {
    uint8_t *out;
    uint64_t in_len;
};

// has_dict: the 16-byte head with FDICT and `dictid` (zlib; dict_plan.h) in place of the 12-byte one
__global__ __launch_bounds__(256)
void frame_compress_kernel(const FrameJob *__restrict__ jobs, uint32_t njobs, int format, uint32_t dictid, int has_dict,
                           const uint32_t *__restrict__ quick, const uint32_t *__restrict__ checks, uint32_t *__restrict__ results) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= njobs) return;
    uint8_t *out = jobs[i].out;
    const uint32_t clen = quick[2 * i], adler = quick[2 * i + 1];
    if (format == 0) {
        results[2 * i] = clen;
        results[2 * i + 1] = adler;                      // of the plaintext alone: a dictionary is in no check value
        return;
    }
    static const uint8_t zhead[12] = {0x78, 0x01, 0x00, 0x00, 0x00, 0xff, 0xff, 0x00, 0x00, 0x00, 0xff, 0xff};
    // ID1 ID2 CM=8 FLG=FEXTRA MTIME=0 XFL=4 (fastest, deflate.c:913-914) OS=3 (Unix) XLEN=0
    static const uint8_t ghead[12] = {0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x04, 0x03, 0x00, 0x00};
    if (has_dict) dict_put_header(out, dictid);
    else for (int k = 0; k < 12; ++k) out[k] = format == 1 ? zhead[k] : ghead[k];
    const uint32_t head = has_dict ? kDictWrapHead : kWrapHead, tail = wrapper_tail_bytes(format);
    const uint32_t check = format == 1 ? adler : checks[2 * i + 1];
    uint8_t *t = out + head + clen;
    for (uint32_t k = 0; k < tail; ++k) t[k] = wrapper_trailer_byte(format, k, check, (uint32_t)jobs[i].in_len);
    results[2 * i] = head + clen + tail;
    results[2 * i + 1] = check;
}

// ---- uncompress side ---------------------------------------------------------------------------------------------------
// without a dictionary: wrapper_parse_whole's verdict per member.  has_dict (raw and zlib): format 0 -- every job decodes with
// the W bytes of the window as history; format 1 -- dict_parse_header's verdict: FDICT with `dictid` gives the history, with
// another id kDictMismatch, and FDICT clear no history
__global__ __launch_bounds__(256)
void parse_header_kernel(const InflateJobDev *__restrict__ given, uint32_t njobs, int format, uint32_t dictid, uint32_t W,
                         int has_dict, const DeviceTables *__restrict__ tabs, InflateJobDev *__restrict__ patched,
                         uint32_t *__restrict__ head /* 2 per job: header bytes, verdict */) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= njobs) return;
    const InflateJobDev j = given[i];
    DictHeader h = {0u, kMsgNone, has_dict ? 1u : 0u};
    if (has_dict) {
        if (format == 1) h = dict_parse_header(j.in, j.in_len, dictid);
    } else {
        const WholeHead w = wrapper_parse_whole(format, LaneBytes{j.in}, j.in_len, tabs->byte_tab);
        h.pos = (uint32_t)w.header_len;
        h.msg = w.msg;
    }
    InflateJobDev p = j;
    p.dict_len = h.history ? W : 0u;
    if (h.msg != kMsgNone) {                             // nothing to decode: an empty job costs the inflater nothing
        p.in_len = 0;
        p.out_cap = 0;
    } else {
        p.in = j.in + h.pos;
        p.in_len = j.in_len - h.pos;
    }
    patched[i] = p;
    head[2 * i] = h.pos;
    head[2 * i + 1] = h.msg;
}

// the checksum descriptors of the inflated streams, as checksum.hip's host code builds them -- but from lengths that
// only exist on the device
__global__ __launch_bounds__(256)
void fill_check_args_kernel(const InflateJobDev *__restrict__ jobs, const uint32_t *__restrict__ inflated, uint32_t njobs,
                            const DeviceTables *__restrict__ tabs, int do_adler, int do_crc, StreamArgs *__restrict__ sa,
                            FinalArgs *__restrict__ fa) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= njobs) return;
    const uint64_t len = (int32_t)inflated[4 * i + 2] == 1 ? inflated[4 * i] : 0u;
    fill_check_descriptor(jobs[i].out, len, tabs, do_adler, do_crc, sa + i, fa + i);
}

// (kDictMismatch is a verdict of dict_parse_header alone: without a dictionary no head row carries it)
__global__ __launch_bounds__(256)
void verify_trailer_kernel(const InflateJobDev *__restrict__ given, const uint32_t *__restrict__ head,
                           const uint32_t *__restrict__ checks, uint32_t njobs, int format, uint32_t *__restrict__ results) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= njobs) return;
    uint32_t out_len = results[4 * i], used = results[4 * i + 1], status = results[4 * i + 2], msg = results[4 * i + 3];
    const uint32_t hdr = head[2 * i], hmsg = head[2 * i + 1];
    if (hmsg == kDictMismatch) {                         // Z_DATA_ERROR without a text (inflate.c:1247-1249), the DICTID consumed
        out_len = 0;
        used = hdr;
        msg = kMsgNone;
        status = (uint32_t)-3;
    } else if (hmsg != kMsgNone) {
        out_len = 0;
        used = 0;
        msg = hmsg;
        status = hmsg == kMsgStarved ? (uint32_t)-5 : (uint32_t)-3;
    } else if ((int32_t)status == 1) {
        const uint32_t tail = wrapper_tail_bytes(format);
        const uint64_t at = (uint64_t)hdr + used;
        if (at + tail > given[i].in_len) {               // the stream ends before its trailer
            status = (uint32_t)-5;
            msg = kMsgStarved;
            used = (uint32_t)given[i].in_len;
        } else {
            const uint32_t adler = format == 1 ? checks[2 * i] : 0u, crc = format == 2 ? checks[2 * i + 1] : 0u;
            const uint32_t verdict = wrapper_trailer_verdict(format, given[i].in + at, adler, crc, out_len);
            if (verdict != kWrapNone) { status = (uint32_t)-3; msg = wrapper_inflate_msg(verdict); }
            used = (uint32_t)(at + tail);
        }
    } else {
        used += hdr;
    }
    results[4 * i] = out_len;
    results[4 * i + 1] = used;
    results[4 * i + 2] = status;
    results[4 * i + 3] = msg;
}

// ---- the host bodies: one for the two compress calls, one for the two uncompress calls; dict = null: the plain call ---------
static size_t frame_bound(size_t source_len, int format, bool has_dict) {
    const uint32_t head = has_dict ? kDictWrapHead : kWrapHead;
    return zng_rocm_deflate_quick_bound(source_len) + (format ? head + wrapper_tail_bytes(format) + 4 : 0);
}

static int compress_streams_body(int format, const zng_rocm_dict *dict, const zng_rocm_stream_job *jobs, size_t njobs,
                                 uint32_t *d_results, hipStream_t st) {
    DeviceGuard dev;
    Workspace *ws = workspace_for(st);
    if (!ws) return ZNG_ROCM_ENOMEM;
    const uint32_t head = format ? (dict ? kDictWrapHead : kWrapHead) : 0u, tail = wrapper_tail_bytes(format);
    uint32_t *d_quick = nullptr, *d_checks = nullptr;
    FrameJob *d_fj = nullptr, *h_fj = nullptr;
    std::vector<zng_rocm_stream_job> inner(njobs);
    std::vector<zng_rocm_check_job> cj(format == 2 ? njobs : 0);
    {
        std::lock_guard<std::mutex> use(ws->mu);
        if (int rc = scratch_reserve(ws, kScrFrameWords, njobs * 4 * sizeof(uint32_t), false, (void **)&d_quick)) return rc;
        d_checks = d_quick + 2 * njobs;
        if (int rc = scratch_reserve(ws, kScrFrameJobs, njobs * sizeof(FrameJob), false, (void **)&d_fj)) return rc;
        if (int rc = host_tables_acquire(ws)) return rc;
        if (int rc = scratch_reserve(ws, kScrFrameJobsHost, njobs * sizeof(FrameJob), true, (void **)&h_fj)) return rc;
        for (size_t i = 0; i < njobs; ++i) {
            const zng_rocm_stream_job &j = jobs[i];
            const bool fits = j.out && !((uintptr_t)j.out & 3) && j.out_cap >= frame_bound(j.in_len, format, dict != nullptr);
            const bool taken = dict ? (!j.in_len || j.in) && !j.dict_len && !(format && j.flags) &&
                                          !(j.flags & ~(uint32_t)(ZNG_ROCM_BLOCK_NOT_FINAL | ZNG_ROCM_BLOCK_SYNC_FLUSH))
                                    : !(format && (j.dict_len || j.flags));
            if (!fits || !taken) {
                set_error(dict ? "job %zu: out must be 4-byte aligned with out_cap >= zng_rocm_compress_streams_dict_bound(); the job's "
                                 "dict_len must be 0 (the history is the dictionary object's) and a zlib stream takes no block flags"
                               : "job %zu: out must be 4-byte aligned with out_cap >= zng_rocm_compress_streams_bound(); a wrapped "
                                 "stream takes neither a dictionary nor block flags", i);
                return ZNG_ROCM_EINVAL;
            }
            inner[i] = j;
            inner[i].out = (uint8_t *)j.out + head;
            inner[i].out_cap = j.out_cap - head - tail;
            h_fj[i] = FrameJob{(uint8_t *)j.out, j.in_len};
            if (format == 2) cj[i] = zng_rocm_check_job{j.in, j.in_len, 1u, 0u};
        }
        ZR_HIP(hipMemcpyAsync(d_fj, h_fj, njobs * sizeof(FrameJob), hipMemcpyHostToDevice, st));
        if (int rc = host_tables_release(ws, st)) return rc;
    }
    // the passes take the stream's workspace themselves
    if (int rc = dict ? launch_deflate_quick_dict(inner.data(), njobs, d_quick, dict, st)
                      : zng_rocm_deflate_quick_dev(inner.data(), njobs, d_quick, st))
        return rc;
    if (format == 2)
        if (int rc = zng_rocm_checksums_dev(2, cj.data(), njobs, d_checks, st)) return rc;
    hipLaunchKernelGGL(frame_compress_kernel, dim3((unsigned)((njobs + 255) / 256)), dim3(256), 0, st, d_fj, (uint32_t)njobs,
                       format, dict ? dict->id : 0u, dict ? 1 : 0, d_quick, d_checks, d_results);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

// the two halves of the uncompress pipeline over tables that already sit in device memory (framing_dev.h): the header pass,
// and everything behind it -- what zng_rocm_uncompress_packed_dev (inflate_sizes.hip) runs on a table the device patched --
// and, behind them, the one place that puts a caller's jobs there (upload_given_jobs)
int launch_parse_header(int format, const zng_rocm_dict *dict, const InflateJobDev *d_given, size_t njobs, InflateJobDev *d_patched,
                        uint32_t *d_head, hipStream_t st) {
    if (!njobs) return ZNG_ROCM_OK;
    const dim3 grid((unsigned)((njobs + 255) / 256)), block(256);
    hipLaunchKernelGGL(parse_header_kernel, grid, block, 0, st, d_given, (uint32_t)njobs, format, dict ? dict->id : 0u,
                       dict ? dict->window : 0u, dict ? 1 : 0, ctx()->tables, d_patched, d_head);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

int uncompress_patched_device(int format, const zng_rocm_dict *dict, const InflateJobDev *d_given, const InflateJobDev *d_patched,
                              const uint32_t *d_head, uint32_t *d_checks, uint8_t *d_msg, Partial *d_part, size_t njobs,
                              uint32_t *d_results, hipStream_t st) {
    if (!njobs) return ZNG_ROCM_OK;
    Context *c = ctx();
    const dim3 grid((unsigned)((njobs + 255) / 256)), block(256);
    if (int rc = dict ? launch_inflate_streams_dict_device(d_patched, njobs, d_results, dict->d_window + dict->window, st)
                      : launch_inflate_streams_device(d_patched, njobs, d_results, st))
        return rc;
    if (format) {
        StreamArgs *d_sa = reinterpret_cast<StreamArgs *>(d_msg);
        FinalArgs *d_fa = reinterpret_cast<FinalArgs *>(d_msg + njobs * sizeof(StreamArgs));
        const bool adler = format == 1, crc = format == 2;
        hipLaunchKernelGGL(fill_check_args_kernel, grid, block, 0, st, d_patched, d_results, (uint32_t)njobs, c->tables,
                           adler ? 1 : 0, crc ? 1 : 0, d_sa, d_fa);
        ZR_HIP(hipGetLastError());
        if (int rc = launch_checksum_batch_device(adler, crc, d_sa, d_fa, d_part, njobs, d_checks, st)) return rc;
    }
    hipLaunchKernelGGL(verify_trailer_kernel, grid, block, 0, st, d_given, d_head, d_checks, (uint32_t)njobs, format, d_results);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

int upload_given_jobs(Workspace *ws, int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                      bool with_out, bool checks, GivenJobs *g, hipStream_t st) {
    InflateJobDev *h_given = nullptr;
    *g = GivenJobs{};
    if (int rc = scratch_reserve(ws, kScrInflateDevJobs, 2 * njobs * sizeof(InflateJobDev), false, (void **)&g->d_given)) return rc;
    g->d_patched = g->d_given + njobs;
    // head rows: 2 words per job; the check values: 2 more
    if (int rc = scratch_reserve(ws, kScrFrameWords, njobs * (checks ? 4 : 2) * sizeof(uint32_t), false, (void **)&g->d_head)) return rc;
    if (checks) {
        g->d_checks = g->d_head + 2 * njobs;
        if (int rc = scratch_reserve(ws, kScrCheckMessages, njobs * (sizeof(StreamArgs) + sizeof(FinalArgs)), false, (void **)&g->d_msg)) return rc;
        if (int rc = scratch_reserve(ws, kScrCheckPartials, njobs * sizeof(Partial), false, (void **)&g->d_part)) return rc;
    }
    if (int rc = host_tables_acquire(ws)) return rc;
    if (int rc = scratch_reserve(ws, kScrInflateDevJobsHost, njobs * sizeof(InflateJobDev), true, (void **)&h_given)) return rc;
    for (size_t i = 0; i < njobs; ++i) {
        const zng_rocm_inflate_dev_job &j = jobs[i];
        if (!with_out) {
            h_given[i] = InflateJobDev{(const uint8_t *)j.in, nullptr, j.in_len, 0u, j.dict_len, 0u};
            continue;
        }
        if ((j.in_len && !j.in) || (j.out_cap && !j.out) || j.in_len > 0x7fffffffull || j.out_cap > 0x7fffffffull ||
            j.dict_len || j.flags) {
            set_error(dict ? "job %zu: null buffer, a stream or output of 2 GiB and more, or dict_len / flags (the history is the "
                             "dictionary object's)"
                           : "job %zu: null buffer, a stream or output of 2 GiB and more, or dict_len / flags (raw streams only: "
                             "zng_rocm_inflate_streams_dev)", i);
            return ZNG_ROCM_EINVAL;
        }
        h_given[i] = InflateJobDev{(const uint8_t *)j.in, (uint8_t *)j.out, j.in_len, j.out_cap, 0u, 0u};
    }
    ZR_HIP(hipMemcpyAsync(g->d_given, h_given, njobs * sizeof(InflateJobDev), hipMemcpyHostToDevice, st));
    if (int rc = host_tables_release(ws, st)) return rc;
    return launch_parse_header(format, dict, g->d_given, njobs, g->d_patched, g->d_head, st);
}

static int uncompress_streams_body(int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                                   uint32_t *d_results, hipStream_t st) {
    DeviceGuard dev;
    Workspace *ws = workspace_for(st);
    if (!ws) return ZNG_ROCM_ENOMEM;
    std::lock_guard<std::mutex> use(ws->mu);
    GivenJobs g;
    if (int rc = upload_given_jobs(ws, format, dict, jobs, njobs, true, true, &g, st)) return rc;
    return uncompress_patched_device(format, dict, g.d_given, g.d_patched, g.d_head, g.d_checks, g.d_msg, g.d_part, njobs, d_results, st);
}

}  // namespace zr

using namespace zr;

extern "C" {

size_t zng_rocm_compress_streams_bound(size_t source_len, int format) { return frame_bound(source_len, format, false); }

int zng_rocm_compress_streams_dev(int format, const zng_rocm_stream_job *jobs, size_t njobs, uint32_t *d_results, void *stream) {
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    if (!njobs) return ZNG_ROCM_OK;
    if (!jobs || !d_results || format < 0 || format > 2 || njobs > 0x7fffffffull) return ZNG_ROCM_EINVAL;
    return compress_streams_body(format, nullptr, jobs, njobs, d_results, (hipStream_t)stream);
}

int zng_rocm_uncompress_streams_dev(int format, const zng_rocm_inflate_dev_job *jobs, size_t njobs, uint32_t *d_results,
                                    void *stream) {
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    if (!njobs) return ZNG_ROCM_OK;
    if (!jobs || !d_results || format < 0 || format > 2 || njobs > 0x7fffffffull) return ZNG_ROCM_EINVAL;
    return uncompress_streams_body(format, nullptr, jobs, njobs, d_results, (hipStream_t)stream);
}

size_t zng_rocm_compress_streams_dict_bound(size_t source_len, int format) {
    if (format != 0 && format != 1) return 0;
    return frame_bound(source_len, format, true);
}

int zng_rocm_compress_streams_dict_dev(int format, const zng_rocm_dict *dict, const zng_rocm_stream_job *jobs, size_t njobs,
                                       uint32_t *d_results, void *stream) {
    if (int rc = dict_usable(dict)) return rc;
    if (!dict || format < 0 || format > 1) {
        set_error("a dictionary object and format 0 (raw) or 1 (zlib): gzip has no preset dictionary");
        return ZNG_ROCM_EINVAL;
    }
    if (!njobs) return ZNG_ROCM_OK;
    if (!jobs || !d_results || njobs > 0x7fffffffull) return ZNG_ROCM_EINVAL;
    return compress_streams_body(format, dict, jobs, njobs, d_results, (hipStream_t)stream);
}

int zng_rocm_uncompress_streams_dict_dev(int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs,
                                         size_t njobs, uint32_t *d_results, void *stream) {
    if (int rc = dict_usable(dict)) return rc;
    if (!dict || format < 0 || format > 1) {
        set_error("a dictionary object and format 0 (raw) or 1 (zlib): gzip has no preset dictionary");
        return ZNG_ROCM_EINVAL;
    }
    if (!njobs) return ZNG_ROCM_OK;
    if (!jobs || !d_results || njobs > 0x7fffffffull) return ZNG_ROCM_EINVAL;
    return uncompress_streams_body(format, dict, jobs, njobs, d_results, (hipStream_t)stream);
}

}  // extern "C"
