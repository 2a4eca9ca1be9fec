// compress_streams.hip -- zng_rocm_compress_streams2_dev and zng_rocm_compress_members_dev: many device-resident streams
// deflated at any level (0..9) and strategy and wrapped as raw / zlib / gzip members with the canonical headers of deflate.c,
// every member in its job's own buffer (streams2) or all of them back to back in one destination (members: the `cat a.gz b.gz`
// file zng_rocm_gunzip_members_dev reads).  Every step is enqueued on the caller's stream; nothing comes back to the host.  The
// host rules are compress_streams_plan.h; the job table of the whole call goes up once, then per round of at most round_bytes
// of plaintext:
//
//   the check value of every job   the many-message pass of zng_rocm_checksums_dev (one workgroup per job; Adler-32, gzip:
//                                  CRC-32), its descriptors filled on the device by cs_check_args_kernel from the job table
//   the deflate data               levels 1..9: the rows engine (deflate_dyn.hip) over all segments of the round's jobs, its
//                                  blocks left in their slots (deflate_blocks.h); level 0: none
//   cs_scan_kernel                 one workgroup: header + stream size (the engine's, or the closed form of the stored blocks)
//                                  + trailer = member size; streams2: the result words; members: an exclusive scan in tiles of
//                                  1024 on top of the file offset the round before left on the device -> d_offsets, d_checks
//   cs_frame_kernel                work items are the members, then the blocks.  A member item writes header, trailer and the
//                                  level-0 sync marker; a block item moves one block of the engine from its slot -- or, at
//                                  level 0, writes one stored block's header and moves its 65535 bytes from the plaintext -- to
//                                  its byte in the member (bgzf_copy.h: 16-byte stores, byte steps at head and tail)
//
// Every store of the frame kernel is bounded by the member's capacity: out_cap, or dst_cap for the file, which is cut at the
// buffer's end while the scan goes on counting, so d_offsets[njobs] is the size the file needs.
//
// zng_rocm_compress_streams2_dict_dev / zng_rocm_compress_members_dict_dev are the same calls with one shared preset dictionary
// (dict.hip) as every stream's history: the rows engine runs its dictionary form (lz_rows_dict_kernel), and the zlib member
// begins with the 6-byte FDICT header -- CMF FLG, the DICTID -- instead of the 2-byte one.
//
// zng_rocm_compress_streams2_header_dev / zng_rocm_compress_members_header_dev are the gzip calls with deflateSetHeader's fields
// per member (gzip_header_plan.h): the host renders every header into one pinned blob that goes up behind the job table in the
// same copy, the scan adds each job's own header length, and the frame kernel moves the header from the blob (bgzf_copy.h) instead
// of computing its 10 bytes.  The kernels are templates over that: the calls without headers run the instructions they always had.
#include "checksum_args.h"
#include "context.h"

#include "bgzf_copy.h"
#include "compress_streams_plan.h"
#include "deflate_blocks.h"
#include "deflate_dev.h"
#include "deflate_window_plan.h"
#include "dict_dev.h"
#include "gzip_header_plan.h"

#include <mutex>
#include <vector>

namespace zr {

struct CsJob {                          // one row per job of the whole call
    const uint8_t *in;
    uint8_t       *out;                 // streams2: the member's buffer
    uint32_t       in_len, out_cap, flags;
    uint32_t       head_len;            // the *_header_dev calls: bytes of the member's rendered header (else 0, not read)
    unsigned long long blk0;            // level 0: stored blocks of the jobs in front of this one
    unsigned long long head_off;        // ... and where it begins in CsRound::blob
};

struct CsRound {                        // the arguments the kernels of a round share
    const CsJob   *jobs;                // the whole call's table
    uint8_t       *dst;                 // members: the file
    unsigned long long dst_cap;
    unsigned long long first;           // index of the round's first job
    uint32_t       nj;                  // jobs of the round
    int            format, level, strategy;
    int            members;             // 1: one destination, 0: per-job buffers
    const uint32_t *check2;             // per job of the round: {Adler-32, CRC-32}, the one the format uses filled
    const unsigned long long *sizes;    // levels 1..9: the engine's {stream size, -} per job of the round
    unsigned long long *offsets;        // members: d_offsets
    uint32_t      *checks;              // members: d_checks or null
    uint32_t      *results;             // streams2: d_results
    uint32_t       dict, dictid;        // 1: the calls with a shared preset dictionary, whose zlib header carries FDICT and this DICTID
    int            window_bits;         // the stream's w_bits (deflate_window_plan.h): 15 but for the *_window_dev calls
    const uint8_t *blob;                // the *_header_dev calls: every member's rendered header, else null
};

// bytes of the member's header, and byte k of it
__device__ __forceinline__ uint32_t cs_round_head(const CsRound &r) { return r.dict ? cs_dict_head_bytes(r.format) : cs_head_bytes(r.format); }
__device__ __forceinline__ uint8_t cs_round_header_byte(const CsRound &r, uint32_t k) {
    return r.dict ? cs_dict_header_byte(r.level, r.strategy, r.dictid, k) : cs_header_byte(r.format, r.level, r.strategy, k, r.window_bits);
}

// kHeads (the *_header_dev calls): the job's own header, whose bytes are in the blob
template <bool kHeads>
__device__ __forceinline__ uint32_t cs_job_head(const CsRound &r, const CsJob &j) {
    return kHeads ? j.head_len : cs_round_head(r);
}

__device__ __forceinline__ uint32_t cs_check_of(const CsRound &r, uint32_t i) { return r.check2[2 * i + (r.format == 2 ? 1 : 0)]; }

// bytes of deflate data of job i of the round
__device__ __forceinline__ unsigned long long cs_stream_bytes(const CsRound &r, uint32_t i, const CsJob &j) {
    return r.level ? r.sizes[2 * i] : cs_stored_bytes(j.in_len, j.flags);
}

// where job g's member goes: base, first byte, and the byte no store may reach
struct CsPlace {
    uint8_t *base;
    unsigned long long at, cap;
};
__device__ __forceinline__ CsPlace cs_place(const CsRound &r, unsigned long long g, const CsJob &j) {
    CsPlace p;
    p.base = r.members ? r.dst : j.out;
    p.at = r.members ? r.offsets[g] : 0ull;
    p.cap = r.members ? r.dst_cap : (unsigned long long)j.out_cap;
    return p;
}

// the checksum descriptors of the round's jobs, as zng_rocm_checksums_dev's host code builds them
__global__ __launch_bounds__(256)
void cs_check_args_kernel(CsRound r, const DeviceTables *__restrict__ tabs, StreamArgs *__restrict__ sa, FinalArgs *__restrict__ fa) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r.nj) return;
    const CsJob j = r.jobs[r.first + i];
    fill_check_descriptor(j.in, j.in_len, tabs, r.format == 2 ? 0 : 1, r.format == 2 ? 1 : 0, sa + i, fa + i);
}

template <bool kHeads>
__global__ __launch_bounds__(1024)
void cs_scan_kernel(CsRound r, unsigned long long *__restrict__ file_off) {
    __shared__ unsigned long long wave_sum[16];
    __shared__ unsigned long long carry;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t tail = cs_tail_bytes(r.format);
    if (!r.members) {                                    // every member in its own buffer: nothing to place
        for (uint32_t i = (uint32_t)t; i < r.nj; i += 1024u) {
            const unsigned long long g = r.first + i;
            const CsJob j = r.jobs[g];
            r.results[2 * g] = (uint32_t)(cs_stream_bytes(r, i, j) + cs_job_head<kHeads>(r, j) + tail);
            r.results[2 * g + 1] = cs_check_of(r, i);
        }
        return;
    }
    if (t == 0) carry = *file_off;
    __syncthreads();
    for (uint32_t base = 0; base < r.nj; base += 1024u) {
        const uint32_t i = base + (uint32_t)t;
        const bool live = i < r.nj;
        unsigned long long v = 0ull;
        if (live) {
            const CsJob j = r.jobs[r.first + i];
            v = cs_stream_bytes(r, i, j) + cs_job_head<kHeads>(r, j) + tail;
        }
        unsigned long long incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long up = (unsigned long long)__shfl_up((long long)incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        unsigned long long before = carry;
        for (int w = 0; w < wave; ++w) before += wave_sum[w];
        if (live) {
            r.offsets[r.first + i] = before + incl - v;
            if (r.checks) r.checks[r.first + i] = cs_check_of(r, i);
        }
        __syncthreads();
        if (t == 1023) carry = before + incl;
        __syncthreads();
    }
    if (t == 0) {
        *file_off = carry;
        r.offsets[r.first + r.nj] = carry;               // the next round's first member; behind the last round the file's length
    }
}

__device__ __forceinline__ void cs_put(const CsPlace &p, unsigned long long at, uint8_t v) {
    if (at < p.cap) p.base[at] = v;
}

// Work item w < nj is member w of the round; work item nj + k is block k: of the rows engine (blk / seg_len / in_stream), or at
// level 0 stored block jobs[first].blk0 + k of the call.
template <bool kHeads>
__global__ __launch_bounds__(256)
void cs_frame_kernel(CsRound r, const BlkJob *__restrict__ blk, const uint32_t *__restrict__ seg_len,
                     const unsigned long long *__restrict__ in_stream, unsigned long long nblk) {
    const int t = threadIdx.x;
    const uint32_t tail = cs_tail_bytes(r.format);
    const unsigned long long items = (unsigned long long)r.nj + nblk;
    for (unsigned long long w = blockIdx.x; w < items; w += gridDim.x) {
        if (w < r.nj) {
            const uint32_t i = (uint32_t)w;
            const unsigned long long g = r.first + i;
            const CsJob j = r.jobs[g];
            const CsPlace p = cs_place(r, g, j);
            const unsigned long long body = cs_stream_bytes(r, i, j);
            const uint32_t head = cs_job_head<kHeads>(r, j);
            if (kHeads) bgzf_copy(p.base, p.at, p.cap, r.blob + j.head_off, head, t);       // up to kGhMaxBytes: a loop
            if (!kHeads && t < (int)head) cs_put(p, p.at + t, cs_round_header_byte(r, (uint32_t)t));
            else if (t >= 32 && t < 32 + (int)tail)
                cs_put(p, p.at + head + body + (t - 32), cs_trailer_byte(r.format, (uint32_t)t - 32u, cs_check_of(r, i), j.in_len));
            else if (r.level == 0 && cs_stored_marker(j.flags) && t >= 64 && t < 64 + (int)kCsStoredHead)
                cs_put(p, p.at + head + body - kCsStoredHead + (t - 64), cs_stored_byte((uint32_t)t - 64u, 0u, false));
        } else if (r.level) {
            const unsigned long long k = w - r.nj;
            const uint32_t s = blk[k].stream & 0x7fffffffu;
            const unsigned long long g = r.first + s;
            const CsJob j = r.jobs[g];
            const CsPlace p = cs_place(r, g, j);
            bgzf_copy(p.base, p.at + cs_job_head<kHeads>(r, j) + in_stream[k], p.cap, blk[k].out, seg_len[k], t);
        } else {
            // the job that holds this stored block: the last one of the round whose blk0 is not behind it
            const unsigned long long b_call = r.jobs[r.first].blk0 + (w - r.nj);
            uint32_t lo = 0, hi = r.nj - 1u;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo + 1u) / 2u;
                if (r.jobs[r.first + mid].blk0 <= b_call) lo = mid;
                else hi = mid - 1u;
            }
            const unsigned long long g = r.first + lo;
            const CsJob j = r.jobs[g];
            const CsPlace p = cs_place(r, g, j);
            const unsigned long long b = b_call - j.blk0;
            const uint32_t len = cs_stored_block_len(j.in_len, b);
            const bool final_block = b + 1u == cs_stored_blocks(j.in_len) && !(j.flags & ZNG_ROCM_BLOCK_NOT_FINAL);
            const unsigned long long at = p.at + cs_job_head<kHeads>(r, j) + b * (kCsMaxStored + kCsStoredHead);
            if (t < (int)kCsStoredHead) cs_put(p, at + t, cs_stored_byte((uint32_t)t, len, final_block));
            bgzf_copy(p.base, at + kCsStoredHead, p.cap, j.in + b * kCsMaxStored, len, t);
        }
    }
}

static thread_local int t_cs_rounds = 0;

// with_dict: the calls with a shared preset dictionary (`dict` is every stream's history), else dict is null.  window_bits: as
// the caller gave it (deflate_window_plan.h); the calls without a window say 15.  heads: the *_header_dev calls (format 2), one
// header per job, else null
static int compress_streams_run(const char *who, bool members, int format, int level, int strategy, const zng_rocm_stream_job *jobs,
                                size_t njobs, uint8_t *d_dst, size_t dst_cap, size_t round_bytes, uint64_t *d_offsets,
                                uint32_t *d_checks, uint32_t *d_results, void *stream, bool with_dict = false,
                                const zng_rocm_dict *dict = nullptr, int window_bits = kWinBitsMax,
                                const zng_rocm_gzip_header *heads = nullptr) {
    t_cs_rounds = 0;
    if (cs_format_ok(format) && win_check(format, window_bits)) {
        set_error("%s: window_bits %d is outside 9..15 (8: the zlib format alone, deflate.c:319)", who, window_bits);
        return ZNG_ROCM_EINVAL;
    }
    window_bits = cs_format_ok(format) ? win_effective(format, window_bits) : kWinBitsMax;
    const void *res = members ? (const void *)d_offsets : (const void *)d_results;
    int rc = with_dict ? cs_dict_call_check(format, level, strategy, dict, jobs, njobs, res)
                       : cs_call_check(format, level, strategy, jobs, njobs, res);
    if (!rc && members) rc = cs_file_check(d_dst, dst_cap);
    if (rc) {
        if (with_dict)
            set_error("%s: no dictionary object, format outside 0..1 (gzip has no preset dictionary), level outside -1..9, strategy "
                      "other than 0, 1 or 4, or a null pointer", who);
        else set_error("%s: format outside 0..2, level outside -1..9, strategy outside 0..4, or a null pointer", who);
        return rc;
    }
    uint64_t bad = 0;
    if ((rc = with_dict ? cs_dict_jobs_check(format, jobs, njobs, !members, &bad) : cs_jobs_check(format, jobs, njobs, !members, &bad))) {
        if (rc == kCsBufError)
            set_error("%s: job %llu: out_cap below zng_rocm_compress_streams2%s_bound()", who, (unsigned long long)bad, with_dict ? "_dict" : "");
        else if (with_dict)
            set_error("%s: job %llu: null buffer, a dict_len of its own, unknown flags, flags in a wrapped format, or a bound that "
                      "does not fit 32 bits", who, (unsigned long long)bad);
        else
            set_error("%s: job %llu: null buffer, dict_len above 32768, unknown flags, dict_len or flags in a wrapped format, or a "
                      "bound that does not fit 32 bits", who, (unsigned long long)bad);
        return rc;
    }
    // the *_header_dev calls: every header's lengths, the first refusal in job order
    std::vector<GhLens> lens(heads ? njobs : 0);
    size_t blob_bytes = 0;
    for (size_t i = 0; heads && i < njobs; ++i) {
        if (gh_check(&heads[i], &lens[i])) {
            set_error("%s: header %zu: extra_len above 65535 or without extra, a name or comment of more than 65535 bytes, or reserved "
                      "not 0", who, i);
            return ZNG_ROCM_EINVAL;
        }
        const uint64_t bound = cs_bound(jobs[i].in_len, format) - cs_head_bytes(format) + gh_bytes(&heads[i], lens[i]);
        if (!members && bound > 0xffffffffull) {
            set_error("%s: job %zu: a bound that does not fit 32 bits", who, i);
            return ZNG_ROCM_EINVAL;
        }
        if (!members && jobs[i].out_cap < bound) {
            set_error("%s: job %zu: out_cap below zng_rocm_compress_streams2_bound() - 10 + zng_rocm_gzip_header_bytes()", who, i);
            return kCsBufError;
        }
        blob_bytes += gh_bytes(&heads[i], lens[i]);
    }
    if (!njobs) return ZNG_ROCM_OK;
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    if (with_dict)
        if ((rc = dict_usable(dict))) return rc;
    level = cs_level(level);
    size_t total_in = 0, np_max = 0;
    for (size_t first = 0; first < njobs;) {
        const size_t last = (size_t)cs_round_end(jobs, njobs, first, round_bytes);
        if (last - first > np_max) np_max = last - first;
        first = last;
    }
    for (size_t i = 0; i < njobs; ++i) total_in += jobs[i].in_len;
    if (np_max > 0x3fffffffull) {
        set_error("%s: more than 2^30 jobs in one round; give a smaller round_bytes", who);
        return ZNG_ROCM_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard dev;
    Workspace *ws = workspace_for(st);
    if (!ws) return ZNG_ROCM_ENOMEM;
    std::lock_guard<std::mutex> use(ws->mu);

    // device: file offset | job table | the *_header_dev calls: the rendered headers | {Adler-32, CRC-32} per job of a round
    // (every part 16-byte aligned); pinned: job table | headers, as they stand on the device: one copy takes both up
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t tab_bytes = njobs * sizeof(CsJob), o_jobs = 16, o_blob = o_jobs + up16(tab_bytes), o_chk = o_blob + up16(blob_bytes);
    const size_t total = o_chk + np_max * 2 * sizeof(uint32_t), up_bytes = heads ? up16(tab_bytes) + blob_bytes : tab_bytes;
    uint8_t *d = nullptr, *d_msg = nullptr;
    Partial *d_part = nullptr;
    CsJob *h_jobs = nullptr;
    if ((rc = scratch_reserve(ws, kScrCompressStreams, total, false, (void **)&d))) return rc;
    if ((rc = scratch_reserve(ws, kScrCompressStreamsHost, up_bytes, true, (void **)&h_jobs))) return rc;
    if ((rc = scratch_reserve(ws, kScrCheckMessages, np_max * (sizeof(StreamArgs) + sizeof(FinalArgs)), false, (void **)&d_msg))) return rc;
    if ((rc = scratch_reserve(ws, kScrCheckPartials, np_max * sizeof(Partial), false, (void **)&d_part))) return rc;
    unsigned long long *d_file_off = reinterpret_cast<unsigned long long *>(d);
    CsJob *d_jobs = reinterpret_cast<CsJob *>(d + o_jobs);
    uint32_t *d_chk = reinterpret_cast<uint32_t *>(d + o_chk);
    StreamArgs *d_sa = reinterpret_cast<StreamArgs *>(d_msg);
    FinalArgs *d_fa = reinterpret_cast<FinalArgs *>(d_msg + np_max * sizeof(StreamArgs));

    if ((rc = host_tables_acquire(ws))) return rc;
    unsigned long long blk0 = 0;
    for (size_t i = 0; i < njobs; ++i) {
        h_jobs[i].in = jobs[i].in;
        h_jobs[i].out = jobs[i].out;
        h_jobs[i].in_len = jobs[i].in_len;
        h_jobs[i].out_cap = jobs[i].out_cap;
        h_jobs[i].flags = jobs[i].flags;
        h_jobs[i].head_len = 0;
        h_jobs[i].blk0 = blk0;
        h_jobs[i].head_off = 0;
        blk0 += cs_stored_blocks(jobs[i].in_len);
    }
    uint8_t *h_blob = reinterpret_cast<uint8_t *>(h_jobs) + up16(tab_bytes);
    for (size_t i = 0, at = 0; heads && i < njobs; ++i) {
        gh_render(&heads[i], lens[i], level, strategy, h_blob + at);
        h_jobs[i].head_len = gh_bytes(&heads[i], lens[i]);
        h_jobs[i].head_off = at;
        at += h_jobs[i].head_len;
    }
    ZR_HIP(hipMemcpyAsync(d_jobs, h_jobs, up_bytes, hipMemcpyHostToDevice, st));
    // the engine records the event that guards the pinned tables behind its own copy, later on this stream; without it, here
    if (level == 0 && (rc = host_tables_release(ws, st))) return rc;
    if (members) ZR_HIP(hipMemsetAsync(d_file_off, 0, sizeof(unsigned long long), st));

    const uint32_t seg_bytes = level ? deflate_rows_segment_bytes(total_in) : 0u;
    int rounds = 0;
    for (size_t first = 0; first < njobs; ++rounds) {
        const size_t last = (size_t)cs_round_end(jobs, njobs, first, round_bytes);
        CsRound r;
        r.jobs = d_jobs;
        r.dst = d_dst;
        r.dst_cap = dst_cap;
        r.first = first;
        r.nj = (uint32_t)(last - first);
        r.format = format;
        r.level = level;
        r.strategy = strategy;
        r.members = members ? 1 : 0;
        r.check2 = d_chk;
        r.sizes = nullptr;
        r.offsets = reinterpret_cast<unsigned long long *>(d_offsets);
        r.checks = d_checks;
        r.results = d_results;
        r.dict = with_dict ? 1u : 0u;
        r.dictid = with_dict ? dict->id : 0u;
        r.window_bits = window_bits;
        r.blob = heads ? d + o_blob : nullptr;
        hipLaunchKernelGGL(cs_check_args_kernel, dim3((r.nj + 255u) / 256u), dim3(256), 0, st, r, ctx()->tables, d_sa, d_fa);
        ZR_HIP(hipGetLastError());
        if ((rc = launch_checksum_batch_device(format != 2, format == 2, d_sa, d_fa, d_part, r.nj, d_chk, st))) return rc;
        RowsBlocks blocks = {nullptr, nullptr, nullptr, nullptr, 0};
        unsigned long long nblk = h_jobs[last - 1].blk0 + cs_stored_blocks(jobs[last - 1].in_len) - h_jobs[first].blk0;
        if (level) {
            const RowsRequest rq = {level, strategy, window_bits, jobs + first, r.nj, seg_bytes, nullptr, with_dict ? dict : nullptr,
                                    kRowsOutKeep, nullptr};
            RowsDone done;
            if ((rc = deflate_rows_enqueue(rq, ws, st, &done))) {
                (void)host_tables_release(ws, st);
                return rc;
            }
            blocks = done.blocks;
            r.sizes = blocks.sizes;
            nblk = blocks.nblk;
        }
        if (heads) hipLaunchKernelGGL(cs_scan_kernel<true>, dim3(1), dim3(1024), 0, st, r, d_file_off);
        else hipLaunchKernelGGL(cs_scan_kernel<false>, dim3(1), dim3(1024), 0, st, r, d_file_off);
        ZR_HIP(hipGetLastError());
        const unsigned long long items = (unsigned long long)r.nj + nblk;
        const unsigned grid = (unsigned)(items < (1u << 20) ? items : (1u << 20));
        if (heads)
            ZR_LAUNCH_TRACED(cs_frame_kernel<true>, dim3(grid), dim3(256), st, r, blocks.blk, blocks.seg_len, blocks.in_stream, nblk);
        else
            ZR_LAUNCH_TRACED(cs_frame_kernel<false>, dim3(grid), dim3(256), st, r, blocks.blk, blocks.seg_len, blocks.in_stream, nblk);
        ZR_HIP(hipGetLastError());
        first = last;
    }
    t_cs_rounds = rounds;
    return ZNG_ROCM_OK;
}

}  // namespace zr

using namespace zr;

extern "C" {

size_t zng_rocm_compress_streams2_bound(size_t source_len, int format) { return (size_t)cs_bound(source_len, format); }

int zng_rocm_compress_streams2_last_rounds(void) { return t_cs_rounds; }

int zng_rocm_compress_streams2_dev(int format, int level, int strategy, const zng_rocm_stream_job *jobs, size_t njobs,
                                   size_t round_bytes, uint32_t *d_results, void *stream) {
    return compress_streams_run("zng_rocm_compress_streams2_dev", false, format, level, strategy, jobs, njobs, nullptr, 0, round_bytes,
                                nullptr, nullptr, d_results, stream);
}

int zng_rocm_compress_members_dev(int format, int level, int strategy, const zng_rocm_stream_job *jobs, size_t njobs, uint8_t *d_dst,
                                  size_t dst_cap, size_t round_bytes, uint64_t *d_offsets, uint32_t *d_checks, void *stream) {
    return compress_streams_run("zng_rocm_compress_members_dev", true, format, level, strategy, jobs, njobs, d_dst, dst_cap,
                                round_bytes, d_offsets, d_checks, nullptr, stream);
}

// The two calls above at deflateInit2's windowBits (deflate_window_plan.h): levels 1..9 run the window form of the matcher unless
// window_bits is 15, the zlib header carries CINFO = w - 8
int zng_rocm_compress_streams2_window_dev(int format, int level, int strategy, int window_bits, const zng_rocm_stream_job *jobs,
                                          size_t njobs, size_t round_bytes, uint32_t *d_results, void *stream) {
    return compress_streams_run("zng_rocm_compress_streams2_window_dev", false, format, level, strategy, jobs, njobs, nullptr, 0,
                                round_bytes, nullptr, nullptr, d_results, stream, false, nullptr, window_bits);
}

int zng_rocm_compress_members_window_dev(int format, int level, int strategy, int window_bits, const zng_rocm_stream_job *jobs,
                                         size_t njobs, uint8_t *d_dst, size_t dst_cap, size_t round_bytes, uint64_t *d_offsets,
                                         uint32_t *d_checks, void *stream) {
    return compress_streams_run("zng_rocm_compress_members_window_dev", true, format, level, strategy, jobs, njobs, d_dst, dst_cap,
                                round_bytes, d_offsets, d_checks, nullptr, stream, false, nullptr, window_bits);
}

// The gzip calls above with deflateSetHeader's fields per member (deflate.c:922-1023; gzip_header_plan.h); heads == NULL: those calls
int zng_rocm_compress_streams2_header_dev(int level, int strategy, int window_bits, const zng_rocm_stream_job *jobs,
                                          const zng_rocm_gzip_header *heads, size_t njobs, size_t round_bytes, uint32_t *d_results,
                                          void *stream) {
    return compress_streams_run("zng_rocm_compress_streams2_header_dev", false, 2, level, strategy, jobs, njobs, nullptr, 0, round_bytes,
                                nullptr, nullptr, d_results, stream, false, nullptr, window_bits, heads);
}

int zng_rocm_compress_members_header_dev(int level, int strategy, int window_bits, const zng_rocm_stream_job *jobs,
                                         const zng_rocm_gzip_header *heads, size_t njobs, uint8_t *d_dst, size_t dst_cap,
                                         size_t round_bytes, uint64_t *d_offsets, uint32_t *d_checks, void *stream) {
    return compress_streams_run("zng_rocm_compress_members_header_dev", true, 2, level, strategy, jobs, njobs, d_dst, dst_cap,
                                round_bytes, d_offsets, d_checks, nullptr, stream, false, nullptr, window_bits, heads);
}

size_t zng_rocm_compress_streams2_dict_bound(size_t source_len, int format) { return (size_t)cs_dict_bound(source_len, format); }

int zng_rocm_compress_streams2_dict_dev(int format, int level, int strategy, const zng_rocm_dict *dict, const zng_rocm_stream_job *jobs,
                                        size_t njobs, size_t round_bytes, uint32_t *d_results, void *stream) {
    return compress_streams_run("zng_rocm_compress_streams2_dict_dev", false, format, level, strategy, jobs, njobs, nullptr, 0,
                                round_bytes, nullptr, nullptr, d_results, stream, true, dict);
}

int zng_rocm_compress_members_dict_dev(int format, int level, int strategy, const zng_rocm_dict *dict, const zng_rocm_stream_job *jobs,
                                       size_t njobs, uint8_t *d_dst, size_t dst_cap, size_t round_bytes, uint64_t *d_offsets,
                                       uint32_t *d_checks, void *stream) {
    return compress_streams_run("zng_rocm_compress_members_dict_dev", true, format, level, strategy, jobs, njobs, d_dst, dst_cap,
                                round_bytes, d_offsets, d_checks, nullptr, stream, true, dict);
}

}  // extern "C"
