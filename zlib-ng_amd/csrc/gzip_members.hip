// gzip_members.hip -- every member of a gzip file that sits in device memory, BGZF included: what gzread does with a file of
// several members (gz_look gzread.c.in:81-154 starts a new member whenever 1f 8b follows a finished one and ignores anything
// else as trailing garbage; gz_decomp :161-207 runs inflate() on each) for a file that is all in memory.
//   scan     one pass over the file, full grid, aligned 16-byte loads: bit p of a bitmap is set iff src[p .. p + 3] is
//            1f 8b 08 F with F & 0xe0 == 0; per tile of 16 KiB a popcount
//   offsets  one workgroup turns the tiles' counts into offsets (exclusive scan) and the total
//   -> the total comes down (four bytes: it sizes the tables and the header kernel's grid)
//   scatter  the set bits become the sorted list of candidate positions and the header kernel's jobs
//   headers  framing_large.hip's kernels on every candidate (one wavefront each, wrapper_parse_rules, FHCRC), unchanged
//   link     one lane per candidate: BSIZE from a BGZF 'BC' subfield (framing_parse.h), next(i) (gzip_members_plan.h), the
//            eight bytes in front of the guessed end
//   -> ONE readback of the candidate table, 40 bytes per candidate
//   (a candidate's header is shown at most 4 KiB, and more than 2^24 candidates are not tabled: gzip_members_plan.h)
//   plan     gzip_members_plan.h: the chain from candidate 0, members below 128 KiB to zng_rocm_uncompress_streams_dev in one
//            launch, the others to zng_rocm_uncompress_large_streams_dev, each with exactly its guessed output; every
//            result verified in order; the first member that refutes its guess is decoded alone
//            (zng_rocm_uncompress_large_dev) and the plan rebuilt from where it really ended
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "context.h"
#include "framing_large.h"
#include "framing_parse.h"
#include "gzip_members_dev.h"
#include "gzip_members_plan.h"

namespace zr {

constexpr uint32_t kScanThreads = 256;
constexpr uint32_t kScanUnroll = 4;                      // 16-byte lines per thread and tile: four loads in flight
constexpr uint32_t kTileLines = kScanThreads * kScanUnroll;   // a tile: 16 KiB of the file

// sum over the workgroup's 256 threads, the same in every thread; `red`: 4 words of LDS
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *red) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();                                     // (the last use of red is over)
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// exclusive prefix of v over the workgroup's 256 threads; *total = the sum
__device__ __forceinline__ uint32_t block_prefix(uint32_t v, uint32_t *red, uint32_t *total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc += up;
    }
    __syncthreads();
    if (lane == 63u) red[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) before += w < wave ? red[w] : 0u;
    *total = red[0] + red[1] + red[2] + red[3];
    return before + inc - v;
}

// Bit k of bitmap[L] says that the byte at (src rounded down to 16) + 16 L + k begins a candidate.  The first and the last
// line reach up to 15 bytes outside the file inside their own 16-byte line (read, never used -- as the header kernel and the
// checksum kernels read around an unaligned buffer; include/zng_rocm.h says so to callers).
__global__ __launch_bounds__(256)
void members_scan_kernel(const uint8_t *__restrict__ src, uint64_t src_len, uint16_t *__restrict__ bitmap,
                         uint32_t *__restrict__ tile_count, uint32_t ntiles) {
    __shared__ uint32_t red[4];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uintptr_t base = (uintptr_t)src & ~(uintptr_t)15;
    const uint64_t head = (uintptr_t)src - base, nlines = (head + src_len + 15) >> 4;
    const uint64_t last = head + src_len - 4;            // the last byte (counted from base) a candidate may begin on
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        uint4 v[kScanUnroll];
        uint32_t nx[kScanUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kScanUnroll; ++u) {
            const uint64_t line = (uint64_t)tile * kTileLines + u * kScanThreads + t;
            v[u] = line < nlines ? *reinterpret_cast<const uint4 *>(base + line * 16) : make_uint4(0u, 0u, 0u, 0u);
            // the three bytes behind my line: the first word of my neighbour's, which the wavefront's last lane fetches itself
            nx[u] = lane == 63u && line + 1 < nlines ? *reinterpret_cast<const uint32_t *>(base + (line + 1) * 16) : 0u;
        }
        uint32_t count = 0;
#pragma unroll
        for (uint32_t u = 0; u < kScanUnroll; ++u) {
            const uint64_t line = (uint64_t)tile * kTileLines + u * kScanThreads + t;
            const uint32_t down = __shfl_down(v[u].x, 1, 64);
            const uint32_t w[5] = {v[u].x, v[u].y, v[u].z, v[u].w, lane == 63u ? nx[u] : down};
            uint32_t mask = 0;
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                const uint32_t sh = 8u * (k & 3u);
                const uint32_t four = sh ? (w[k >> 2] >> sh) | (w[(k >> 2) + 1] << (32u - sh)) : w[k >> 2];
                mask |= member_candidate(four) ? 1u << k : 0u;
            }
            if (mask) {                                  // (rare) only bytes of the file, and four of them
                const uint64_t at = line * 16;
#pragma unroll
                for (uint32_t k = 0; k < 16; ++k)
                    if (at + k < head || at + k > last) mask &= ~(1u << k);
            }
            if (line < nlines) bitmap[line] = (uint16_t)mask;
            count += __popc(mask);
        }
        const uint32_t sum = block_sum(count, red);
        if (t == 0) tile_count[tile] = sum;
    }
}

// one workgroup: tile_off[i] = candidates in front of tile i, tile_off[ntiles] = all of them -- or kMembersTooMany when they are
// more than kMembersMaxCandidates (the offsets, 32 bits wide, are then not used: no table is built)
__global__ __launch_bounds__(256)
void members_offsets_kernel(const uint32_t *__restrict__ tile_count, uint32_t ntiles, uint32_t *__restrict__ tile_off) {
    __shared__ uint32_t red[4];
    const uint32_t t = threadIdx.x;
    uint64_t running = 0;                                // (up to 2^31 tiles of up to 4096 candidates)
    for (uint32_t at = 0; at < ntiles; at += kScanThreads) {     // (uniform trip count: the barriers inside are reached by all)
        const uint32_t c = at + t < ntiles ? tile_count[at + t] : 0u;
        uint32_t total;
        const uint32_t before = block_prefix(c, red, &total);
        if (at + t < ntiles) tile_off[at + t] = (uint32_t)running + before;
        running += total;
    }
    if (t == 0) tile_off[ntiles] = running > kMembersMaxCandidates ? kMembersTooMany : (uint32_t)running;
}

// the set bits in order: pos[r] = the r-th candidate's position in the file, jobs[r] = the bytes from there on that a header
// may take (member_header_look)
__global__ __launch_bounds__(256)
void members_scatter_kernel(const uint8_t *__restrict__ src, uint64_t src_len, const uint16_t *__restrict__ bitmap,
                            const uint32_t *__restrict__ tile_off, uint32_t ntiles, uint64_t *__restrict__ pos,
                            HeadJob *__restrict__ jobs) {
    __shared__ uint32_t red[4];
    const uint32_t t = threadIdx.x;
    const uint64_t head = (uintptr_t)src & 15u, nlines = (head + src_len + 15) >> 4;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        uint32_t running = tile_off[tile];
        if (tile_off[tile + 1] == running) continue;     // (the same answer in every thread)
        for (uint32_t u = 0; u < kScanUnroll; ++u) {
            const uint64_t line = (uint64_t)tile * kTileLines + u * kScanThreads + t;
            uint32_t mask = line < nlines ? bitmap[line] : 0u;
            uint32_t total;
            uint32_t r = running + block_prefix(__popc(mask), red, &total);
            while (mask) {
                const uint32_t k = __ffs((int)mask) - 1;
                mask &= mask - 1;
                const uint64_t p = line * 16 + k - head;
                pos[r] = p;
                jobs[r] = HeadJob{src + p, member_header_look(src_len, p)};
                ++r;
            }
            running += total;
        }
    }
}

struct GlobalBytes {                                     // one lane reads the header it was given
    const uint8_t *src;
    __device__ uint32_t byte(uint64_t at) const { return src[at]; }
};

__global__ __launch_bounds__(256)
void members_link_kernel(const uint8_t *__restrict__ src, uint64_t src_len, const uint64_t *__restrict__ pos,
                         const WrapperHead *__restrict__ heads, uint32_t n, CandRow *__restrict__ rows) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const WrapperHead h = heads[i];
    const uint64_t p = pos[i];
    CandRow r = {p, h.header_len, 0u, h.status, h.msg, 0u, 0u, 0u};
    uint32_t bsize = 0;
    const bool bgzf = h.status == 0 && gzip_bgzf_bsize(GlobalBytes{src + p}, src_len - p, &bsize);
    if (bgzf) r.flags |= kCandBgzf;
    r.next = member_next(pos, n, i, bgzf, bsize, src_len);
    const uint64_t end = r.next < n ? pos[r.next] : src_len;
    if (h.status == 0 && end >= p + h.header_len + 8) {  // inflate.c:1105-1147: CRC-32 and ISIZE, least significant byte first
        const uint8_t *t = src + end - 8;
        r.crc = wrapper_le32(t);
        r.isize = wrapper_le32(t + 4);
        r.flags |= kCandTrailer;
    }
    rows[i] = r;
}

namespace {

thread_local int g_candidates = 0, g_replans = 0, g_small = 0, g_large = 0;

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

struct Call {
    const uint8_t *d_src;
    size_t src_len;
    uint8_t *d_dst;
    size_t dst_cap;
    zng_rocm_gzip_member *members;
    size_t members_cap;
    uint32_t flags;
    hipStream_t st;
    Workspace *ws;
    // progress
    uint64_t at = 0, out = 0;
    size_t nm = 0;

    void add(uint64_t src_off, uint64_t len, uint64_t out_len, uint32_t crc, uint32_t bgzf) {
        if (nm < members_cap) members[nm] = zng_rocm_gzip_member{src_off, len, out, out_len, crc, bgzf};
        ++nm;
        at = src_off + len;
        out += out_len;
    }
};

// the candidates of the file and what their headers say: scan .. link.  Two readbacks: the candidates' number (members_heads),
// then `rows`, once.  *too_many: more than kMembersMaxCandidates, no table.
int discover(Call &c, std::vector<CandRow> &rows, bool *too_many) {
    rows.clear();
    *too_many = false;
    MembersHeads m;
    if (int rc = members_heads("zng_rocm_gunzip_members_dev", c.d_src, c.src_len, sizeof(CandRow), c.st, c.ws, &m)) return rc;
    *too_many = m.too_many;
    const uint32_t n = m.n;
    if (!n) return ZNG_ROCM_OK;
    CandRow *d_rows = reinterpret_cast<CandRow *>(m.d_rows);
    hipLaunchKernelGGL(members_link_kernel, dim3((n + 255u) / 256u), dim3(256), 0, c.st, c.d_src, (uint64_t)c.src_len, m.d_pos, m.d_heads, n,
                       d_rows);
    ZR_HIP(hipGetLastError());
    ZR_HIP(hipMemcpyAsync(m.h_rows, d_rows, (size_t)n * sizeof(CandRow), hipMemcpyDeviceToHost, c.st));
    ZR_HIP(hipStreamSynchronize(c.st));
    rows.resize(n);
    memcpy(rows.data(), m.h_rows, (size_t)n * sizeof(CandRow));
    return ZNG_ROCM_OK;
}

// a few bytes of the file on the host (behind the last member; a member's verified CRC-32)
int peek(Call &c, uint64_t at, size_t n, uint8_t *out) {
    ZR_HIP(hipMemcpyAsync(out, c.d_src + at, n, hipMemcpyDeviceToHost, c.st));
    ZR_HIP(hipStreamSynchronize(c.st));
    return ZNG_ROCM_OK;
}

// The member at c.at alone, as the caller's loop decodes it today: zng_rocm_uncompress_large_dev(2, ...) at its true place
// with the capacity that is left.  *status = that call's; 1: the member is recorded.
int decode_alone(Call &c, uint32_t bgzf, int *status, uint64_t *out_len, size_t *in_used) {
    *status = zng_rocm_uncompress_large_dev(2, c.d_src + c.at, c.src_len - (size_t)c.at, nullptr, 0, c.d_dst + c.out, c.dst_cap - (size_t)c.out,
                                            out_len, in_used, 0, c.flags, c.st);
    if (*status == ZNG_ROCM_EHIP || *status == ZNG_ROCM_ENOMEM || *status == ZNG_ROCM_ENODEV) return *status;
    if (*status != 1) return ZNG_ROCM_OK;
    uint8_t t[4] = {0, 0, 0, 0};
    if (c.nm < c.members_cap)
        if (int rc = peek(c, c.at + *in_used - 8, 4, t)) return rc;
    ++g_large;
    c.add(c.at, *in_used, *out_len, wrapper_le32(t), bgzf);
    return ZNG_ROCM_OK;
}

// the planned members through the two engines; res[k] = what was said about items[k]
int run_plan(Call &c, const MembersPlan &plan, std::vector<MemberResult> &res) {
    const size_t m = plan.items.size();
    res.assign(m, MemberResult{0, 0, 0});
    std::vector<zng_rocm_inflate_dev_job> small;
    std::vector<zng_rocm_inflate_large_job> large;
    std::vector<size_t> small_of, large_of;
    for (size_t k = 0; k < m; ++k) {
        const PlannedMember &p = plan.items[k];
        if (p.engine == kEngineSmall) {
            small.push_back(zng_rocm_inflate_dev_job{c.d_src + p.src_off, c.d_dst + p.dst_off, p.span, p.out_guess, 0u, 0u});
            small_of.push_back(k);
        } else {
            large.push_back(zng_rocm_inflate_large_job{c.d_src + p.src_off, (size_t)p.span, nullptr, 0u, c.d_dst + p.dst_off,
                                                       (size_t)p.out_guess, 0, 0, 0, nullptr, 0, 0});
            large_of.push_back(k);
        }
    }
    uint32_t *d_res = nullptr, *h_res = nullptr;
    if (!small.empty()) {
        {
            std::lock_guard<std::mutex> use(c.ws->mu);
            // (the scan's slot: the bitmap has been scattered and the stream synchronised since)
            if (int rc = scratch_reserve(c.ws, kScrMembersScan, small.size() * 4 * sizeof(uint32_t), false, (void **)&d_res)) return rc;
            if (int rc = scratch_reserve(c.ws, kScrMembersHost, small.size() * 4 * sizeof(uint32_t), true, (void **)&h_res)) return rc;
        }
        if (int rc = zng_rocm_uncompress_streams_dev(2, small.data(), small.size(), d_res, c.st)) return rc;
    }
    if (!large.empty())                                  // synchronous; behind the small members' launch on the same stream
        if (int rc = zng_rocm_uncompress_large_streams_dev(2, large.data(), large.size(), 0, c.flags, c.st)) return rc;
    if (!small.empty()) {
        ZR_HIP(hipMemcpyAsync(h_res, d_res, small.size() * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, c.st));
        ZR_HIP(hipStreamSynchronize(c.st));
        for (size_t j = 0; j < small.size(); ++j)
            res[small_of[j]] = MemberResult{(int32_t)h_res[4 * j + 2], h_res[4 * j], h_res[4 * j + 1]};
    }
    for (size_t j = 0; j < large.size(); ++j) res[large_of[j]] = MemberResult{large[j].status, large[j].out_len, large[j].in_used};
    return ZNG_ROCM_OK;
}

int gunzip_members(Call &c, uint64_t *out_len, size_t *in_used, size_t *nmembers) {
    std::vector<CandRow> rows;
    bool too_many = false;
    if (int rc = discover(c, rows, &too_many)) return rc;
    const uint32_t n = (uint32_t)rows.size();                // (0 when there were too many: every member below is decoded alone)
    g_candidates = too_many ? -1 : (int)n;
    std::vector<uint64_t> pos(n);
    for (uint32_t i = 0; i < n; ++i) pos[i] = rows[i].pos;
    auto finish = [&](int status, uint64_t o, size_t u) {
        *out_len = o;
        *in_used = u;
        *nmembers = c.nm;
        return status;
    };
    MembersPlan plan;
    std::vector<MemberResult> res;
    for (bool first = true;; first = false) {
        // c.at: the file's first byte, or the end of a complete member
        const uint32_t ci = member_at(pos.data(), n, c.at);
        if (!first && ci == n) {                         // no header the rules accept begins here: garbage, or a member in trouble
            uint8_t two[2] = {0, 0};
            if (c.src_len - c.at >= 2)
                if (int rc = peek(c, c.at, 2, two)) return rc;
            if (after_member(c.at, c.src_len, two[0], two[1]) == kAfterDone) return finish(1, c.out, (size_t)c.at);
        }
        if (ci < n && g_replans < kMembersMaxReplans) {
            plan_members(rows.data(), n, c.src_len, ci, c.out, c.dst_cap, plan);
            if (!plan.items.empty()) {
                if (int rc = run_plan(c, plan, res)) return rc;
                const size_t good = first_unverified(plan, res.data());
                for (size_t k = 0; k < good; ++k) {
                    const PlannedMember &p = plan.items[k];
                    ++(p.engine == kEngineSmall ? g_small : g_large);
                    c.add(p.src_off, res[k].in_used, res[k].out_len, p.crc, p.bgzf);
                }
                if (good < plan.items.size()) {          // a wrong guess: this member alone, then a new plan from its real end
                    ++g_replans;
                    plan.bad_guess = false;
                } else if (!plan.alone) {
                    continue;                            // the chain reached the end of the file: what is behind the last member?
                }
            }
            if (plan.bad_guess) ++g_replans;             // ... as is a guess the plan itself could tell was wrong
        }
        const uint32_t at_cand = member_at(pos.data(), n, c.at);
        int status = 0;
        uint64_t o = 0;
        size_t u = 0;
        if (int rc = decode_alone(c, at_cand < n && (rows[at_cand].flags & kCandBgzf) ? 1u : 0u, &status, &o, &u)) return rc;
        if (status != 1) return finish(status, c.out + o, (size_t)c.at + u);
    }
}

}  // namespace

// scan, offsets, the candidates' number, scatter, headers (gzip_members_dev.h)
int members_heads(const char *who, const uint8_t *d_src, size_t src_len, size_t row_bytes, hipStream_t st, Workspace *ws,
                  MembersHeads *out) {
    *out = MembersHeads{0u, false, nullptr, nullptr, nullptr, nullptr};
    if (src_len < 4) return ZNG_ROCM_OK;
    Context *cx = ctx();
    const uint64_t head = (uintptr_t)d_src & 15u, nlines = (head + src_len + 15) >> 4;
    const uint64_t ntiles64 = (nlines + kTileLines - 1) / kTileLines;
    if (ntiles64 > 0x7fffffffull) {
        set_error("%s: a file of %zu bytes is more than 2^31 tiles of 16 KiB", who, src_len);
        return ZNG_ROCM_EINVAL;
    }
    const uint32_t ntiles = (uint32_t)ntiles64;
    const size_t o_count = up16(nlines * sizeof(uint16_t)), o_off = o_count + up16((size_t)ntiles * sizeof(uint32_t));
    uint8_t *d = nullptr, *h = nullptr;
    {
        std::lock_guard<std::mutex> use(ws->mu);
        if (int rc = scratch_reserve(ws, kScrMembersScan, o_off + ((size_t)ntiles + 1) * sizeof(uint32_t), false, (void **)&d)) return rc;
        if (int rc = scratch_reserve(ws, kScrMembersHost, 16, true, (void **)&h)) return rc;
    }
    uint16_t *d_bitmap = reinterpret_cast<uint16_t *>(d);
    uint32_t *d_count = reinterpret_cast<uint32_t *>(d + o_count), *d_off = reinterpret_cast<uint32_t *>(d + o_off);
    const uint32_t grid = ntiles < (uint32_t)cx->cus * 8u ? ntiles : (uint32_t)cx->cus * 8u;
    hipLaunchKernelGGL(members_scan_kernel, dim3(grid), dim3(kScanThreads), 0, st, d_src, (uint64_t)src_len, d_bitmap, d_count, ntiles);
    ZR_HIP(hipGetLastError());
    hipLaunchKernelGGL(members_offsets_kernel, dim3(1), dim3(kScanThreads), 0, st, d_count, ntiles, d_off);
    ZR_HIP(hipGetLastError());
    ZR_HIP(hipMemcpyAsync(h, d_off + ntiles, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ZR_HIP(hipStreamSynchronize(st));
    uint32_t n;
    memcpy(&n, h, sizeof n);
    if (n == kMembersTooMany) out->too_many = true;
    if (!n || out->too_many) return ZNG_ROCM_OK;
    const size_t o_jobs = up16((size_t)n * sizeof(uint64_t)), o_heads = o_jobs + up16((size_t)n * sizeof(HeadJob));
    const size_t o_rows = o_heads + up16((size_t)n * sizeof(WrapperHead)), o_work = o_rows + up16((size_t)n * row_bytes);
    uint8_t *tab = nullptr;
    {
        std::lock_guard<std::mutex> use(ws->mu);
        if (int rc = scratch_reserve(ws, kScrMembersTab, o_work + header_rows_scratch(n), false, (void **)&tab)) return rc;
        if (int rc = scratch_reserve(ws, kScrMembersHost, (size_t)n * row_bytes, true, (void **)&h)) return rc;
    }
    uint64_t *d_pos = reinterpret_cast<uint64_t *>(tab);
    HeadJob *d_jobs = reinterpret_cast<HeadJob *>(tab + o_jobs);
    WrapperHead *d_heads = reinterpret_cast<WrapperHead *>(tab + o_heads);
    hipLaunchKernelGGL(members_scatter_kernel, dim3(grid), dim3(kScanThreads), 0, st, d_src, (uint64_t)src_len, d_bitmap, d_off, ntiles,
                       d_pos, d_jobs);
    ZR_HIP(hipGetLastError());
    if (int rc = header_rows_device(2, d_jobs, n, d_heads, tab + o_work, st)) return rc;
    *out = MembersHeads{n, false, d_pos, d_heads, tab + o_rows, h};
    return ZNG_ROCM_OK;
}

}  // namespace zr

using namespace zr;

extern "C" {

int zng_rocm_gunzip_last_candidates(void) { return g_candidates; }
int zng_rocm_gunzip_last_replans(void) { return g_replans; }
int zng_rocm_gunzip_last_small(void) { return g_small; }
int zng_rocm_gunzip_last_large(void) { return g_large; }

int zng_rocm_gunzip_members_dev(const uint8_t *d_src, size_t src_len, uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, size_t *in_used,
                                zng_rocm_gzip_member *members, size_t members_cap, size_t *nmembers, uint32_t flags, void *stream) {
    g_candidates = g_replans = g_small = g_large = 0;
    if (out_len) *out_len = 0;
    if (in_used) *in_used = 0;
    if (nmembers) *nmembers = 0;
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    if (flags & ~ZNG_ROCM_INFLATE_SUBBLOCK) {
        set_error("zng_rocm_gunzip_members_dev: unknown flag bits 0x%x", flags & ~ZNG_ROCM_INFLATE_SUBBLOCK);
        return ZNG_ROCM_EINVAL;
    }
    if ((!d_src && src_len) || (!d_dst && dst_cap) || (!members && members_cap) || !out_len || !in_used || !nmembers) {
        set_error("zng_rocm_gunzip_members_dev: a null buffer with a length, or a null result pointer");
        return ZNG_ROCM_EINVAL;
    }
    DeviceGuard dev;
    Call c = {d_src, src_len, d_dst, dst_cap, members, members_cap, flags, (hipStream_t)stream, workspace_for((hipStream_t)stream)};
    if (!c.ws) return ZNG_ROCM_ENOMEM;
    return gunzip_members(c, out_len, in_used, nmembers);
}

}  // extern "C"
