// bgzf.hip -- zng_rocm_bgzf_compress_dev: device-resident plaintext written as a BGZF file (SAM specification 4.1; what
// bgzip, BAM and tabix read and zng_rocm_gunzip_members_dev decodes), every step on the device.  The plaintext is cut into
// pieces of at most 65280 bytes; piece i becomes member i: 18 bytes of header with the member's own size in it (BSIZE), the
// piece deflated with no history, CRC-32 and length.  The members stand one behind the other at byte granularity and the
// 28-byte end-of-file block closes the file.  The host steps are bgzf_plan.h; per round of at most round_bytes of plaintext:
//
//   CRC-32 of every piece          the many-message pass of zng_rocm_checksums_dev (one workgroup per piece), its descriptors
//                                  filled on the device by bgzf_check_args_kernel from (base, piece size, count): the host
//                                  builds no table of 392 bytes per piece
//   the payloads                   levels 1..9: the rows engine (deflate_dyn.hip) over the pieces as independent streams; its
//                                  blocks stay in their slots (deflate_blocks.h), nothing is packed per stream
//                                  ZNG_ROCM_BGZF_QUICK: zng_rocm_deflate_quick_dev into one scratch buffer per piece
//                                  level 0: none
//   bgzf_scan_kernel               one workgroup: the engines' lengths -> stored or not (bgzf_member) -> member sizes -> an
//                                  exclusive scan in tiles of 1024 on top of the file offset the round before left on the
//                                  device -> every member's place, its row of the members table, the stored count
//   bgzf_frame_kernel              every header, every trailer, and every payload to its byte in the file: a rows block from
//                                  its slot (one trip through HBM for the compressed bytes), a QUICK payload from its scratch
//                                  buffer, a stored member's bytes from the plaintext behind 01 LEN NLEN
//   bgzf_eof_kernel                behind the last round: the end-of-file block and its row
//
// Nothing is stored at or behind d_dst + dst_cap: every store of the two writing kernels is clamped, so a file that does not
// fit is cut at the buffer's end while the scan goes on counting -- the call then reports the size the file needs.
#include "checksum_args.h"
#include "context.h"

#include "bgzf_copy.h"
#include "bgzf_plan.h"
#include "deflate_blocks.h"
#include "deflate_dev.h"

#include <mutex>
#include <vector>

extern "C" size_t zng_rocm_deflate_quick_bound(size_t source_len);
extern "C" int zng_rocm_deflate_quick_dev(const zng_rocm_stream_job *jobs, size_t njobs, uint32_t *d_results, void *stream);

namespace zr {

struct BgzfState {                      // carried on the device from round to round
    unsigned long long file_off;        // bytes of the file so far
    unsigned long long stored;          // members written through the stored fallback
    unsigned long long members;         // members so far
    unsigned long long overflow;        // 1: the file has passed dst_cap
};

constexpr uint32_t kBgzfStoredBit = 0x80000000u;      // in BgzfRound::payload

struct BgzfRound {                      // the arguments both kernels of a round share
    const uint8_t *src;                 // the whole plaintext
    uint8_t       *dst;
    unsigned long long src_len, dst_cap;
    unsigned long long first;           // index of the round's first piece
    uint32_t       np, piece;           // pieces of the round, bytes per piece
    const uint32_t *crc2;               // {-, crc} per piece
    unsigned long long *member_off;     // per piece: where its member begins in the file
    uint32_t      *payload;             // per piece: payload bytes | kBgzfStoredBit
};

// the checksum descriptors of the round's pieces, as zng_rocm_checksums_dev's host code builds them
__global__ __launch_bounds__(256)
void bgzf_check_args_kernel(BgzfRound r, const DeviceTables *__restrict__ tabs, StreamArgs *__restrict__ sa, FinalArgs *__restrict__ fa) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r.np) return;
    const unsigned long long g = r.first + i;
    fill_check_descriptor(r.src + g * r.piece, bgzf_piece_len(r.src_len, r.piece, g), tabs, 0, 1, sa + i, fa + i);
}

// the engine's length of piece i: kind 0 = none (level 0), 1 = u32 at stride 2 (QUICK's results), 2 = u64 at stride 2 (rows)
__device__ __forceinline__ uint32_t bgzf_clen(const void *lens, int kind, uint32_t i) {
    if (kind == 1) return static_cast<const uint32_t *>(lens)[2 * i];
    if (kind == 2) {
        const unsigned long long v = static_cast<const unsigned long long *>(lens)[2 * i];
        return v > 0xfffffffeull ? 0xfffffffeu : (uint32_t)v;
    }
    return kBgzfForceStored;
}

__global__ __launch_bounds__(1024)
void bgzf_scan_kernel(BgzfRound r, const void *__restrict__ lens, int kind, BgzfState *__restrict__ state,
                      zng_rocm_gzip_member *__restrict__ rows, unsigned long long rows_cap) {
    __shared__ unsigned long long wave_sum[16];
    __shared__ unsigned long long carry;
    __shared__ uint32_t nstored;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) {
        carry = state->file_off;
        nstored = 0;
    }
    __syncthreads();
    uint32_t mine_stored = 0;
    for (uint32_t base = 0; base < r.np; base += 1024u) {
        const uint32_t i = base + (uint32_t)t;
        const bool live = i < r.np;
        uint32_t n = 0;
        BgzfMember m = {0u, 0u};
        if (live) {
            n = bgzf_piece_len(r.src_len, r.piece, r.first + i);
            m = bgzf_member(n, bgzf_clen(lens, kind, i));
        }
        const unsigned long long v = live ? bgzf_member_bytes(m) : 0ull;
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
            const unsigned long long off = before + incl - v;
            r.member_off[i] = off;
            r.payload[i] = m.payload | (m.stored ? kBgzfStoredBit : 0u);
            mine_stored += m.stored;
            const unsigned long long g = r.first + i;
            if (g < rows_cap) {
                zng_rocm_gzip_member row;
                row.src_off = off;
                row.src_len = v;
                row.dst_off = g * r.piece;
                row.out_len = n;
                row.crc = r.crc2[2 * i + 1];
                row.bgzf = 1u;
                rows[g] = row;
            }
        }
        __syncthreads();
        if (t == 1023) carry = before + incl;
        __syncthreads();
    }
    if (mine_stored) atomicAdd(&nstored, mine_stored);
    __syncthreads();
    if (t == 0) {
        state->file_off = carry;
        state->stored += nstored;
        state->members += r.np;
        if (carry > r.dst_cap) state->overflow = 1;
    }
}

__device__ __forceinline__ void bgzf_put(uint8_t *dst, unsigned long long at, unsigned long long cap, uint8_t v) {
    if (at < cap) dst[at] = v;
}

// Work item w < np is member w of the round: header, trailer, and the payload unless it lies in the rows engine's slots;
// work item np + k is block k of the rows engine.  qbuf / qstride: QUICK's buffer per piece, or null.
__global__ __launch_bounds__(256)
void bgzf_frame_kernel(BgzfRound r, const uint8_t *__restrict__ qbuf, unsigned long long qstride, const BlkJob *__restrict__ blk,
                       const uint32_t *__restrict__ seg_len, const unsigned long long *__restrict__ in_stream, uint32_t nblk) {
    const int t = threadIdx.x;
    const unsigned long long items = (unsigned long long)r.np + nblk;
    for (unsigned long long w = blockIdx.x; w < items; w += gridDim.x) {
        if (w < r.np) {
            const uint32_t i = (uint32_t)w;
            const unsigned long long off = r.member_off[i];
            const uint32_t pl = r.payload[i] & ~kBgzfStoredBit;
            const bool stored = (r.payload[i] & kBgzfStoredBit) != 0;
            const unsigned long long g = r.first + i;
            const uint32_t n = bgzf_piece_len(r.src_len, r.piece, g);
            if (t < (int)kBgzfHead) bgzf_put(r.dst, off + t, r.dst_cap, bgzf_header_byte((uint32_t)t, kBgzfHead + pl + kBgzfTail));
            else if (t >= 32 && t < 32 + (int)kBgzfTail)
                bgzf_put(r.dst, off + kBgzfHead + pl + (t - 32), r.dst_cap, bgzf_trailer_byte((uint32_t)t - 32u, r.crc2[2 * i + 1], n));
            else if (stored && t >= 64 && t < 64 + (int)kBgzfStoredHead)
                bgzf_put(r.dst, off + kBgzfHead + (t - 64), r.dst_cap, bgzf_stored_byte((uint32_t)t - 64u, n));
            if (stored) bgzf_copy(r.dst, off + kBgzfHead + kBgzfStoredHead, r.dst_cap, r.src + g * r.piece, n, t);
            else if (qbuf) bgzf_copy(r.dst, off + kBgzfHead, r.dst_cap, qbuf + i * qstride, pl, t);
        } else {
            const uint32_t k = (uint32_t)(w - r.np);
            const uint32_t s = blk[k].stream & 0x7fffffffu;
            if (r.payload[s] & kBgzfStoredBit) continue;
            bgzf_copy(r.dst, r.member_off[s] + kBgzfHead + in_stream[k], r.dst_cap, blk[k].out, seg_len[k], t);
        }
    }
}

__global__ __launch_bounds__(64)
void bgzf_eof_kernel(uint8_t *__restrict__ dst, unsigned long long dst_cap, unsigned long long src_len, BgzfState *__restrict__ state,
                     zng_rocm_gzip_member *__restrict__ rows, unsigned long long rows_cap) {
    const uint32_t t = threadIdx.x;
    const unsigned long long off = state->file_off, g = state->members;
    if (t < kBgzfEofBytes) bgzf_put(dst, off + t, dst_cap, bgzf_eof_byte(t));
    __syncthreads();                                     // every lane has read the state
    if (t == 0) {
        if (g < rows_cap) {
            zng_rocm_gzip_member row;
            row.src_off = off;
            row.src_len = kBgzfEofBytes;
            row.dst_off = src_len;
            row.out_len = 0;
            row.crc = 0;
            row.bgzf = 1u;
            rows[g] = row;
        }
        state->file_off = off + kBgzfEofBytes;
        state->members = g + 1;
        if (off + kBgzfEofBytes > dst_cap) state->overflow = 1;
    }
}

static thread_local int t_bgzf_rounds = 0, t_bgzf_stored = 0;

}  // namespace zr

using namespace zr;

extern "C" {

size_t zng_rocm_bgzf_bound(size_t src_len, uint32_t block_bytes) { return (size_t)bgzf_bound(src_len, block_bytes); }

int zng_rocm_bgzf_last_rounds(void) { return t_bgzf_rounds; }
int zng_rocm_bgzf_last_stored(void) { return t_bgzf_stored; }

int zng_rocm_bgzf_compress_dev(int level, const uint8_t *d_src, size_t src_len, uint32_t block_bytes, uint8_t *d_dst, size_t dst_cap,
                               uint64_t *out_len, zng_rocm_gzip_member *members, size_t members_cap, size_t *nmembers,
                               size_t round_bytes, uint32_t flags, void *stream) {
    if (out_len) *out_len = 0;
    if (nmembers) *nmembers = 0;
    t_bgzf_rounds = t_bgzf_stored = 0;
    if (!bgzf_args_ok(level, d_src, src_len, block_bytes, d_dst, dst_cap, out_len, members, members_cap, nmembers, flags)) {
        set_error("zng_rocm_bgzf_compress_dev: level outside -1..9, ZNG_ROCM_BGZF_QUICK at a level other than 1, unknown flags, "
                  "block_bytes above 65280, or a null pointer");
        return ZNG_ROCM_EINVAL;
    }
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    const bool eof = (flags & kBgzfNoEof) == 0, quick = (flags & kBgzfQuick) != 0;
    if (!src_len && !eof) return ZNG_ROCM_OK;
    level = bgzf_level(level);
    const uint32_t piece = bgzf_piece_bytes(block_bytes);
    const uint64_t np_all = bgzf_pieces(src_len, piece), per = bgzf_round_pieces(round_bytes, piece);
    const uint64_t np_max = np_all < per ? np_all : per;
    if (np_max > 0x3fffffffull) {
        set_error("zng_rocm_bgzf_compress_dev: more than 2^30 members in one round; give a smaller round_bytes");
        return ZNG_ROCM_EINVAL;
    }
    const uint64_t rows_cap = members_cap < np_all + (eof ? 1 : 0) ? members_cap : np_all + (eof ? 1 : 0);
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard dev;
    Workspace *ws = workspace_for(st);
    if (!ws) return ZNG_ROCM_ENOMEM;

    // device: state | rows | member_off | {-, crc} | payload | QUICK's results | QUICK's buffers (every part 16-byte aligned)
    const size_t qstride = quick ? zng_rocm_deflate_quick_bound(piece) : 0;
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t o_rows = up16(sizeof(BgzfState)), o_off = o_rows + up16(rows_cap * sizeof(zng_rocm_gzip_member)),
                 o_crc = o_off + up16(np_max * sizeof(unsigned long long)), o_pay = o_crc + up16(np_max * 2 * sizeof(uint32_t)),
                 o_qres = o_pay + up16(np_max * sizeof(uint32_t)), o_qbuf = o_qres + up16(quick ? np_max * 2 * sizeof(uint32_t) : 0),
                 total = o_qbuf + np_max * qstride;
    uint8_t *d = nullptr, *d_msg = nullptr;
    Partial *d_part = nullptr;
    BgzfState *h_state = nullptr;
    {
        std::lock_guard<std::mutex> use(ws->mu);
        if (int rc = scratch_reserve(ws, kScrBgzf, total, false, (void **)&d)) return rc;
        if (int rc = scratch_reserve(ws, kScrCheckMessages, np_max * (sizeof(StreamArgs) + sizeof(FinalArgs)), false, (void **)&d_msg)) return rc;
        if (int rc = scratch_reserve(ws, kScrCheckPartials, np_max * sizeof(Partial), false, (void **)&d_part)) return rc;
        if (int rc = scratch_reserve(ws, kScrBgzfHost, sizeof(BgzfState), true, (void **)&h_state)) return rc;
    }
    BgzfState *d_state = reinterpret_cast<BgzfState *>(d);
    zng_rocm_gzip_member *d_rows = reinterpret_cast<zng_rocm_gzip_member *>(d + o_rows);
    uint32_t *d_crc = reinterpret_cast<uint32_t *>(d + o_crc), *d_qres = reinterpret_cast<uint32_t *>(d + o_qres);
    ZR_HIP(hipMemsetAsync(d_state, 0, sizeof(BgzfState), st));

    StreamArgs *d_sa = reinterpret_cast<StreamArgs *>(d_msg);
    FinalArgs *d_fa = reinterpret_cast<FinalArgs *>(d_msg + np_max * sizeof(StreamArgs));
    std::vector<zng_rocm_stream_job> sj;
    int rounds = 0;
    for (uint64_t first = 0; first < np_all; first += per, ++rounds) {
        const uint32_t np = (uint32_t)(np_all - first < per ? np_all - first : per);
        BgzfRound r;
        r.src = d_src;
        r.dst = d_dst;
        r.src_len = src_len;
        r.dst_cap = dst_cap;
        r.first = first;
        r.np = np;
        r.piece = piece;
        r.crc2 = d_crc;
        r.member_off = reinterpret_cast<unsigned long long *>(d + o_off);
        r.payload = reinterpret_cast<uint32_t *>(d + o_pay);
        hipLaunchKernelGGL(bgzf_check_args_kernel, dim3((np + 255u) / 256u), dim3(256), 0, st, r, ctx()->tables, d_sa, d_fa);
        ZR_HIP(hipGetLastError());
        if (int rc = launch_checksum_batch_device(false, true, d_sa, d_fa, d_part, np, d_crc, st)) return rc;
        const void *lens = nullptr;
        int kind = 0;
        RowsBlocks blocks = {nullptr, nullptr, nullptr, nullptr, 0};
        if (level > 0) {
            sj.resize(np);
            for (uint32_t i = 0; i < np; ++i) {
                sj[i].in = d_src + (first + i) * piece;
                sj[i].in_len = bgzf_piece_len(src_len, piece, first + i);
                sj[i].out = quick ? d + o_qbuf + i * qstride : nullptr;
                sj[i].out_cap = (uint32_t)qstride;
                sj[i].dict_len = 0;
                sj[i].flags = 0;
            }
            if (quick) {
                if (int rc = zng_rocm_deflate_quick_dev(sj.data(), np, d_qres, st)) return rc;
                lens = d_qres;
                kind = 1;
            } else {
                std::lock_guard<std::mutex> use(ws->mu);
                // every piece is short enough for one segment
                const RowsRequest rq = {level, 0, kWinBitsMax, sj.data(), np, kSegBytesMin, nullptr, nullptr, kRowsOutKeep, nullptr};
                RowsDone done;
                if (int rc = deflate_rows_enqueue(rq, ws, st, &done)) return rc;
                blocks = done.blocks;
                lens = blocks.sizes;
                kind = 2;
            }
        }
        hipLaunchKernelGGL(bgzf_scan_kernel, dim3(1), dim3(1024), 0, st, r, lens, kind, d_state, d_rows, (unsigned long long)rows_cap);
        ZR_HIP(hipGetLastError());
        const uint64_t items = (uint64_t)np + blocks.nblk;
        const unsigned grid = (unsigned)(items < (1u << 20) ? items : (1u << 20));
        hipLaunchKernelGGL(bgzf_frame_kernel, dim3(grid), dim3(256), 0, st, r, quick ? d + o_qbuf : nullptr, (unsigned long long)qstride,
                           blocks.blk, blocks.seg_len, blocks.in_stream, (uint32_t)blocks.nblk);
        ZR_HIP(hipGetLastError());
    }
    if (eof) {
        hipLaunchKernelGGL(bgzf_eof_kernel, dim3(1), dim3(64), 0, st, d_dst, (unsigned long long)dst_cap, (unsigned long long)src_len,
                           d_state, d_rows, (unsigned long long)rows_cap);
        ZR_HIP(hipGetLastError());
    }
    // one synchronisation for the whole call: the state comes down, and the rows when the caller asked for any
    ZR_HIP(hipMemcpyAsync(h_state, d_state, sizeof(BgzfState), hipMemcpyDeviceToHost, st));
    if (rows_cap) ZR_HIP(hipMemcpyAsync(members, d_rows, rows_cap * sizeof(zng_rocm_gzip_member), hipMemcpyDeviceToHost, st));
    ZR_HIP(hipStreamSynchronize(st));
    t_bgzf_rounds = rounds;
    t_bgzf_stored = (int)h_state->stored;
    *out_len = h_state->file_off;
    *nmembers = (size_t)h_state->members;
    if (h_state->overflow) {
        set_error("the BGZF file needs %llu bytes, dst_cap is %llu", h_state->file_off, (unsigned long long)dst_cap);
        return -5;
    }
    return ZNG_ROCM_OK;
}

}  // extern "C"
