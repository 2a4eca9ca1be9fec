// inflate_sizes.hip -- the read side of zng_rocm_compress_members_dev: many device-resident raw / zlib / gzip streams whose
// plaintext lengths nobody handed over.
//   zng_rocm_inflate_sizes_dev       one small kernel parses every header (framing_dev.hip: parse_header_kernel) -> the SIZING
//                                    kernel walks every payload and adds up what it would produce: the row the decode would
//                                    write with all the room there is, without the comparison of the check value and ISIZE
//   zng_rocm_uncompress_packed_dev   the same two kernels, the rows to scratch -> one workgroup turns the sizes into places (a
//                                    tiled scan over any njobs) -> one small kernel patches out / out_cap of the device job table
//                                    -> the existing engine, check-value pass and verify_trailer_kernel decode that table
//                                    (framing_dev.hip: uncompress_patched_device) -> one small kernel writes the final rows
// Nothing crosses PCIe between the kernels and nothing synchronises: the lengths only ever exist on the device.
//
// The sizing kernel is the stream kernel of inflate_dev.hip with everything taken out that moves a byte: one wavefront per
// stream and a symbol loop that adds a literal's 1 and a match's length to a count.  What comes in front of the symbol loop is
// the decoder's own text, included here as it is there: the 64-word fetch and bit buffer (inflate_bits_body.h), the fixed
// tables and the dynamic block header (inflate_block_tables_body.h), the table builder and the packed LDS layout
// (inflate_tables.h) -- so the same bits are consumed in front of every header fault by construction.  The loop still decodes
// every distance -- for its bits, and for "invalid distance too far back" against count + history length -- but has no window,
// no ring, no copy and no store: the history's LENGTH is all it knows of the history.  Every verdict, message and count of
// consumed bytes of the loop is the decoder's (inflate_streams_body.h), the truncation rule of kBadWide included: the two are
// held against each other stream by stream in tests/test_gpu_inflate_sizes.py.  The rules on top -- argument checks,
// saturation, the member's row, places, fit, final rows -- are inflate_sizes_plan.h's, for host and device alike.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "context.h"
#include "dict_dev.h"
#include "framing_dev.h"
#include "inflate_dev.h"
#include "inflate_sizes_plan.h"
#include "inflate_tables.h"

namespace zr {

__device__ __forceinline__ IsRow load_row(const uint32_t *rows, uint32_t i) {
    return IsRow{rows[4 * i], rows[4 * i + 1], rows[4 * i + 2], rows[4 * i + 3]};
}
__device__ __forceinline__ void store_row(uint32_t *rows, uint32_t i, IsRow r) {
    rows[4 * i] = r.out_len;
    rows[4 * i + 1] = r.used;
    rows[4 * i + 2] = r.status;
    rows[4 * i + 3] = r.msg;
}

// given: the members as the caller named them; patched, head: parse_header_kernel's tables of them.  own_hist: a raw stream
// without a dictionary object counts given[job].dict_len bytes as present in front of its output (the header pass knows no
// such history); else the history is what the header's verdict gave, patched[job].dict_len.
__global__ __launch_bounds__(64)
void inflate_sizes_kernel(const InflateJobDev *__restrict__ given, const InflateJobDev *__restrict__ patched,
                          const uint32_t *__restrict__ head, uint32_t njobs, int format, int own_hist,
                          uint32_t *__restrict__ results) {
    constexpr int kLitRoot = kLitRootStream, kDistRoot = kDistRootStream;
    __shared__ SizesLds<kDistRoot, kLitRoot> L;
    const int lane = threadIdx.x;
    const uint32_t job = blockIdx.x;
    if (job >= njobs) return;
    const InflateJobDev J = patched[job];
    const uint32_t hdr = head[2 * job], hmsg = head[2 * job + 1];
    const uint64_t member_len = given[job].in_len;
    if (hmsg != kMsgNone) {                              // a refused header, another dictionary: nothing to parse
        if (lane == 0) store_row(results, job, is_sizing_row(format, hdr, hmsg, member_len, IsRow{0u, 0u, 0u, 0u}));
        return;
    }
    const ZR_GLOBAL uint8_t *const in = (const ZR_GLOBAL uint8_t *)J.in;
    const uint32_t in_len = (uint32_t)J.in_len, hist = own_hist ? given[job].dict_len : J.dict_len;

#include "inflate_bits_body.h"
    auto widen_literals = [&]() __attribute__((always_inline)) {
        uint32_t w[(1 << kLitRoot) / 64];
#pragma unroll
        for (int j = 0; j < (1 << kLitRoot) / 64; ++j) w[j] = wide_literal(reinterpret_cast<const uint16_t *>(L.lit)[lane + 64 * j]);
        wave_sync();
#pragma unroll
        for (int j = 0; j < (1 << kLitRoot) / 64; ++j) L.lit[lane + 64 * j] = w[j];
        wave_sync();
    };
    auto tables_ready = [&]() __attribute__((always_inline)) { widen_literals(); widen_distances<kDistRoot>(L, lane); };
    seek(0);

    // `count`: what the decode's `op` would be.  `sure`: the count behind the last symbol whose bits were ALL input -- the zero
    // bits behind a truncated stream decode to something too, and the row of such a stream carries this count instead: the
    // bytes inflate() itself delivers for that input, where the decoder's partial count depends on where its flush tests fall.
    // While whole words of input are still to come nothing needs a look (`sure` follows `count` where a word enters the bit
    // buffer); once the last word is in (`tail`), every symbol goes through the general path and is held against the input's end.
    uint32_t count = 0, sure = 0, tail = 0;
    uint32_t msg = kMsgNone;
    bool last = false;
    while (!last && msg == kMsgNone) {
        if (bit_pos() <= 8ull * in_len) sure = count;
        if (cnt < 32) append();
        last = hold & 1u;
        const uint32_t type = (uint32_t)(hold >> 1) & 3u;
        hold >>= 3;
        cnt -= 3;
        if (type == 3) { msg = kMsgBlockType; break; }
        if (type == 0) {
            // stored block (inflate.c:759-800): LEN / NLEN at the next byte boundary are checked, LEN bytes are skipped
            hold >>= cnt & 7u;
            cnt -= cnt & 7u;
            if (cnt < 32) append();
            const uint32_t len = (uint32_t)hold & 0xffffu, nlen = (uint32_t)(hold >> 16) & 0xffffu;
            hold >>= 32;
            cnt -= 32;
            if (bit_pos() > 8ull * in_len) { msg = kMsgStarved; break; }
            if (len != (nlen ^ 0xffffu)) { msg = kMsgStoredLen; break; }
            const uint32_t from = (uint32_t)(bit_pos() >> 3);          // byte aligned here
            const uint32_t avail = in_len - from;
            if (len > avail) {                                         // the bytes that are there count, as in the decode
                is_count_add(&count, avail);
                sure = count;
                msg = kMsgStarved;
                break;
            }
            if (is_count_add(&count, len)) { msg = kMsgOutFull; break; }
            seek(from + len);
            continue;
        }
#include "inflate_block_tables_body.h"

        // ---- symbol loop: the decode half of inflate_fast (inffast_tpl.h:140-226) and nothing of its store half ------------
        // Every branch is wave-uniform and every loop has ONE exit (the stream kernel's lesson: anything else makes the compiler
        // carry exit conditions around as lane masks).  A round is a run of root-table literals -- the inner loop, which does
        // nothing but look up, shift and count -- and then the one symbol that ended the run.  What is rare is looked at where
        // a word enters the bit buffer, once per 32 bits: the end of a truncated stream (whole words behind the input are in
        // the buffer), a count beyond the largest room, and the input's last word (`tail`, above); each sets `halt`, which is
        // OR-ed into the entry so that the run ends as if on a symbol that is no literal.  (Taking the first of the three tests
        // out of this place, to the general path, made the compiler's loop slower: 170 -> 185 ms on the level-1 class's
        // streams of DESIGN 3.9h.)  A literal is counted without a test, so the count may pass
        // kIsCountMax by the literals of one word before the halt: it is clamped behind the loops, and the decode, too,
        // would have stopped at the first byte that did not fit, whatever came after it.
        uint32_t end = 0;                                // 1: the end of the block; 2: `msg` says why
        if (wnext >= total_words) tail = kLitHalt;       // (the block's header took the last word in)
        do {
            uint32_t e, halt = tail, stop = 0;
            do {
                if (cnt < 32) {
                    if (wnext > total_words + 2u || count > kIsCountMax) stop = halt = kLitHalt;
                    if (wnext < total_words) sure = count;                            // (every bit consumed so far is input)
                    if (wnext + 1u >= total_words) tail = halt = kLitHalt;            // the last word of input comes in
                    append();
                }
                e = uni(L.lit[(uint32_t)hold & ((1u << kLitRoot) - 1u)]) | halt;
                const uint32_t nb = e < 16u ? e : 0u;                                 // a literal: taken; anything else: looked at below
                hold >>= nb;
                cnt -= nb;
                count += e < 16u ? 1u : 0u;
            } while (e < 16u);
            if (stop) {
                msg = count > kIsCountMax ? kMsgOutFull : kMsgStarved;
                end = 2;
            } else {
                e &= ~kLitHalt;
                if (e == kLitLong) e = wide_literal(long_code(L, kCodeLit, kLitRoot, L.sorted_lit, hold));
                const uint32_t nb = e & 15u;
                if (e & kLitBad) {
                    msg = bit_pos() + nb > 8ull * in_len ? kMsgStarved : kMsgLitLenCode;  // (its bits must all be input)
                    end = 2;
                } else {
                    hold >>= nb;
                    cnt -= nb;
                    if (e < 16u) {                                                    // a literal: one with a long code, or one of the tail
                        ++count;
                    } else if (e & kLitEob) {                                         // end of block
                        end = 1;
                    } else {
                        const uint32_t xb = (e >> 4) & 15u;
                        const uint32_t len = ((e >> 8) & 0x1ffu) + ((uint32_t)hold & ((1u << xb) - 1u));
                        hold >>= xb;
                        cnt -= xb;
                        if (cnt < 32) append();
                        uint32_t d = uni(L.dist[(uint32_t)hold & ((1u << kDistRoot) - 1u)]);
                        if (d == kLongWide) d = wide_distance(long_code(L, kCodeDist, kDistRoot, L.sorted_dist, hold));
                        if (d >= kBadWide) {
                            msg = bit_pos() + (d & 15u) > 8ull * in_len ? kMsgStarved : kMsgDistCode;
                            end = 2;
                        } else {
                            const uint32_t dnb = d & 15u, dxb = (d >> 4) & 15u;
                            hold >>= dnb;
                            const uint32_t dist = (d >> 8) + ((uint32_t)hold & ((1u << dxb) - 1u));
                            hold >>= dxb;
                            cnt -= dnb + dxb;
                            if (dist > count + hist) {                                // inffast_tpl.h:203-210
                                msg = kMsgTooFar;
                                end = 2;
                            } else if (count > kIsCountMax || is_count_add(&count, len)) {
                                msg = kMsgOutFull;
                                end = 2;
                            }
                        }
                    }
                    // (a match may have brought the last word in by itself)
                    if (wnext >= total_words) {
                        tail = kLitHalt;
                        if (end != 2 && bit_pos() <= 8ull * in_len) sure = count;
                    }
                }
            }
        } while (!end);
    }
    if (count > kIsCountMax) {                           // literals counted past the largest room (see the symbol loop)
        count = kIsCountMax;
        msg = kMsgOutFull;
    }
    if (sure > kIsCountMax) sure = kIsCountMax;
    // bits that do not exist were consumed: whatever happened after that point, the stream ended early
    if (bit_pos() > 8ull * in_len) msg = kMsgStarved;
    if (lane == 0) {
        const unsigned long long used = (bit_pos() + 7ull) >> 3;
        const IsRow raw = {msg == kMsgStarved ? sure : count, used > in_len ? in_len : (uint32_t)used, is_status_of(msg), msg};
        store_row(results, job, is_sizing_row(format, hdr, hmsg, member_len, raw));
    }
}

// ---- packed decode: places, the patched table, the final rows -----------------------------------------------------------
// one workgroup, a tiled scan over any njobs (as cs_scan_kernel): offsets[i] = the sum of the padded rooms in front of job i,
// offsets[njobs] = the end of the last job's bytes
__global__ __launch_bounds__(1024)
void sizes_place_kernel(const uint32_t *__restrict__ sizing, uint32_t njobs, uint32_t align, unsigned long long *__restrict__ offsets) {
    __shared__ unsigned long long wave_sum[16];
    __shared__ unsigned long long carry;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) {
        carry = 0;
        if (!njobs) offsets[0] = 0;
    }
    __syncthreads();
    for (uint32_t base = 0; base < njobs; base += 1024u) {
        const uint32_t i = base + (uint32_t)t;
        const bool live = i < njobs;
        const unsigned long long room = live ? is_room(load_row(sizing, i)) : 0ull;
        const unsigned long long v = is_padded(room, align);
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
            offsets[i] = off;
            if (i + 1u == njobs) offsets[njobs] = is_need(off, room);
        }
        __syncthreads();
        if (t == 1023) carry = before + incl;
        __syncthreads();
    }
}

__device__ __forceinline__ bool sizes_decoded(IsRow sizing, unsigned long long off, unsigned long long dst_cap) {
    return (int32_t)sizing.status == 1 && is_fits(off, is_room(sizing), dst_cap);
}

// a job that has a place and fits: out = d_dst + its offset, out_cap = its size; every other job becomes an empty job, which
// costs the engine nothing and stores nothing
__global__ __launch_bounds__(256)
void sizes_patch_kernel(const uint32_t *__restrict__ sizing, const unsigned long long *__restrict__ offsets, uint32_t njobs,
                        uint8_t *d_dst, unsigned long long dst_cap, InflateJobDev *__restrict__ patched) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= njobs) return;
    const IsRow s = load_row(sizing, i);
    InflateJobDev p = patched[i];
    if (sizes_decoded(s, offsets[i], dst_cap)) {
        p.out = d_dst + offsets[i];
        p.out_cap = s.out_len;
    } else {
        p.out = nullptr;
        p.in_len = 0;
        p.out_cap = 0;
    }
    patched[i] = p;
}

__global__ __launch_bounds__(256)
void sizes_final_kernel(const uint32_t *__restrict__ sizing, const unsigned long long *__restrict__ offsets, uint32_t njobs,
                        unsigned long long dst_cap, uint32_t *__restrict__ results) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= njobs) return;
    const IsRow s = load_row(sizing, i);
    store_row(results, i, is_final_row(s, sizes_decoded(s, offsets[i], dst_cap), load_row(results, i)));
}

// Streams per CU: the tables let 22 wavefronts share a CU's 160 KiB of LDS; held at the decoder's 16 (padded to 10 KiB in a
// build made for the measurement) the kernel measured the same within the spread, so the natural size stays.
static int launch_inflate_sizes(const InflateJobDev *d_given, const InflateJobDev *d_patched, const uint32_t *d_head, size_t njobs,
                                int format, bool own_hist, uint32_t *d_rows, hipStream_t st) {
    ZR_LAUNCH_TRACED(inflate_sizes_kernel, dim3((unsigned)njobs), dim3(64), st, d_given, d_patched, d_head, (uint32_t)njobs, format,
                     own_hist ? 1 : 0, d_rows);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

// both calls: `packed` = zng_rocm_uncompress_packed_dev.  The arguments have passed inflate_sizes_plan.h's checks.
static int sizes_body(bool packed, int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                      uint8_t *d_dst, size_t dst_cap, uint32_t align, uint64_t *d_offsets, uint32_t *d_results, hipStream_t st) {
    DeviceGuard dev;
    Workspace *ws = workspace_for(st);
    if (!ws) return ZNG_ROCM_ENOMEM;
    std::lock_guard<std::mutex> use(ws->mu);
    unsigned long long *const d_off = reinterpret_cast<unsigned long long *>(d_offsets);
    if (!njobs) {                                        // (the packed call alone gets here: an empty batch needs no room)
        hipLaunchKernelGGL(sizes_place_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t *)nullptr, 0u, align, d_off);
        ZR_HIP(hipGetLastError());
        return ZNG_ROCM_OK;
    }
    uint32_t *d_sizing = d_results;
    if (packed)
        if (int rc = scratch_reserve(ws, kScrSizes, njobs * 4 * sizeof(uint32_t), false, (void **)&d_sizing)) return rc;
    GivenJobs g;
    if (int rc = upload_given_jobs(ws, format, dict, jobs, njobs, false, packed, &g, st)) return rc;
    if (int rc = launch_inflate_sizes(g.d_given, g.d_patched, g.d_head, njobs, format, format == 0 && !dict, d_sizing, st)) return rc;
    if (!packed) return ZNG_ROCM_OK;
    const dim3 grid((unsigned)((njobs + 255) / 256)), block(256);
    hipLaunchKernelGGL(sizes_place_kernel, dim3(1), dim3(1024), 0, st, d_sizing, (uint32_t)njobs, align, d_off);
    ZR_HIP(hipGetLastError());
    hipLaunchKernelGGL(sizes_patch_kernel, grid, block, 0, st, d_sizing, d_off, (uint32_t)njobs, d_dst, (unsigned long long)dst_cap,
                       g.d_patched);
    ZR_HIP(hipGetLastError());
    if (int rc = uncompress_patched_device(format, dict, g.d_given, g.d_patched, g.d_head, g.d_checks, g.d_msg, g.d_part, njobs,
                                           d_results, st))
        return rc;
    hipLaunchKernelGGL(sizes_final_kernel, grid, block, 0, st, d_sizing, d_off, (uint32_t)njobs, (unsigned long long)dst_cap,
                       d_results);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

// the refusals in inflate_sizes_plan.h's order, then the device (the dictionary's, or the context of zng_rocm_init): 0 = go on
static int sizes_enter(bool packed, int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                       const void *d_dst, size_t dst_cap, uint32_t align, const void *d_offsets, const void *d_results) {
    const int rc = packed ? is_packed_call_check(format, dict != nullptr, jobs, njobs, d_dst, dst_cap, align, d_offsets, d_results)
                          : is_call_check(format, dict != nullptr, jobs, njobs, d_results);
    if (rc) {
        set_error(packed ? "format 0..2 (2 takes no dictionary), align 0, 1 or a power of two up to 4096, d_offsets and d_results, "
                           "and d_dst unless dst_cap is 0"
                         : "format 0..2 (2 takes no dictionary), and jobs and d_results unless njobs is 0");
        return rc;
    }
    uint64_t bad = 0;
    if (int jrc = is_jobs_check(format, dict != nullptr, jobs, njobs, packed, &bad)) {
        set_error("job %llu: null input, a stream of 2 GiB and more, flags, or a dict_len that is above 32768 or stands beside a "
                  "dictionary object, a wrapped format or a packed destination", (unsigned long long)bad);
        return jrc;
    }
    if (!packed && !njobs) return ZNG_ROCM_OK;           // (the caller returns: nothing to do needs no device)
    if (dict) return dict_usable(dict);
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    return ZNG_ROCM_OK;
}

}  // namespace zr

using namespace zr;

extern "C" {

int zng_rocm_inflate_sizes_dev(int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                               uint32_t *d_results, void *stream) {
    if (int rc = sizes_enter(false, format, dict, jobs, njobs, nullptr, 0, 0, nullptr, d_results)) return rc;
    if (!njobs) return ZNG_ROCM_OK;
    return sizes_body(false, format, dict, jobs, njobs, nullptr, 0, 0, nullptr, d_results, (hipStream_t)stream);
}

int zng_rocm_uncompress_packed_dev(int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                                   uint8_t *d_dst, size_t dst_cap, uint32_t align, uint64_t *d_offsets, uint32_t *d_results,
                                   void *stream) {
    if (int rc = sizes_enter(true, format, dict, jobs, njobs, d_dst, dst_cap, align, d_offsets, d_results)) return rc;
    return sizes_body(true, format, dict, jobs, njobs, d_dst, dst_cap, align, d_offsets, d_results, (hipStream_t)stream);
}

}  // extern "C"
