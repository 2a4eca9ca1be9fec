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
// stream, the same 64-word fetch and bit buffer, the same block headers and the same table builder (inflate_tables.h), and a
// symbol loop that adds a literal's 1 and a match's length to a count.  It still decodes every distance -- for its bits, and
// for "invalid distance too far back" against count + history length -- but has no window, no ring, no copy and no store: the
// history's LENGTH is all it knows of the history.  Every verdict, message and count of consumed bytes is the decoder's
// (inflate_streams_body.h), the truncation rule of kBadWide included: the two are held against each other stream by stream
// in tests/test_gpu_inflate_sizes.py.  The rules on top -- argument checks, saturation, the member's row, places, fit, final
// rows -- are inflate_sizes_plan.h's, for host and device alike.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "context.h"
#include "dict_dev.h"
#include "framing_dev.h"
#include "inflate_dev.h"
#include "inflate_sizes_plan.h"
#include "inflate_tables.h"

namespace zr {

// The tables of one stream, packed as InflateLdsPart packs them (the code-length code only lives while a dynamic header is
// read: it shares the distance table's place) and without a ring: 7.2 KiB against the decoder's 9.9 KiB.
template <int DR, int LR>
struct SizesLds {
    uint32_t lit[1 << LR];                  // wide entries (wide_literal); the builder's 16-bit entries lie in the first half
    union {
        uint32_t dist[1 << DR];             // wide entries (wide_distance)
        struct {
            uint16_t cl[1 << kClRoot];
            uint16_t sorted_cl[32];
            uint32_t cnt[16];
            uint16_t first[16], offs[16];
            uint8_t  cl_lens[24];
        } h;
    };
    uint32_t cnt_[2][16];               // [code][length]; slot 0 of a code: its longest length
    uint16_t first_[2][16], offs_[2][16], run[16];
    uint16_t sorted_lit[288], sorted_dist[32];
    uint8_t  lens[320 + 8];
    __device__ __forceinline__ uint32_t *cnt(int which) { return which == kCodeCl ? h.cnt : cnt_[which]; }
    __device__ __forceinline__ uint16_t *first(int which) { return which == kCodeCl ? h.first : first_[which]; }
    __device__ __forceinline__ uint16_t *offs(int which) { return which == kCodeCl ? h.offs : offs_[which]; }
    __device__ __forceinline__ uint16_t *cl() { return h.cl; }
    __device__ __forceinline__ uint16_t *sorted_cl() { return h.sorted_cl; }
    __device__ __forceinline__ uint8_t *cl_lens() { return h.cl_lens; }
};
constexpr int kSizesLitRoot = kLitRootStream, kSizesDistRoot = kDistRootStream;
static_assert(sizeof(((SizesLds<kSizesDistRoot, kSizesLitRoot> *)nullptr)->h) <= sizeof(uint32_t) << kSizesDistRoot,
              "the header's tables must fit the distance table's place");

// The literal/length table's loop form.  The sizing pass never needs a literal's VALUE, so a literal's entry is its code length
// alone (1 .. 15: "entry < 16" is the literal test and the entry is the shift), and a length symbol's entry carries its base
// length and extra-bit count, as wide_distance's entries do: no arithmetic on the symbol in the loop.
constexpr uint32_t kLitLength = 1u << 20, kLitEob = 1u << 21, kLitLong = 1u << 22, kLitBad = 1u << 23, kLitHalt = 1u << 24;
__device__ __forceinline__ uint32_t wide_literal(uint32_t e) {            // e: a 16-bit entry
    if (e == kLongMark) return kLitLong;
    const uint32_t sym = e >> 4, nb = e & 15u;
    if (sym < 256u) return nb;
    if (sym == 256u) return kLitEob | nb;
    if (sym > 285u) return kLitBad | nb;                                      // 286, 287 (inftrees.c:44-45), no code
    uint32_t b = 0, x = 0;
    length_of(sym - 257u, &b, &x);
    return kLitLength | (b << 8) | (x << 4) | nb;
}

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
    constexpr int kLR = kSizesLitRoot, kDR = kSizesDistRoot;
    __shared__ SizesLds<kDR, kLR> L;
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

    // ---- compressed words: 64 per fetch, the next 64 prefetched (as the stream kernel) --------------------------------
    const uint32_t lead = (uint32_t)((uintptr_t)J.in & 3u);
    const ZR_GLOBAL uint32_t *const words = (const ZR_GLOBAL uint32_t *)(in - lead);
    const uint32_t total_words = (lead + in_len + 3u) >> 2;
    auto fetch = [&](uint32_t base) __attribute__((always_inline)) -> uint32_t {
        const uint32_t k = base + (uint32_t)lane;
        return k < total_words ? words[k] : 0u;
    };
    uint32_t cbase = 0, cur = 0, nxt = 0;
    uint32_t wnext = 0;                                  // index of the next word to enter the bit buffer
    unsigned long long hold = 0;
    uint32_t cnt = 0;
    auto append = [&]() __attribute__((always_inline)) {                                // cnt <= 32 on entry
        const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)(wnext - cbase));
        hold |= (unsigned long long)w << cnt;
        cnt += 32;
        ++wnext;
        if (wnext - cbase == 64) {
            cbase += 64;
            cur = nxt;
            nxt = fetch(cbase + 64);
        }
    };
    auto seek = [&](uint32_t byte_off) __attribute__((always_inline)) {                 // restart the bit buffer at a byte of the stream
        const uint32_t a = lead + byte_off;
        wnext = a >> 2;
        cbase = wnext;
        cur = fetch(cbase);
        nxt = fetch(cbase + 64);
        hold = 0;
        cnt = 0;
        append();
        hold >>= 8 * (a & 3u);
        cnt -= 8 * (a & 3u);
    };
    auto bit_pos = [&]() __attribute__((always_inline)) -> unsigned long long {         // stream bits consumed so far
        return 32ull * wnext - 8ull * lead - cnt;
    };
    auto widen_distances = [&]() __attribute__((always_inline)) {
        uint32_t w[(1 << kDR) / 64];
#pragma unroll
        for (int j = 0; j < (1 << kDR) / 64; ++j) w[j] = wide_distance(reinterpret_cast<const uint16_t *>(L.dist)[lane + 64 * j]);
        wave_sync();
#pragma unroll
        for (int j = 0; j < (1 << kDR) / 64; ++j) L.dist[lane + 64 * j] = w[j];
        wave_sync();
    };
    auto widen_literals = [&]() __attribute__((always_inline)) {
        uint32_t w[(1 << kLR) / 64];
#pragma unroll
        for (int j = 0; j < (1 << kLR) / 64; ++j) w[j] = wide_literal(reinterpret_cast<const uint16_t *>(L.lit)[lane + 64 * j]);
        wave_sync();
#pragma unroll
        for (int j = 0; j < (1 << kLR) / 64; ++j) L.lit[lane + 64 * j] = w[j];
        wave_sync();
    };
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
        if (type == 1) {
            // fixed codes (RFC 1951 3.2.6, inflate.c:801-813): the same builder, from the fixed lengths
            for (int s = lane; s < 288; s += 64) L.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
            if (lane < 32) L.lens[288 + lane] = 5;
            wave_sync();
            build_code(L, kCodeLit, L.lens, 288, kLR, reinterpret_cast<uint16_t *>(L.lit), L.sorted_lit, lane);
            build_code(L, kCodeDist, L.lens + 288, 32, kDR, reinterpret_cast<uint16_t *>(L.dist), L.sorted_dist, lane);
            widen_literals();
            widen_distances();
        } else {
            // dynamic block header (inflate.c:814-917), read as the stream kernel reads it: the same bits consumed in
            // front of every fault
            if (cnt < 32) append();
            const uint32_t nlen = ((uint32_t)hold & 31u) + 257u, ndist = ((uint32_t)(hold >> 5) & 31u) + 1u,
                           ncode = ((uint32_t)(hold >> 10) & 15u) + 4u;
            hold >>= 14;
            cnt -= 14;
            if (nlen > 286 || ndist > 30) { msg = kMsgTooMany; break; }
            if (lane < 19) L.cl_lens()[lane] = 0;
            wave_sync();
            for (uint32_t i = 0; i < ncode; ++i) {
                if (cnt < 32) append();
                if (lane == 0) L.cl_lens()[kClOrder[i]] = (uint8_t)(hold & 7u);
                hold >>= 3;
                cnt -= 3;
            }
            wave_sync();
            if (uni((uint32_t)build_code(L, kCodeCl, L.cl_lens(), 19, kClRoot, L.cl(), L.sorted_cl(), lane))) { msg = kMsgCodeLengthsSet; break; }
            uint32_t have = 0;
            while (have < nlen + ndist) {
                if (cnt < 32) append();
                const uint32_t e = uni(L.cl()[(uint32_t)hold & ((1u << kClRoot) - 1u)]);
                const uint32_t nb = e & 15u, sym = e >> 4;
                hold >>= nb;
                cnt -= nb;
                if (sym < 16) {
                    if (lane == 0) L.lens[have] = (uint8_t)sym;
                    ++have;
                    continue;
                }
                uint32_t rep, val = 0;
                if (sym == 16) {
                    rep = 3u + ((uint32_t)hold & 3u);
                    hold >>= 2;
                    cnt -= 2;
                    if (have == 0) { msg = kMsgBitRepeat; break; }
                    wave_sync();
                    val = uni(L.lens[have - 1]);
                } else if (sym == 17) {
                    rep = 3u + ((uint32_t)hold & 7u);
                    hold >>= 3;
                    cnt -= 3;
                } else {
                    rep = 11u + ((uint32_t)hold & 127u);
                    hold >>= 7;
                    cnt -= 7;
                }
                if (have + rep > nlen + ndist) { msg = kMsgBitRepeat; break; }
                for (uint32_t k = (uint32_t)lane; k < rep; k += 64) L.lens[have + k] = (uint8_t)val;
                have += rep;
            }
            if (msg != kMsgNone) break;
            wave_sync();
            if (bit_pos() > 8ull * in_len) { msg = kMsgStarved; break; }
            if (uni(L.lens[256]) == 0) { msg = kMsgNoEob; break; }
            if (uni((uint32_t)build_code(L, kCodeLit, L.lens, (int)nlen, kLR, reinterpret_cast<uint16_t *>(L.lit), L.sorted_lit, lane))) { msg = kMsgLitLenSet; break; }
            if (uni((uint32_t)build_code(L, kCodeDist, L.lens + nlen, (int)ndist, kDR, reinterpret_cast<uint16_t *>(L.dist),
                                         L.sorted_dist, lane))) {
                msg = kMsgDistSet;
                break;
            }
            widen_literals();
            widen_distances();
        }

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
                e = uni(L.lit[(uint32_t)hold & ((1u << kLR) - 1u)]) | halt;
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
                if (e == kLitLong) e = wide_literal(long_code(L, kCodeLit, kLR, L.sorted_lit, hold));
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
                        uint32_t d = uni(L.dist[(uint32_t)hold & ((1u << kDR) - 1u)]);
                        if (d == kLongWide) d = wide_distance(long_code(L, kCodeDist, kDR, L.sorted_dist, hold));
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
    InflateJobDev *d_given = nullptr, *h_given = nullptr, *d_patched = nullptr;
    uint32_t *d_words = nullptr, *d_sizing = d_results;
    uint8_t *d_msg = nullptr;
    Partial *d_part = nullptr;
    if (int rc = scratch_reserve(ws, kScrInflateDevJobs, 2 * njobs * sizeof(InflateJobDev), false, (void **)&d_given)) return rc;
    d_patched = d_given + njobs;
    // head rows: 2 words per job; the packed call's check values: 2 more
    if (int rc = scratch_reserve(ws, kScrFrameWords, njobs * (packed ? 4 : 2) * sizeof(uint32_t), false, (void **)&d_words)) return rc;
    uint32_t *d_head = d_words, *d_checks = packed ? d_words + 2 * njobs : nullptr;
    if (packed) {
        if (int rc = scratch_reserve(ws, kScrSizes, njobs * 4 * sizeof(uint32_t), false, (void **)&d_sizing)) return rc;
        if (int rc = scratch_reserve(ws, kScrCheckMessages, njobs * (sizeof(StreamArgs) + sizeof(FinalArgs)), false, (void **)&d_msg)) return rc;
        if (int rc = scratch_reserve(ws, kScrCheckPartials, njobs * sizeof(Partial), false, (void **)&d_part)) return rc;
    }
    if (int rc = host_tables_acquire(ws)) return rc;
    if (int rc = scratch_reserve(ws, kScrInflateDevJobsHost, njobs * sizeof(InflateJobDev), true, (void **)&h_given)) return rc;
    for (size_t i = 0; i < njobs; ++i) {
        const zng_rocm_inflate_dev_job &j = jobs[i];
        h_given[i] = InflateJobDev{(const uint8_t *)j.in, nullptr, j.in_len, 0u, j.dict_len, 0u};
    }
    ZR_HIP(hipMemcpyAsync(d_given, h_given, njobs * sizeof(InflateJobDev), hipMemcpyHostToDevice, st));
    if (int rc = host_tables_release(ws, st)) return rc;
    if (int rc = launch_parse_header(format, dict, d_given, njobs, d_patched, d_head, st)) return rc;
    if (int rc = launch_inflate_sizes(d_given, d_patched, d_head, njobs, format, format == 0 && !dict, d_sizing, st)) return rc;
    if (!packed) return ZNG_ROCM_OK;
    const dim3 grid((unsigned)((njobs + 255) / 256)), block(256);
    hipLaunchKernelGGL(sizes_place_kernel, dim3(1), dim3(1024), 0, st, d_sizing, (uint32_t)njobs, align, d_off);
    ZR_HIP(hipGetLastError());
    hipLaunchKernelGGL(sizes_patch_kernel, grid, block, 0, st, d_sizing, d_off, (uint32_t)njobs, d_dst, (unsigned long long)dst_cap,
                       d_patched);
    ZR_HIP(hipGetLastError());
    if (int rc = uncompress_patched_device(format, dict, d_given, d_patched, d_head, d_checks, d_msg, d_part, njobs, d_results, st))
        return rc;
    hipLaunchKernelGGL(sizes_final_kernel, grid, block, 0, st, d_sizing, d_off, (uint32_t)njobs, (unsigned long long)dst_cap,
                       d_results);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

// the refusals in inflate_sizes_plan.h's order, then the device: 0 = go on
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
    return ZNG_ROCM_OK;
}

}  // namespace zr

using namespace zr;

extern "C" {

int zng_rocm_inflate_sizes_dev(int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                               uint32_t *d_results, void *stream) {
    if (int rc = sizes_enter(false, format, dict, jobs, njobs, nullptr, 0, 0, nullptr, d_results)) return rc;
    if (!njobs) return ZNG_ROCM_OK;
    if (dict) {
        if (int rc = dict_usable(dict)) return rc;
    } else if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    return sizes_body(false, format, dict, jobs, njobs, nullptr, 0, 0, nullptr, d_results, (hipStream_t)stream);
}

int zng_rocm_uncompress_packed_dev(int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                                   uint8_t *d_dst, size_t dst_cap, uint32_t align, uint64_t *d_offsets, uint32_t *d_results,
                                   void *stream) {
    if (int rc = sizes_enter(true, format, dict, jobs, njobs, d_dst, dst_cap, align, d_offsets, d_results)) return rc;
    if (dict) {
        if (int rc = dict_usable(dict)) return rc;
    } else if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    return sizes_body(true, format, dict, jobs, njobs, d_dst, dst_cap, align, d_offsets, d_results, (hipStream_t)stream);
}

}  // extern "C"
