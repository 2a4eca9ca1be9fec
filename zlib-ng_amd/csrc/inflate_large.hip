// inflate_large.hip -- ONE large raw deflate stream inflated on the device (BASELINE.json configs[2]).
//
// inflate_fast (inffast_tpl.h:53-318) is a serial bit parse: where a code starts depends on every code before it, and a
// block header carries no marker.  inflate_dev.hip therefore needs many streams to fill the chip (one wavefront each).
// This file cuts ONE stream into parts the same kernel can take -- the scheme of inflate_threads.cpp (pugz / rapidgzip),
// with the device in place of the host threads:
//   F1 find_headers_table_kernel  every BIT position of the stream is tested for the start of a dynamic block the decoder
//        would accept, cheap tests first: BTYPE / HLIT / HDIST in range (inflate.c:808-813), the code-length code complete
//        (inftrees.c:126-131; a Kraft sum over the 3-bit fields, three fields per table lookup).  About 1 position in
//        10^3 is left.  Also: the byte pattern 00 00 ff ff of a sync-flush marker (deflate.c:1064-1076) -- the block
//        behind it starts on the next byte, whatever its type -- and a stored block's header on a byte boundary
//        (header byte, LEN, NLEN = ~LEN; inflate.c:759-775): incompressible data is a chain of those.
//   F2 validate_headers_table_kernel  one lane per survivor decodes the whole header (inflate.c:814-917) and applies the
//        validity rules of inflate_table to the two code sets (inftrees.c:104-137): about 1 random position in 10^6
//        survives both kernels, real block starts all do.
//   host                        sorts the few thousand candidates (at least 2 KiB of compressed bytes apart); bit 0 is
//        always a start (thin_starts).
//   P  inflate_streams_kernel<PART>  one wavefront per part, from its start until a block ends EXACTLY on a later start
//        (or BFINAL), 16-bit symbols into the part's own slot (a symbol >= 256 names a byte of the 32 KiB in front of
//        the part: nobody knows yet what is there).
//   host                        chains the parts from bit 0: part 0 is genuine, the part that starts where it ended is
//        therefore genuine too, ...; a candidate that was noise is simply never reached (and the part in front of it has
//        run across it).  Then every part's place in the output is known (walk_chain, group_segments).
//   C  compact_parts_kernel     slots -> one symbol array, consecutive parts grouped into segments of >= 40 KiB (the
//        context chain of inflate_resolve.hip looks one segment back) with their references re-based to the segment;
//        K2 / K3 of inflate_resolve.hip resolve and translate.
// Anything irregular on the chain -- a data error, a truncated stream, a distance too far back, no candidates (a stream of fixed-Huffman blocks only) -- sends the call to the sequential host decoder, which
// then reports exactly what the reference would (status, message, bytes produced, bytes consumed).
// Every step is written ONCE, for N streams.  The finder (find_starts) scans a table of (stream, range) items whose survivors
// carry their stream: the byte patterns for all streams, F1 / F2 for those they do not cut.  The pass behind it (pass_run):
// one part launch over the parts of all streams, one more for the parts whose slot was too small, one chain per stream, one
// compaction, one resolve.  ONE stream -- inflate_large_try: the one-pass call, every piece of
// zng_rocm_inflate_large_pieces_dev, the hook's blocks mode, a host-resident stream -- is a table of one;
// zng_rocm_inflate_large_streams_dev takes a round of streams at a time.  Each caller maps what the finder and the pass say
// about a stream -- done, too large for dst_cap, or "left the pass" -- to its own convention.
// What the host does between the launches -- the steps named above, the SUBBLOCK regions and their merge, the slot sizes,
// where the tables lie in scratch, which parts run again, the symbol array's layout -- is in inflate_large_plan.h.  This file
// keeps the kernels, the scratch and table uploads, the launches and synchronisations, and each entry point's policy for a
// stream the device path cannot do.  ONE stream's pass is asked for and answered by value (LargeRequest, LargeAnswer); what
// the last_* getters report is published once, at each entry point's exit (LargeCounters, one_pass).  The pieces loop
// (inflate_pieces_call) steps by the plan's rules too (PiecesState): here it splices the history, runs the pass or the
// sequential decoder, and uploads.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "inflate_large_limits.h"
#include "inflate_large_plan.h"
#include "context.h"
#include "deflate_dev.h"
#include "inflate_dev.h"
#include "inflate_large_size_plan.h"
#include "inflate_threads.h"

namespace zr {

// SUBBLOCK (zng_rocm_inflate_large_ex_dev): guesses for starts inside blocks, one every `step` compressed bits of a region,
// step = the stream's bits / (kSubPerSlot x the chip's resident parts), at least kSubMinStep bits -- so that a block of any
// length is cut into pieces of about the same compressed size, whatever it expands to
constexpr uint32_t kSubPerSlot = 4;
constexpr uint64_t kSubMinStep = 8ull * (2u << 10);

// 64 bits of the stream starting at `bit` (bits beyond the end read 0)
__device__ __forceinline__ unsigned long long bits_at_dev(const uint8_t *src, unsigned long long src_len, unsigned long long bit) {
    const unsigned long long byte = bit >> 3;
    unsigned long long lo = 0, hi = 0;
    if (byte + 16 <= src_len) {
        const u32x4_unaligned v = load_u128(src + byte);
        lo = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
        hi = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
    } else {
        for (unsigned k = 0; k < 16 && byte + k < src_len; ++k) {
            const unsigned long long b = load_u8(src + byte + k);
            if (k < 8) lo |= b << (8 * k);
            else hi |= b << (8 * (k - 8));
        }
    }
    const unsigned s = (unsigned)(bit & 7ull);
    return s ? (lo >> s) | (hi << (64 - s)) : lo;
}

// F1.  One lane per byte, its eight bit positions in turn; a workgroup scans a contiguous piece of the stream and collects its
// survivors in LDS, so the global list takes one atomic per workgroup and flush (a single contended word manages ~90
// atomics per microsecond: one per survivor would cost more than the scan).  cand: bit position, bit 63 set for "block
// behind a marker".
// PATTERNS = true: the two byte patterns only (no bit position is tested): the first pass -- a stream whose encoder left a
// sync marker or a stored block every few tens of KiB (this library's level-6 class, pigz) offers enough starts that way.
constexpr uint32_t kFindLocal = 2048;
// The scan itself, bytes [lo_b, hi_b) of one stream: find_headers_table_kernel gives every workgroup a (stream, range) pair
// of a table; `tag` (the stream's index << kFindTagShift, inflate_dev_types.h) is set in every survivor.
template <bool PATTERNS>
__device__ __forceinline__ void find_headers_range(const uint8_t *__restrict__ src, const unsigned long long src_len,
                                                   const unsigned long long lo_b, const unsigned long long hi_b,
                                                   const unsigned long long tag, unsigned long long *__restrict__ cand,
                                                   uint32_t *__restrict__ ncand, uint32_t cap) {
    __shared__ uint8_t kraft9[512];            // three 3-bit code lengths -> their share of the Kraft sum, in 1/128
    __shared__ unsigned long long local[kFindLocal];
    __shared__ uint32_t nlocal, gbase;
    for (int v = threadIdx.x; v < 512 && !PATTERNS; v += 256) {
        unsigned sum = 0;
        for (int f = 0; f < 3; ++f) {
            const unsigned l = (v >> (3 * f)) & 7;
            if (l) sum += 128u >> l;
        }
        kraft9[v] = (uint8_t)sum;
    }
    if (threadIdx.x == 0) nlocal = 0;
    __syncthreads();
    auto flush = [&]() {                         // all threads
        __syncthreads();
        const uint32_t n = nlocal < kFindLocal ? nlocal : kFindLocal;
        if (threadIdx.x == 0) gbase = n ? atomicAdd(ncand, n) : 0u;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += 256)
            if (gbase + i < cap) cand[gbase + i] = local[i];
        __syncthreads();
        if (threadIdx.x == 0) nlocal = 0;
        __syncthreads();
    };
    if constexpr (PATTERNS) {
        // the two byte patterns alone: a lane takes 16 byte positions from one 24-byte window (position by position, with a
        // 16-byte load each, the pass read every byte 16 times and ran at 0.44 TB/s: 0.22 ms for 96 MB)
        auto test = [&](unsigned long long w, unsigned long long b) {      // w: the 8 bytes at position b
            if (b >= hi_b || b + 8 >= src_len) return;
            if ((uint32_t)w == 0xffff0000u && b + 6 <= src_len) {
                const uint32_t i = atomicAdd(&nlocal, 1u);
                if (i < kFindLocal) local[i] = (8ull * (b + 4)) | (1ull << 63) | tag;
            }
            const uint32_t len16 = (uint32_t)(w >> 8) & 0xffffu, nlen16 = (uint32_t)(w >> 24) & 0xffffu;
            if (((uint32_t)w & 0xfeu) == 0u && len16 != 0u && (len16 ^ nlen16) == 0xffffu && b + 5 + len16 <= src_len) {
                const uint32_t i = atomicAdd(&nlocal, 1u);
                if (i < kFindLocal) local[i] = (8ull * b) | (3ull << 62) | tag;
            }
        };
        for (unsigned long long base = lo_b; base < hi_b; base += 4096) {
            const unsigned long long b0 = base + 16ull * threadIdx.x;
            if (b0 < hi_b) {
                unsigned long long lo = 0, hi = 0, nx = 0;
                if (b0 + 24 <= src_len) {
                    const u32x4_unaligned v = load_u128(src + b0);
                    lo = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
                    hi = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
                    const u32x4_unaligned n = load_u128(src + b0 + 8);                   // bytes 8 .. 23: the upper half is what is new
                    nx = (unsigned long long)n.z | ((unsigned long long)n.w << 32);
                } else {
                    for (unsigned k = 0; k < 24 && b0 + k < src_len; ++k) {
                        const unsigned long long x = load_u8(src + b0 + k);
                        if (k < 8) lo |= x << (8 * k);
                        else if (k < 16) hi |= x << (8 * (k - 8));
                        else nx |= x << (8 * (k - 16));
                    }
                }
                // a byte 0 or 1 in front, or 00 00 ff ff: positions whose first byte is neither 0x00 nor 0x01 cannot match
#pragma unroll
                for (unsigned k = 0; k < 16; ++k) {
                    const unsigned long long a = k < 8 ? lo : hi, c = k < 8 ? hi : nx;
                    const unsigned sh = 8 * (k & 7);
                    const unsigned long long w = sh ? (a >> sh) | (c << (64 - sh)) : a;
                    if (((uint32_t)w & 0xfeu) == 0u) test(w, b0 + k);
                }
            }
            __syncthreads();
            const uint32_t nl = nlocal;
            __syncthreads();
            if (nl > kFindLocal / 4) flush();
        }
        flush();
        return;
    }
    for (unsigned long long base = lo_b; base < hi_b; base += 256) {
        const unsigned long long b = base + threadIdx.x;
        if (b < hi_b && b + 8 < src_len) {
            unsigned long long lo = 0, hi = 0;
            if (b + 16 <= src_len) {
                const u32x4_unaligned v = load_u128(src + b);
                lo = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
                hi = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
            } else {
                for (unsigned k = 0; k < 16 && b + k < src_len; ++k) {
                    const unsigned long long x = load_u8(src + b + k);
                    if (k < 8) lo |= x << (8 * k);
                    else hi |= x << (8 * (k - 8));
                }
            }
            if ((uint32_t)lo == 0xffff0000u && b + 6 <= src_len) {       // 00 00 ff ff: the block behind the marker
                const uint32_t i = atomicAdd(&nlocal, 1u);
                if (i < kFindLocal) local[i] = (8ull * (b + 4)) | (1ull << 63) | tag;
            }
            // a stored block that starts on a byte boundary (as every stored block behind another one does: a run of
            // incompressible data is a chain of them, and without these starts it would be ONE part -- 8 MiB of the cfg3 mix
            // were, and that part was the whole kernel's tail): header byte 0 or 1, LEN, NLEN = ~LEN.  Noise passes this
            // once in 2^23 bytes; a false start costs one wasted part (nothing ever ends on it).
            {
                const uint32_t len16 = (uint32_t)(lo >> 8) & 0xffffu, nlen16 = (uint32_t)(lo >> 24) & 0xffffu;
                if (((uint32_t)lo & 0xfeu) == 0u && len16 != 0u && (len16 ^ nlen16) == 0xffffu && b + 5 + len16 <= src_len) {
                    const uint32_t i = atomicAdd(&nlocal, 1u);
                    if (i < kFindLocal) local[i] = (8ull * b) | (3ull << 62) | tag;          // bit 62: a stored block (light work)
                }
            }
            if constexpr (!PATTERNS) {
                // the cheap header tests for the eight bit positions of this byte at once, as bit masks over the window (bit k
                // = position k): BTYPE = 2 (bit k+1 clear, bit k+2 set), HLIT and HDIST not 30 or 31 (their upper four bits not
                // all set); the Kraft sum only for the positions left, one by one (a wavefront executes as many turns as
                // its busiest lane has positions left -- ~5 -- where the unrolled form executed the sum eight times)
                const uint32_t w = (uint32_t)lo;
                const uint32_t hl = (w >> 4) & (w >> 5) & (w >> 6) & (w >> 7), hd = (w >> 9) & (w >> 10) & (w >> 11) & (w >> 12);
                uint32_t left = (~w >> 1) & (w >> 2) & ~hl & ~hd & 0xffu;
                while (left) {
                    const unsigned k = (unsigned)__builtin_ctz(left);
                    left &= left - 1u;
                    const unsigned long long v = k ? (lo >> k) | (hi << (64 - k)) : lo;
                    const unsigned ncode = ((uint32_t)(v >> 13) & 15u) + 4u;
                    unsigned long long c = (lo >> (k + 17)) | (hi << (64 - (k + 17)));       // 57 bits: all 19 fields
                    c &= (1ull << (3 * ncode)) - 1ull;                                          // (19 fields are 57 bits: the table lookups below read 63)
                    unsigned sum = 0;
#pragma unroll
                    for (int g = 0; g < 7; ++g) sum += kraft9[(uint32_t)(c >> (9 * g)) & 511u];
                    if (sum != 128u) continue;
                    const uint32_t i = atomicAdd(&nlocal, 1u);
                    if (i < kFindLocal) local[i] = (8ull * b + k) | tag;
                }
            }
        }
        // 2048 positions per round leave ~2 survivors on real data; a round of adversarial data could fill the list
        __syncthreads();
        const uint32_t nl = nlocal;                     // the same value for every thread: nobody adds between the barriers
        __syncthreads();
        if (nl > kFindLocal / 4) flush();
    }
    flush();
}

// F1 over the streams of a finder pass (FindStreamDev / FindItemDev: inflate_dev_types.h): grid.x = work item, a range of one
// stream; the survivors of all streams go to ONE list, each tagged with its stream's index in the table (still one global
// atomic per workgroup and flush)
template <bool PATTERNS>
__global__ __launch_bounds__(256)
void find_headers_table_kernel(const FindStreamDev *__restrict__ streams, const FindItemDev *__restrict__ items,
                               unsigned long long *__restrict__ cand, uint32_t *__restrict__ ncand, uint32_t cap) {
    const FindItemDev it = items[blockIdx.x];
    const FindStreamDev s = streams[it.stream];
    find_headers_range<PATTERNS>(s.src, s.src_len, it.lo, it.hi < s.src_len ? it.hi : s.src_len,
                                 (unsigned long long)it.stream << kFindTagShift, cand, ncand, cap);
}

// F2.  One lane per survivor of F1: the whole dynamic header (inflate.c:814-917) and inflate_table's validity rules for the
// literal/length and the distance code (inftrees.c:104-137).  Those rules are statements about Kraft sums, so the code
// lengths are summed as they are decoded and never stored: a set is over-subscribed when its sum passes 1 (the lane
// leaves at once -- noise does so within a few symbols, which is what keeps this kernel short), complete when it ends at
// exactly 1, and an incomplete set is allowed only as ONE code of length 1 (inftrees.c:133-134: left > 0 needs max == 1).
// Per lane in LDS: the code-length code as a 128-entry direct table (length << 5 | symbol).  Survivors are appended to
// good[] (bit positions; the marker bit removed).
constexpr int kValLanes = 64;
__device__ __forceinline__ void validate_one(const uint8_t *__restrict__ src, unsigned long long src_len, const unsigned long long c0, uint8_t *T,
                             unsigned long long *__restrict__ good, uint32_t *__restrict__ ngood, uint32_t cap,
                             const unsigned long long tag);
// F2 over the tagged list of find_headers_table_kernel: a survivor's stream is looked up by its tag, which it keeps
__global__ __launch_bounds__(kValLanes)
void validate_headers_table_kernel(const FindStreamDev *__restrict__ streams, const unsigned long long *__restrict__ cand,
                                   const uint32_t *__restrict__ ncand, uint32_t cand_cap, unsigned long long *__restrict__ good,
                                   uint32_t *__restrict__ ngood, uint32_t cap) {
    __shared__ uint8_t tab[kValLanes][128];
    // the number of candidates is read here, not on the host: F1 -> F2 needs no round trip (the grid is fixed, each
    // workgroup takes every gridDim.x-th group of 64 candidates; a lane's candidates are independent of each other)
    const uint32_t n = *ncand < cand_cap ? *ncand : cand_cap;
    for (uint32_t i = blockIdx.x * kValLanes + threadIdx.x; i < n; i += gridDim.x * kValLanes) {
        const unsigned long long c = cand[i];
        const FindStreamDev s = streams[(c & kFindTagMask) >> kFindTagShift];
        validate_one(s.src, s.src_len, c & ~kFindTagMask, tab[threadIdx.x], good, ngood, cap, c & kFindTagMask);
    }
}
// the tables of a finder pass (and its zeroed counts) from the pinned host memory they were written to, `n` 16-byte words,
// one per lane: the device reads host memory over the bus, so the upload is a launch on the queue the scan follows on
__global__ __launch_bounds__(256)
void finder_tables_kernel(const uint4 *__restrict__ pinned, uint4 *__restrict__ tables, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) tables[i] = pinned[i];
}
// the first two bytes of every stream of the table (SUBBLOCK wants the first block's type), one lane each
__global__ __launch_bounds__(256)
void first_bytes_kernel(const FindStreamDev *__restrict__ streams, uint32_t n, uint16_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const FindStreamDev s = streams[i];
    out[i] = (uint16_t)((s.src_len > 0 ? (unsigned)load_u8(s.src) : 0u) | (s.src_len > 1 ? (unsigned)load_u8(s.src + 1) << 8 : 0u));
}

__device__ __forceinline__ void validate_one(const uint8_t *__restrict__ src, unsigned long long src_len, const unsigned long long c0, uint8_t *T,
                             unsigned long long *__restrict__ good, uint32_t *__restrict__ ngood, uint32_t cap,
                             const unsigned long long tag) {
    auto accept = [&]() {
        const uint32_t at = atomicAdd(ngood, 1u);
        if (at < cap) good[at] = (c0 & ~(1ull << 63)) | tag;      // (bit 62, "a stored block", stays; a batch: the stream's tag)
    };
    if (c0 >> 63) {                                       // behind a marker: taken as it is
        accept();
        return;
    }
    const unsigned long long bit = c0;
    unsigned long long w = bits_at_dev(src, src_len, bit + 3);
    const unsigned nlen = (unsigned)(w & 31) + 257, ndist = (unsigned)((w >> 5) & 31) + 1, ncode = (unsigned)((w >> 10) & 15) + 4;
    if (nlen > 286 || ndist > 30) return;
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
#pragma unroll
    for (int k = 0; k < 19; ++k) cl[k] = 0;
    unsigned long long pos = bit + 17;
    {
        const unsigned long long f = bits_at_dev(src, src_len, pos);
        for (unsigned k = 0; k < ncode; ++k) {
            const unsigned l = (unsigned)(f >> (3 * k)) & 7u;
            // cl[order[k]] = l without a dynamically indexed register array
#pragma unroll
            for (int s = 0; s < 19; ++s)
                if (order[k] == s) cl[s] = (uint8_t)l;
        }
        pos += 3ull * ncode;
    }
    if ((pos >> 3) + 8 > src_len) return;
    // canonical code of the code-length code -> direct table (complete: F1 checked the Kraft sum)
    unsigned count[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 19; ++s) {
#pragma unroll
        for (int l = 1; l < 8; ++l)
            if (cl[s] == l) ++count[l];
    }
    unsigned next[8];
    {
        unsigned code = 0;
#pragma unroll
        for (int l = 1; l < 8; ++l) {
            code = (code + count[l - 1]) << 1;
            next[l] = code;
        }
    }
#pragma unroll
    for (int s = 0; s < 19; ++s) {
        const unsigned l = cl[s];
        if (!l) continue;
        unsigned code = 0;
#pragma unroll
        for (int q = 1; q < 8; ++q)
            if (l == (unsigned)q) code = next[q]++;
        const unsigned rev = __builtin_bitreverse32(code) >> (32 - l);
        for (unsigned e = rev; e < 128; e += 1u << l) T[e] = (uint8_t)((l << 5) | (unsigned)s);
    }
    // Kraft sums in 1/32768; codes used and the longest code per set; the length the end-of-block symbol got
    unsigned have = 0, prev = 0, eob = 0;
    unsigned kraft[2] = {0, 0}, used[2] = {0, 0}, longest[2] = {0, 0};
    const unsigned total = nlen + ndist;
    // `rep` symbols from `have` on get code length l.  No loop over the run: the lanes of a wave execute the longest run
    // any of them has (138 zeros is common), and that loop was most of this kernel's time.
    auto put = [&](unsigned l, unsigned rep) -> bool {
        if (have <= 256u && 256u < have + rep) eob = l;
        if (l) {
            const unsigned n0 = have < nlen ? (rep < nlen - have ? rep : nlen - have) : 0u, n1 = rep - n0;
            kraft[0] += n0 * (32768u >> l);
            kraft[1] += n1 * (32768u >> l);
            used[0] += n0;
            used[1] += n1;
            if (n0 && l > longest[0]) longest[0] = l;
            if (n1 && l > longest[1]) longest[1] = l;
        }
        have += rep;
        return kraft[0] <= 32768u && kraft[1] <= 32768u;
    };
    unsigned long long hold = bits_at_dev(src, src_len, pos);
    unsigned spent = 0;                                   // bits of `hold` used up
    while (have < total) {
        if (spent > 48u) {                                // a symbol takes at most 7 + 7 bits
            pos += spent;
            if ((pos >> 3) + 8 > src_len) return;
            hold = bits_at_dev(src, src_len, pos);
            spent = 0;
        }
        const unsigned long long v = hold >> spent;
        const unsigned e = T[(unsigned)v & 127u];
        const unsigned nb = e >> 5, sym = e & 31u;
        spent += nb;
        if (sym < 16) {
            prev = sym;
            if (!put(sym, 1)) return;
            continue;
        }
        unsigned rep, val = 0;
        const unsigned long long x = v >> nb;
        if (sym == 16) {
            if (have == 0) return;
            val = prev;
            rep = 3 + (unsigned)(x & 3);
            spent += 2;
        } else if (sym == 17) {
            rep = 3 + (unsigned)(x & 7);
            spent += 3;
        } else {
            rep = 11 + (unsigned)(x & 127);
            spent += 7;
        }
        if (have + rep > total) return;
        prev = val;
        if (!put(val, rep)) return;
    }
    if ((((pos + spent) >> 3) + 8) > src_len) return;
    if (eob == 0) return;                                 // no end-of-block code (inflate.c:897-901)
    // literal/length set: complete, or the single code of length 1; distance set: the same, or no code at all
    if (kraft[0] != 32768u && !(used[0] == 1u && longest[0] == 1u)) return;
    if (kraft[1] != 32768u && !(used[1] == 0u || (used[1] == 1u && longest[1] == 1u))) return;
    accept();
}

// C.  grid.y = part on the chain: its symbols go to their place in the stream's symbol array.  A part's references count
// back from the PART's first byte; the context chain wants them counted from the SEGMENT's: a reference that lands inside
// an earlier part of the same segment is replaced by the symbol that part has there (itself possibly a reference: the
// loop follows it), one that lands in front of the segment is re-based.
__global__ __launch_bounds__(256)
void compact_parts_kernel(const PartCopy *__restrict__ parts, uint16_t *__restrict__ sym) {
    const uint32_t j0 = blockIdx.y;
    const PartCopy p = parts[j0];
    uint16_t *d = sym + p.dst;
    const bool rebase = p.dst != p.gstart;               // a segment's first part needs nothing
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, gsz = gridDim.x * blockDim.x;
    auto fix = [&](uint32_t v) -> uint32_t {             // a reference of this part, counted from the segment's first byte
        uint32_t j = j0;
        uint64_t base = p.dst;                           // first symbol of the part v counts back from
        for (;;) {
            const uint64_t k = 33024u - v;               // bytes in front of `base`, 1 .. 32768
            if (base - p.gstart < k) return 33024u - (uint32_t)(k - (base - p.gstart));      // in front of the segment
            const uint64_t g = base - k;                 // a symbol of an earlier part of this segment
            do --j; while (parts[j].dst > g);
            v = parts[j].src[g - parts[j].dst];
            if (v < 256u) return v;
            base = parts[j].dst;
        }
    };
    // 8 symbols (16 bytes) per lane where the destination allows it (slots are 16-byte aligned)
    const uint32_t lead = (uint32_t)((8u - (((uintptr_t)d >> 1) & 7u)) & 7u);
    for (uint32_t q = gid; q < lead && q < p.n; q += gsz) {
        uint32_t v = p.src[q];
        if (rebase && v >= 256u) v = fix(v);
        d[q] = (uint16_t)v;
    }
    if (p.n > lead) {
        const uint32_t chunks = (p.n - lead) >> 3;
        for (uint32_t c = gid; c < chunks; c += gsz) {
            const uint32_t at = lead + 8u * c;
            uint16_t v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = p.src[at + k];
            if (rebase) {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (v[k] >= 256u) v[k] = (uint16_t)fix(v[k]);
            }
            *reinterpret_cast<uint4 *>(d + at) = *reinterpret_cast<const uint4 *>(v);
        }
        for (uint32_t q = lead + 8u * chunks + gid; q < p.n; q += gsz) {
            uint32_t v = p.src[q];
            if (rebase && v >= 256u) v = fix(v);
            d[q] = (uint16_t)v;
        }
    }
}

// What the zng_rocm_inflate_large_last_* getters report: the calling thread's last call.  An entry point counts in a value of
// its own (or takes inflate_large_try's answer) and publishes it here once, at its exit; nothing below an entry point writes it.
struct LargeCounters {
    int      parts = 0;
    int      subparts = 0;                              // of them, parts that began inside a block
    int      substarts = 0;                             // SUBBLOCK: sub-starts placed (the sync kernel's boundaries, deduplicated)
    int      pieces = 0;                                // pieces: device passes of the call
    uint64_t host_bytes = 0;                            // pieces: compressed bytes the sequential decoder took
};
static thread_local LargeCounters t_last;
static thread_local IndexSink *t_index_sink = nullptr;  // an index is being built (inflate_dev.h); null outside such a call
#ifdef ZR_INFLATE_STATS
static std::vector<unsigned long long> g_dbg_starts;     // diagnostic builds: the last call's part starts and result words
static std::vector<uint32_t> g_dbg_res;
#endif

// why the device path handed the stream to the sequential decoder (readable through zng_rocm_last_error())
static int why(const char *reason) {
    set_error("inflate_large: sequential decoder (%s)", reason);
    return 0;
}
// the same for a chain walk that failed: its reason, or -- a part's own result -- which part (of `np`; starts, keys or null,
// result words and job entries are the stream's own) and what it said; `job` < 0: not a batch
static int why_chain(const Chain &c, size_t np, const unsigned long long *starts, const unsigned long long *keys, const uint32_t *res,
                     const InflateJobDev *jobs, long job) {
    if (c.bad_part >= np) return why(c.reason);
    char of[32] = "";
    if (job >= 0) snprintf(of, sizeof of, "job %ld, ", job);
    const size_t cur = c.bad_part;
    const uint32_t *r = &res[8 * cur];                    // (key, where the part began: 0 a block start, 1 fixed, H + 2 dynamic)
    set_error("inflate_large: sequential decoder (%spart %zu of %zu at bit %llu, key %llu: message %u \"%s\", %u symbols of %llu, "
              "ended on %d)", of, cur, np, starts[cur], keys ? keys[cur] : 0ull, r[4], zng_rocm_inflate_message(r[4]), r[0],
              (unsigned long long)jobs[cur].out_cap, (int)r[6]);
    return 0;
}

IndexSink *inflate_index_sink() { return t_index_sink; }
void inflate_index_sink_set(IndexSink *sink) { t_index_sink = sink; }

// the part counters of the calling thread back to 0 (a call begins; or "the sequential decoder did it": inflate_resolve.hip)
void inflate_large_forget_parts() { t_last.parts = t_last.subparts = t_last.substarts = 0; }

// ---- the pass -----------------------------------------------------------------------------------------------------------
// One stream of a device pass: what its finder found, and what pass_run made of it.
struct PassStream {
    // in
    const uint8_t *d_src = nullptr;
    size_t         src_len = 0;
    const uint8_t *d_window = nullptr;
    uint32_t       window_len = 0;
    uint8_t       *d_dst = nullptr;
    size_t         dst_cap = 0;
    unsigned long long start_bit = 0;                     // the stream begins at this bit of d_src (blocks mode, pieces)
    size_t         scan_lo = 0;                           // the finder scans from this byte of d_src on: the byte start_bit lies in
                                                          // (pieces: the buffer may begin in front of the piece, PiecePass)
    unsigned long long key0 = 0;                         // pieces: the first start may lie inside a block itself (PiecePass)
    uint16_t       b0 = 0;                                // the two bytes at scan_lo, where start_bit lies (SUBBLOCK, when F1 + F2 ran)
    bool           patterns_do = false;                   // the byte patterns alone cut the stream
    std::vector<unsigned long long> starts;               // sorted (thin_starts)
    size_t         heavy = 1;
    long           job = -1;                              // a batch: its index in the caller's array, for why_chain
    // out
    bool           left = false;                          // not done here (set on entry: not taken up at all); the reason went
                                                          // through why() / why_chain()
    int            status = 0;                            // 1: chain.produced bytes are at d_dst; -5: they do not fit dst_cap and
                                                          // nothing was written (the chain's counts hold either way)
    Chain          chain;                                 // parts: chain.copies.size(), subparts: chain.subparts
    size_t         counted_parts = 0;                     // the counting mode: genuine parts (there are no copies); chain holds
                                                          // produced / end_bit / final alone
    size_t         substarts = 0;                         // SUBBLOCK: sub-starts placed (deduplicated)
    std::vector<unsigned long long> keys;                 // SUBBLOCK, per start: 0 a block start, 1 inside a fixed-code block,
                                                          // H + 2 inside the dynamic block at H
    size_t         pbase = 0;                             // its first part in the launch's tables
    const uint32_t *res = nullptr;                        // its parts' result words in the pinned mirror, once they ran (they
                                                          // stay until the workspace's next pass)
};
static void leave(PassStream &s, const char *reason) {
    s.left = true;
    why(reason);
}

// ---- the finder ---------------------------------------------------------------------------------------------------------
// One finder pass over the streams `which` (indices into ss and good), each from its scan_lo on: the patterns alone, or F1 +
// F2 (and, `bytes`, every stream's first two scanned bytes).  What is scanned, the caps and whose a survivor is are find_plan's
// and find_demux's (inflate_large_plan.h).  Fills good[..] with each stream's survivors, as bit positions of its d_src,
// sorted; when the lists cannot be had the streams leave the device path.  The tables (streams | items | the counts, zero) go
// up from the pinned scratch, which is free -- every pass ends in a synchronisation; one copy down and one synchronisation
// (a second of each when the list is longer than what comes back with the counts).
// What a caller with ONE stream wants to know besides (inflate_large_try keeps its own answers to both):
struct FindOne {
    uint32_t n_f1 = ~0u;                                  // F1's survivors, when F1 + F2 ran over the one stream
    int      no_room = ZNG_ROCM_OK;                       // the scratch reservation's error, when that is why the streams left
};
static int find_pass(Workspace *ws, std::vector<PassStream> &ss, std::vector<std::vector<unsigned long long>> &good,
                     const std::vector<size_t> &which, bool patterns, bool bytes, hipStream_t st, FindOne *one = nullptr) {
    const size_t ns = which.size();
    if (!ns) return ZNG_ROCM_OK;
    std::vector<uint64_t> lens(ns);
    for (size_t k = 0; k < ns; ++k) lens[k] = ss[which[k]].src_len - ss[which[k]].scan_lo;
    const FindPlan P = find_plan(lens.data(), ns);
    const uint32_t cap1 = P.cap1, cap2 = P.cap2, first = P.first;
    // streams | items | counts | first bytes | survivors on both sides (the pinned side: the first survivors alone), so that
    // streams | items | counts go up in one copy and counts | first bytes | the first survivors come down in one; behind
    // them, on the device, F1's candidates
    TableLayout dl;
    const size_t o_tab = dl.add(ns * sizeof(FindStreamDev)), o_items = dl.add(P.nitems * sizeof(FindItemDev)), o_n = dl.add(64),
                 o_b0 = dl.add(ns * 2);
    TableLayout hl = dl;
    const size_t o_good = dl.add((size_t)cap2 * 8), o_cand = dl.add((size_t)cap1 * 8), o_hgood = hl.add((size_t)first * 8);
    uint8_t *fp = nullptr, *hp = nullptr;
    auto out = [&](const char *reason) {
        for (size_t w : which) ss[w].left = true;
        return why(reason);
    };
    int room = scratch_reserve(ws, kScrLargeCand, dl.bytes, false, (void **)&fp);
    if (room == ZNG_ROCM_OK) room = scratch_reserve(ws, kScrLargeCandHost, hl.bytes, true, (void **)&hp);
    if (room != ZNG_ROCM_OK) {
        if (one) one->no_room = room;
        return out("no room for the finder's candidates");
    }
    FindStreamDev *d_tab = (FindStreamDev *)(fp + o_tab), *h_tab = (FindStreamDev *)(hp + o_tab);
    FindItemDev *d_items = (FindItemDev *)(fp + o_items);
    uint32_t *d_n = (uint32_t *)(fp + o_n), *n12 = (uint32_t *)(hp + o_n);       // [0] survivors of F1, [1] of F2 (or the patterns)
    uint16_t *d_b0 = (uint16_t *)(fp + o_b0), *h_b0 = (uint16_t *)(hp + o_b0);
    unsigned long long *d_cand = (unsigned long long *)(fp + o_cand), *d_good = (unsigned long long *)(fp + o_good);
    unsigned long long *h_good = (unsigned long long *)(hp + o_hgood);
    for (size_t k = 0; k < ns; ++k) h_tab[k] = FindStreamDev{ss[which[k]].d_src + ss[which[k]].scan_lo, lens[k]};
    find_items(lens.data(), ns, P.share, (FindItemDev *)(hp + o_items));
    n12[0] = n12[1] = 0;
    // streams | items | the two counts, zero: fetched by a kernel (o_n + 256 bytes, which both sides have: every table is a
    // multiple of 256).  The stream is idle here, and a copy on the copy engine in front of the scan cost each pass 10 us
    // more than the fill kernel that zeroed the counts of the one-stream finder.
    hipLaunchKernelGGL(finder_tables_kernel, dim3((unsigned)((o_n + 256) / 16 + 255) / 256), dim3(256), 0, st, (const uint4 *)hp, (uint4 *)fp,
                       (uint32_t)((o_n + 256) / 16));
    ZR_HIP(hipGetLastError());
    if (patterns) {
        hipLaunchKernelGGL(find_headers_table_kernel<true>, dim3((unsigned)P.nitems), dim3(256), 0, st, d_tab, d_items, d_good, d_n + 1, cap2);
        ZR_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(find_headers_table_kernel<false>, dim3((unsigned)P.nitems), dim3(256), 0, st, d_tab, d_items, d_cand, d_n, cap1);
        ZR_HIP(hipGetLastError());
        hipLaunchKernelGGL(validate_headers_table_kernel, dim3(8192), dim3(kValLanes), 0, st, d_tab, d_cand, d_n, cap1, d_good, d_n + 1, cap2);
        ZR_HIP(hipGetLastError());
        if (bytes) {
            hipLaunchKernelGGL(first_bytes_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st, d_tab, (uint32_t)ns, d_b0);
            ZR_HIP(hipGetLastError());
        }
    }
    // the counts, the first bytes and (what is almost always all of) the list in one copy and one round trip
    ZR_HIP(hipMemcpyAsync(n12, d_n, (o_good - o_n) + (size_t)first * 8, hipMemcpyDeviceToHost, st));
    ZR_HIP(hipStreamSynchronize(st));
    if (one && ns == 1 && !patterns) one->n_f1 = n12[0];
    if (n12[0] > cap1 || n12[1] > cap2) {
        // One stream's payload can hold more places that pass for a block start than the whole pass has room for (a stored
        // block full of 00 00 ff ff).  That is that stream's trouble, not its neighbours': each half of the streams on its
        // own, down to the stream that has them -- which leaves.
        if (ns == 1)
            return out(n12[0] > cap1 ? "far more candidates in the stream than a deflate stream has"
                                     : "far more valid block headers than a deflate stream has");
        const std::vector<size_t> lower(which.begin(), which.begin() + ns / 2), upper(which.begin() + ns / 2, which.end());
        if (int rc = find_pass(ws, ss, good, lower, patterns, bytes, st)) return rc;
        return find_pass(ws, ss, good, upper, patterns, bytes, st);
    }
    const uint32_t n2 = n12[1];
    std::vector<unsigned long long> rest;
    if (n2 > first) {
        rest.resize(n2 - first);
        ZR_HIP(hipMemcpyAsync(rest.data(), d_good + first, (size_t)(n2 - first) * 8, hipMemcpyDeviceToHost, st));
        ZR_HIP(hipStreamSynchronize(st));
    }
    std::vector<std::vector<unsigned long long>> per = find_demux(h_good, std::min(n2, first), rest.data(), rest.size(), ns);
    for (size_t k = 0; k < ns; ++k) {
        PassStream &s = ss[which[k]];
        if (bytes && !patterns) s.b0 = h_b0[k];
        for (unsigned long long &b : per[k]) b += 8ull * s.scan_lo;
        good[which[k]].swap(per[k]);
    }
    return ZNG_ROCM_OK;
}

// The finder, for the streams `scan` (indices into ss and good) of a pass: the byte patterns (sync markers, byte-aligned
// stored blocks) for every stream; when they leave no 128 KiB of a stream's compressed bytes without a start, that is all the
// cutting it needs, and the search of every bit position (F1's main loop) and F2 run for the other streams alone -- 1.3 of
// 9.4 ms for the 256 MiB cfg3 stream of this library's level-6 class.  `sub`: with F1 + F2 come the stream's first two bytes.
// A stream whose lists cannot be had has left the device path; thinning the lists into starts is the caller's.
// The scan begins at the byte the stream's first bit lies in, so the two bytes handed back (b0) hold the first block's header
// at bit start_bit & 7.  Every caller has it so -- pieces pass start_bit = bit - 8 base and scan_lo = (bit >> 3) - base, blocks
// mode start_bit < 8 and scan_lo = 0 -- and anything else is refused before a launch.
static int find_starts(Workspace *ws, std::vector<PassStream> &ss, std::vector<std::vector<unsigned long long>> &good,
                       const std::vector<size_t> &scan, bool sub, hipStream_t st, FindOne *one = nullptr) {
    for (size_t k : scan) {
        if ((ss[k].start_bit >> 3) != ss[k].scan_lo) {
            set_error("inflate_large: the finder's scan does not begin at the byte of the stream's first bit");
            return ZNG_ROCM_EINVAL;
        }
    }
    if (int rc = find_pass(ws, ss, good, scan, true, false, st, one)) return rc;
    std::vector<size_t> full;
    for (size_t k : scan) {
        PassStream &s = ss[k];
        if (s.left) continue;
        s.patterns_do = good[k].size() <= patterns_first(s.src_len - s.scan_lo) && patterns_cut(good[k], s.start_bit, 8ull * s.src_len);
        if (!s.patterns_do) full.push_back(k);
    }
    return find_pass(ws, ss, good, full, false, sub, st, one);
}

// pass_run's counting mode (zng_rocm_uncompress_large_size_dev / _sizes_dev): the parts of the streams `on` -- `np` together,
// placed by pass_run -- through inflate_size_parts_kernel (inflate_large_size.hip) in ONE launch, and one walk per stream
// (inflate_large_size_plan.h).  A counting part has no slot, so nothing overflows and nothing runs again; the scratch is
// jobs | starts | results and nothing else.  A stream whose walk fails leaves the pass: the caller sizes it whole, with the
// decoder's verdict.  (A stream of one part is a chain of one: what the finder could not cut, see pass_run.)
static int count_parts(Workspace *ws, std::vector<PassStream> &ss, const std::vector<size_t> &on, size_t np, hipStream_t st,
                       int *launches) {
    const PartTables T = part_tables(np, false, false, 0);
    uint8_t *sp = nullptr, *hq = nullptr;
    if (scratch_reserve(ws, kScrLargeParts, T.device_bytes, false, (void **)&sp) != ZNG_ROCM_OK ||
        scratch_reserve(ws, kScrLargePartsHost, T.mirror_bytes, true, (void **)&hq) != ZNG_ROCM_OK) {
        for (size_t k : on) ss[k].left = true;
        return why("no room for the part tables");
    }
    InflateJobDev *pj = (InflateJobDev *)(hq + T.jobs);
    unsigned long long *h_starts = (unsigned long long *)(hq + T.starts);
    uint32_t *res = (uint32_t *)(hq + T.res);
    for (size_t k : on) {
        const PassStream &s = ss[k];
        const size_t n = s.starts.size();
        std::copy(s.starts.begin(), s.starts.end(), h_starts + s.pbase);
        // (a part that is not its stream's first has all the history a distance can reach: inflate_size_parts_kernel)
        for (size_t i = 0; i < n; ++i)
            pj[s.pbase + i] = InflateJobDev{s.d_src, nullptr, s.src_len, 0, i == 0 ? s.window_len : 32768u, (uint32_t)(s.pbase + n)};
    }
    ZR_HIP(hipMemcpyAsync(sp, hq, T.up_bytes, hipMemcpyHostToDevice, st));       // jobs | starts in one copy
    if (int rc = launch_inflate_size_parts_device((const InflateJobDev *)(sp + T.jobs), np, (const unsigned long long *)(sp + T.starts),
                                                  (uint32_t *)(sp + T.res), st))
        return rc;
    ++*launches;
    ZR_HIP(hipMemcpyAsync(res, sp + T.res, np * 32, hipMemcpyDeviceToHost, st));
    ZR_HIP(hipStreamSynchronize(st));
    for (size_t k : on) {
        PassStream &s = ss[k];
        s.res = res + 8 * s.pbase;
        SizeChain c;
        if (!walk_size_chain(res, s.pbase, s.starts.size(), s.starts.data(), s.window_len, c)) {
            // (readable through zng_rocm_last_error() until the stream's own verdict replaces it)
            if (c.bad_part < s.starts.size())
                set_error("inflate_large: sized whole by one wavefront (job %ld, part %zu of %zu at bit %llu: message %u \"%s\")", s.job,
                          c.bad_part, s.starts.size(), s.starts[c.bad_part], s.res[8 * c.bad_part + 4],
                          zng_rocm_inflate_message(s.res[8 * c.bad_part + 4]));
            else
                set_error("inflate_large: sized whole by one wavefront (job %ld: %s)", s.job, c.reason);
            s.left = true;
            continue;
        }
        s.status = 1;
        s.chain.produced = c.produced;
        s.chain.end_bit = c.end_bit;
        s.chain.final = true;
        s.counted_parts = c.parts;
    }
    return ZNG_ROCM_OK;
}

// The device pass over the streams `ss` whose starts are found, ONE of each step for all of them: the SUBBLOCK sync launch,
// one part launch over the parts of all streams (each stream's starts together; a part looks for its end among its own
// stream's only: InflateJobDev::flags) and one more for the parts whose slot was too small, one chain walk per stream on
// the host, one compaction and one resolve over a symbol array that holds the streams one behind the other (symbol_tables).
// So the long parts of one stream run under the short parts of the others, and the host round trips between the kernels
// are paid once.  The rules are inflate_large_plan.h's; here are the launches, the copies and the scratch.
// `sub` (ZNG_ROCM_INFLATE_SUBBLOCK): starts inside blocks too -- guesses in the gaps the finder leaves, the sync kernel's dry
// parse, hand-offs on the chain (inflate_dev.hip, inflate_streams_kernel<..., SUB>).  `blocks` (the streaming hook; never
// with `sub`): input that ends inside a block is no irregularity -- the chain stops at the first part that ran out of
// input and that part's complete blocks (its marks) are kept.  `pp`: a piece (PiecePass); its caps bound the scratch, and a
// pass over one of them sets pp->halve.  `blocks` and `pp` take ONE stream.
// A stream the pass cannot do leaves it (PassStream::left); the others do not notice.  The streams from *taken on were not
// taken up: their parts and those in front of them would be more than one launch (and the compaction grid) takes.
// *launches counts the part launches.  Negative returns are HIP and allocation errors of the whole pass.
// `counting` (never with `sub`, `blocks` or `pp`): the sizes alone -- the same streams are taken up and placed, and
// count_parts does the rest: no slots, no rerun, no compaction, no resolve.
static int pass_run(Workspace *ws, std::vector<PassStream> &ss, bool sub, bool blocks, PiecePass *pp, hipStream_t st, size_t *taken,
                    int *launches, bool counting = false) {
    *taken = ss.size();
    if (((blocks || pp) && ss.size() != 1) || (sub && blocks) || (counting && (sub || blocks || pp))) {
        set_error("inflate_large: blocks mode and pieces take one stream, blocks mode no sub-starts, the counting mode neither");
        return ZNG_ROCM_EINVAL;
    }
    const size_t cus = (size_t)ctx()->cus;
    // ---- SUBBLOCK: guesses in the gaps (plan_sub_regions), with a step that fills the chip once per PASS (a stream never
    // gets a coarser step than a sixteenth of itself: a small stream among large ones is still cut).
    // No guesses when the pattern pass alone cut the stream: its writer (this library's level-6 class, pigz) already closed
    // a block every few tens of KiB, and that kernel is bound by throughput, not by a long part.  Dynamic
    // blocks are split while the Huffman starts found are no more than the chip's resident parts (12 per CU): the 256 MiB
    // CPython level-6 stream (about 2700 of them) takes 10.3 ms split against 10.6 ms whole; with more
    // starts than slots the chip is full without splitting. ----
    if (sub) {
        uint64_t pass_bits = 0;
        size_t pass_heavy = 0;
        for (const PassStream &s : ss) {
            if (s.left) continue;
            pass_bits += 8ull * s.src_len - s.start_bit;
            pass_heavy += s.heavy;
        }
        const unsigned long long pass_step = std::max<unsigned long long>(kSubMinStep, pass_bits / (kSubPerSlot * 12ull * cus));
        const uint32_t split_dynamic = pass_heavy <= 12u * cus ? 1u : 0u;
        std::vector<SubRegionDev> regions;
        std::vector<std::pair<uint32_t, uint32_t>> span(ss.size(), {0u, 0u});      // a stream's guess slots: two per guess
        uint32_t nguess = 0;
        for (size_t k = 0; k < ss.size(); ++k) {
            PassStream &s = ss[k];
            if (s.left) continue;
            s.keys.assign(s.starts.size(), 0ull);
            s.keys[0] = s.key0;
            span[k].first = nguess;
            const unsigned long long own = 8ull * s.src_len - s.start_bit;
            const unsigned long long step = std::max<unsigned long long>(kSubMinStep, std::min<unsigned long long>(pass_step, own / 16));
            const bool fixed_first = !s.patterns_do && (s.key0 == 1u || (s.key0 == 0u && (((unsigned)s.b0 >> ((s.start_bit & 7u) + 1u)) & 3u) == 1u));
            // (every region carries its own stream: the sync kernel's launch names none)
            if (!s.patterns_do)
                plan_sub_regions(s.starts, 8ull * s.src_len, step, split_dynamic, fixed_first, s.key0, s.d_src, s.src_len, regions, nguess);
            span[k].second = nguess;
        }
        if (nguess) {
            TableLayout l;
            l.add(regions.size() * sizeof(SubRegionDev));
            const size_t reg_b = l.bytes, out_b = (size_t)nguess * 16;
            uint8_t *dp = nullptr, *hp2 = nullptr;
            if (pp && reg_b + out_b > piece_cap_sub(pp->q)) {
                pp->halve = true;
                leave(ss[0], "the piece's sub-starts need more scratch than its cap");
            } else if (scratch_reserve(ws, kScrLargeSub, reg_b + out_b, false, (void **)&dp) == ZNG_ROCM_OK &&
                       scratch_reserve(ws, kScrLargeSubHost, reg_b + out_b, true, (void **)&hp2) == ZNG_ROCM_OK) {
                // (without the scratch: no sub-starts, the streams go on with the starts found)
                std::copy(regions.begin(), regions.end(), (SubRegionDev *)hp2);
                unsigned long long *d_bit = (unsigned long long *)(dp + reg_b), *h_bit = (unsigned long long *)(hp2 + reg_b);
                ZR_HIP(hipMemcpyAsync(dp, hp2, regions.size() * sizeof(SubRegionDev), hipMemcpyHostToDevice, st));
                if (int rc = launch_subblock_sync(nullptr, 0, (const SubRegionDev *)dp, regions.size(), d_bit, d_bit + nguess, st)) return rc;
                ZR_HIP(hipMemcpyAsync(h_bit, d_bit, out_b, hipMemcpyDeviceToHost, st));
                ZR_HIP(hipStreamSynchronize(st));
                for (size_t k = 0; k < ss.size(); ++k) {
                    PassStream &s = ss[k];
                    if (s.left || span[k].first == span[k].second) continue;
                    s.substarts = merge_sub_starts(s.starts, s.keys, h_bit, h_bit + nguess, span[k].first, span[k].second, s.start_bit,
                                                   s.src_len, s.heavy);
                }
            }
        }
    }
    // ---- the pass's parts: each stream's together, the streams one behind the other ---------------------------------------
    size_t np = 0, heavy = 0;
    std::vector<size_t> on;                               // streams in the part launch
    for (size_t k = 0; k < ss.size(); ++k) {
        PassStream &s = ss[k];
        if (s.left) continue;
        // (the counting mode: a stream that is not cut -- not scanned, too few starts, too many -- is ONE part from its first
        // bit, which costs what sizing it whole costs and, when the stream is sound, is the answer)
        if (s.starts.size() < 4) {
            if (!counting) {
                leave(s, "fewer than four block starts found");
                continue;
            }
            s.starts.assign(1, s.start_bit);
        }
        if (counting && on.empty() && s.starts.size() > kPieceMaxParts) s.starts.assign(1, s.start_bit);
        if (np + s.starts.size() > kPieceMaxParts) {      // more parts than one launch (and the compaction grid's y) takes
            if (on.empty()) {                             // one stream alone has them: not a stream for the device path
                if (pp) pp->halve = true;
                leave(s, "more parts in one stream than one launch takes");
                continue;
            }
            *taken = k;                                   // this stream and the ones behind it: the next pass
            break;
        }
        s.pbase = np;
        np += s.starts.size();
        heavy += s.heavy;
        on.push_back(k);
    }
    if (on.empty()) return ZNG_ROCM_OK;
    if (counting) return count_parts(ws, ss, on, np, st, launches);
    auto all_out = [&](const char *reason) {
        for (size_t k : on) ss[k].left = true;
        return why(reason);
    };
    const bool many = heavy > 12u * cus;
    std::vector<uint64_t> slot_off(np + 1, 0), part_bytes(np, 0);
    // (slot_slack sees the parts of the whole pass: the slack of all slots together is what has to stay in bounds)
    for (size_t k : on)
        slot_caps(ss[k].starts.data(), ss[k].starts.size(), 8ull * ss[k].src_len, slot_slack(np, pp), &slot_off[ss[k].pbase],
                  &part_bytes[ss[k].pbase]);
    const PartTables T = part_tables(np, sub, blocks, slot_off[np]);
    // what comes back from and goes up to the device between the launches passes through pinned memory (pageable copies of
    // these few hundred KiB were a good part of the 0.55 ms the host spends between the kernels of a 256 MiB stream)
    uint8_t *sp = nullptr, *hq = nullptr;
    if (scratch_reserve(ws, kScrLargeParts, T.device_bytes, false, (void **)&sp) != ZNG_ROCM_OK) return all_out("no room for the part slots");
    if (scratch_reserve(ws, kScrLargePartsHost, T.mirror_bytes, true, (void **)&hq) != ZNG_ROCM_OK)
        return all_out("no pinned memory for the part tables");
    InflateJobDev *d_jobs = (InflateJobDev *)(sp + T.jobs), *pj = (InflateJobDev *)(hq + T.jobs);
    unsigned long long *d_starts = (unsigned long long *)(sp + T.starts), *h_starts = (unsigned long long *)(hq + T.starts);
    uint32_t *d_res = (uint32_t *)(sp + T.res), *res = (uint32_t *)(hq + T.res);
    uint16_t *d_slots = (uint16_t *)(sp + T.slots);
    uint32_t *d_extra = (uint32_t *)(sp + T.extra), *extra = (uint32_t *)(hq + T.extra);     // marks (blocks mode) or side words (SUBBLOCK)
    for (size_t k : on) {
        const PassStream &s = ss[k];
        const size_t n = s.starts.size();
        std::copy(s.starts.begin(), s.starts.end(), h_starts + s.pbase);
        if (sub) std::copy(s.keys.begin(), s.keys.end(), (unsigned long long *)(hq + T.keys) + s.pbase);
        for (size_t i = 0; i < n; ++i)
            pj[s.pbase + i] = InflateJobDev{s.d_src, (uint8_t *)(d_slots + slot_off[s.pbase + i]), s.src_len,
                                            slot_off[s.pbase + i + 1] - slot_off[s.pbase + i], i == 0 ? s.window_len : 32768u,
                                            (uint32_t)(s.pbase + n)};
    }
    auto launch_parts = [&]() -> int {
        if (int rc = launch_inflate_parts_device(d_jobs, np, d_res, d_starts, many, st, blocks ? d_extra : nullptr, sub ? d_extra : nullptr))
            return rc;
        ++*launches;
        ZR_HIP(hipMemcpyAsync(res, d_res, np * 4 * T.res_words, hipMemcpyDeviceToHost, st));
        ZR_HIP(hipStreamSynchronize(st));
        return ZNG_ROCM_OK;
    };
    ZR_HIP(hipMemcpyAsync(sp, hq, T.up_bytes, hipMemcpyHostToDevice, st));       // jobs | starts (| keys) in one copy
    if (int rc = launch_parts()) return rc;
    // parts whose slot was too small, of all streams: ONE launch more, with retry_cap's room (plan_retry).  A stream whose
    // parts want more than its limit leaves the pass; the others' parts are run again without it.
    std::vector<uint16_t *> slot_ptr(np);
    for (size_t i = 0; i < np; ++i) slot_ptr[i] = d_slots + slot_off[i];
    {
        std::vector<std::pair<size_t, size_t>> spans;
        for (size_t k : on) spans.emplace_back(ss[k].pbase, ss[k].starts.size());
        RetryPlan retry = plan_retry(res, spans, part_bytes.data(), pp ? piece_cap_retry(pp->q) : 24ull << 30);
        // A piece over its cap: most of what asks may be noise that no chain reaches (decoy stored headers in a stored block's
        // payload, each promising 65535 bytes to a slot whose slack the piece bounds).  The full parts ON the chain run again
        // one at a time, each found by following the links so far (first_full_on_chain), in one buffer of the cap's size,
        // while turns and room last; the stream leaves as before when they do not, or when the chain breaks.
        if (pp && !retry.over.empty()) {
            retry.over.clear();
            PassStream &s = ss[on[0]];
            const size_t i0 = s.pbase, i1 = s.pbase + s.starts.size();
            uint8_t *capp = nullptr;
            uint64_t used = 0;
            bool over = false;
            for (int turn = 0;; ++turn) {
                const size_t i = first_full_on_chain(res, i0, i1);
                if (i == i1) break;
                const uint64_t cap = i < i1 ? retry_cap(part_bytes[i]) : 0;
                over = i > i1 || turn == kChainRetryTurns || (used + cap) * 2 > piece_cap_retry(pp->q) ||
                       (!capp && scratch_reserve(ws, kScrLargeRetry, piece_cap_retry(pp->q), false, (void **)&capp) != ZNG_ROCM_OK);
                if (over) break;
                for (size_t k = 0; k < np; ++k) pj[k].out_cap = 0;
                slot_ptr[i] = (uint16_t *)capp + used;
                pj[i].out = (uint8_t *)slot_ptr[i];
                pj[i].out_cap = cap;
                used += cap;
                ZR_HIP(hipMemcpyAsync(d_jobs, pj, np * sizeof(InflateJobDev), hipMemcpyHostToDevice, st));
                if (int rc = launch_parts()) return rc;
                // full again: its room goes by the bytes up to the next START, and a noise start a few bytes behind a genuine one
                // makes that room small while the block runs on past it -- as in plan_retry's one rerun, such a stream leaves
                if (res[8 * i + 4] == kMsgOutFull) {
                    over = true;
                    break;
                }
            }
            if (over) retry.over.push_back(0);
        }
        for (size_t o : retry.over) {
            if (pp) pp->halve = true;
            leave(ss[on[o]], pp ? "the piece's parts above a ratio of 64 need more scratch than its cap"
                                : "parts with a ratio above 64 need more scratch than is reasonable");
        }
        uint8_t *bigp = nullptr;
        if (!retry.again.empty() && scratch_reserve(ws, kScrLargeRetry, retry.total * 2, false, (void **)&bigp) != ZNG_ROCM_OK) {
            for (size_t k : on)                           // (the streams that asked leave; the others are complete)
                for (size_t i : retry.again)
                    if (i >= ss[k].pbase && i < ss[k].pbase + ss[k].starts.size()) ss[k].left = true;
            why("no room for the parts with a ratio above 64");
        } else if (!retry.again.empty()) {
            for (size_t i = 0; i < np; ++i) pj[i].out_cap = 0;
            for (size_t a = 0; a < retry.again.size(); ++a) {
                const size_t i = retry.again[a];
                slot_ptr[i] = (uint16_t *)bigp + retry.off[a];
                pj[i].out = (uint8_t *)slot_ptr[i];
                pj[i].out_cap = retry.cap[a];
            }
            ZR_HIP(hipMemcpyAsync(d_jobs, pj, np * sizeof(InflateJobDev), hipMemcpyHostToDevice, st));
            if (int rc = launch_parts()) return rc;
        }
    }
    // ---- one chain per stream from its first part; a stream whose walk fails leaves the pass -------------------------------
    std::vector<SymStream> placed;
    std::vector<BatchStream> wins;
    for (size_t k : on) {
        PassStream &s = ss[k];
        s.res = res + 8 * s.pbase;
        if (s.left) continue;
        const unsigned long long *keys = sub ? s.keys.data() : nullptr;
        if (!walk_chain(res, extra, extra, slot_ptr.data(), s.pbase, s.starts.size(), s.starts.data(), keys, s.window_len, s.src_len, sub,
                        blocks, pp, s.chain)) {
            why_chain(s.chain, s.starts.size(), s.starts.data(), keys, s.res, pj + s.pbase, s.job);
            s.left = true;
            continue;
        }
        s.status = s.chain.produced > s.dst_cap ? -5 : 1;  // (too small: this stream's trouble alone, nothing of it is written)
        if (s.status == 1 && s.chain.produced) {
            placed.push_back(SymStream{&s.chain.copies, s.chain.produced, (uint64_t)(uintptr_t)s.d_dst});
            wins.push_back(BatchStream{0, s.window_len ? s.d_window : nullptr, s.window_len});
        }
    }
    // ---- the streams one behind the other in ONE symbol array; compaction, resolve, translate ----------------------------
    if (placed.empty()) return ZNG_ROCM_OK;
    const SymTables Y = symbol_tables(placed);
    for (size_t w = 0; w < wins.size(); ++w) wins[w].v_start = placed[w].v;
    const size_t nsegs = Y.seg_dst.size();                // (and Y.copies.size() <= np <= kPieceMaxParts, the grid's y limit)
    TableLayout l;
    const size_t o_segs = l.add(Y.segs.size() * 8), o_sd = l.add(nsegs * 8), o_se = l.add(nsegs * 8),
                 o_win = l.add(wins.size() * sizeof(BatchStream)), o_cp = l.add(Y.copies.size() * sizeof(PartCopy)), o_sym = l.bytes;
    uint8_t *yp = nullptr;
    if (scratch_reserve(ws, kScrLargeSym, o_sym + ((size_t)Y.v_end + 64) * 2, false, (void **)&yp) != ZNG_ROCM_OK) {
        for (size_t k : on)
            if (!ss[k].left && ss[k].status == 1 && ss[k].chain.produced) ss[k].left = true;     // (the -5 streams keep their status)
        return why("no room for the symbols");
    }
    uint16_t *sym = (uint16_t *)(yp + o_sym);
    // (the five tables go up in ONE copy: each copy from pageable memory costs the host tens of microseconds)
    std::vector<uint8_t> up(o_sym);
    memcpy(up.data() + o_segs, Y.segs.data(), Y.segs.size() * 8);
    memcpy(up.data() + o_sd, Y.seg_dst.data(), nsegs * 8);
    memcpy(up.data() + o_se, Y.seg_end.data(), nsegs * 8);
    memcpy(up.data() + o_win, wins.data(), wins.size() * sizeof(BatchStream));
    memcpy(up.data() + o_cp, Y.copies.data(), Y.copies.size() * sizeof(PartCopy));
    ZR_HIP(hipMemcpyAsync(yp, up.data(), up.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(compact_parts_kernel, dim3(16, (unsigned)Y.copies.size()), dim3(256), 0, st, (const PartCopy *)(yp + o_cp), sym);
    ZR_HIP(hipGetLastError());
    if (int rc = inflate_resolve_symbols_batch((const uint64_t *)(yp + o_segs), nsegs, sym, (const uint64_t *)(yp + o_sd),
                                               (const uint64_t *)(yp + o_se), (const BatchStream *)(yp + o_win), wins.size(), st))
        return rc;
    ZR_HIP(hipStreamSynchronize(st));
    return ZNG_ROCM_OK;
}

// ONE stream through the finder and the pass, as a table of one.  What a caller asks for:
struct LargeRequest {
    const uint8_t *d_src = nullptr;
    size_t         src_len = 0;
    const uint8_t *d_window = nullptr;
    uint32_t       window_len = 0;
    uint8_t       *d_dst = nullptr;
    size_t         dst_cap = 0;
    uint64_t       start_bit = 0;                         // the stream begins at this bit of d_src (blocks mode, pieces)
    bool           blocks = false;                        // blocks mode (the streaming hook), `sub`, `pp`: see pass_run
    bool           sub = false;
    PiecePass     *pp = nullptr;
};
// ... and what it gets.  The counts hold when inflate_large_try returns 1, or -5 (`produced` says how much room is needed);
// the counters and the block starts always (a pass that was not done has no parts).
struct LargeAnswer {
    uint64_t produced = 0;
    size_t   in_used = 0;
    uint64_t end_bit = 0;                                 // blocks mode: where the delivered blocks end ...
    bool     final = false;                               // ... and whether the BFINAL one is among them
    int      parts = 0, subparts = 0, substarts = 0;      // LargeCounters' first three, of this pass
    std::vector<std::pair<unsigned long long, uint64_t>> cands;      // an index is being built: Chain::cands, the pass's own positions
};
// Returns 1, or 0 = "irregular: use the sequential decoder", or a negative error (-5: dst_cap is too small).
static int inflate_large_try(Workspace *ws, const LargeRequest &q, LargeAnswer &a, hipStream_t st) {
    if (!large_length_ok(q.src_len)) return why("stream below 128 KiB (or 2 GiB and more)");
    std::vector<PassStream> ss(1);
    PassStream &s = ss[0];
    s.d_src = q.d_src;
    s.src_len = q.src_len;
    s.d_window = q.d_window;
    s.window_len = q.window_len;
    s.d_dst = q.d_dst;
    s.dst_cap = q.dst_cap;
    s.start_bit = q.start_bit;
    s.scan_lo = q.pp ? (size_t)q.pp->scan_lo : 0;         // (pieces: the finder scans the piece alone)
    s.key0 = q.pp ? q.pp->key0 : 0ull;
    // ---- candidates: the finder over a table of this one stream ---------------------------------------------------------
    std::vector<std::vector<unsigned long long>> good(1);
    FindOne one;
    if (int rc = find_starts(ws, ss, good, {0}, q.sub, st, &one)) return rc;
    if (one.no_room) return one.no_room;                  // (no scratch is this call's error, not a reason for the slow path)
    if (s.left) return 0;                                 // (far more candidates than a deflate stream has)
    // (SUBBLOCK goes on without candidates: a stream of fixed-code blocks is cut inside them)
    if (one.n_f1 == 0 && !q.sub) return why("no candidate block starts, or far more than a deflate stream has");
    // ---- the pass over this one stream ------------------------------------------------------------------------------
    thin_starts(good[0], q.start_bit, q.src_len, s.starts, s.heavy);
    s.chain.record = t_index_sink != nullptr;
    size_t taken = 0;
    int launches = 0;
    const int rc = pass_run(ws, ss, q.sub, q.blocks, q.pp, st, &taken, &launches);
    a.cands.swap(s.chain.cands);
    a.substarts = (int)s.substarts;
#ifdef ZR_INFLATE_STATS
    if (s.res) {
        g_dbg_starts = s.starts;
        g_dbg_res.assign(s.res, s.res + 8 * s.starts.size());
    }
#endif
    if (rc) return rc;
    if (s.left) return 0;
    a.produced = s.chain.produced;
    a.in_used = (size_t)((s.chain.end_bit + 7) >> 3);
    a.end_bit = s.chain.end_bit;
    a.final = s.chain.final;
    // no block complete yet (pieces: no symbol): nothing was launched
    if ((q.blocks || (q.pp && q.pp->stopped)) && a.produced == 0) return 1;
    if (s.status == -5) {
        set_error("inflate output (%llu bytes) exceeds dst_cap", (unsigned long long)a.produced);
        return -5;
    }
    a.parts = (int)s.chain.copies.size();
    a.subparts = (int)s.chain.subparts;
    return 1;
}
// A one-pass entry point's call (the workspace's lock is held): the stream through inflate_large_try, the calling thread's
// part counters from its answer (`pieces` and `host_bytes` are a pieces call's, and stay), and the caller's out parameters
// as far as the return value says they hold.
static int one_pass(Workspace *ws, const LargeRequest &q, hipStream_t st, uint64_t *out_len, size_t *in_used,
                    uint64_t *end_bit = nullptr, int *final = nullptr) {
    LargeAnswer a;
    const int rc = inflate_large_try(ws, q, a, st);
    t_last.parts = a.parts;
    t_last.subparts = a.subparts;
    t_last.substarts = a.substarts;
    if (rc != 1 && rc != -5) return rc;
    if (out_len) *out_len = a.produced;
    if (in_used) *in_used = a.in_used;
    if (end_bit) *end_bit = a.end_bit;
    if (final) *final = a.final ? 1 : 0;
    return rc;
}

// A large stream that is in HOST memory (zng_rocm_inflate_raw*, and with them uncompress2 and the gzip / zlib one-shots):
// up over PCIe once and through the device path; 0 = not done here (the caller's sequential decoder takes it).
int inflate_large_from_host(const uint8_t *src, size_t src_len, const uint8_t *d_window, uint32_t window_len, uint8_t *d_dst,
                            size_t dst_cap, uint64_t *out_len, size_t *in_used, hipStream_t st) {
    Workspace *ws = workspace_for(st);
    if (!ws) return 0;
    std::lock_guard<std::mutex> use(ws->mu);
    uint8_t *d_src = nullptr;
    if (scratch_reserve(ws, kScrLargeSrc, src_len + 64, false, (void **)&d_src) != ZNG_ROCM_OK) return 0;
    if (hipMemcpyAsync(d_src, src, src_len, hipMemcpyHostToDevice, st) != hipSuccess) return 0;
    LargeRequest q;
    q.d_src = d_src;
    q.src_len = src_len;
    q.d_window = d_window;
    q.window_len = window_len;
    q.d_dst = d_dst;
    q.dst_cap = dst_cap;
    const int rc = one_pass(ws, q, st, out_len, in_used);
    return rc == 1 || rc == -5 ? rc : 0;
}

// The device path alone, for callers that have their own sequential decoder to fall back on (hook.hip; inflate_large_call):
// 1 = done, 0 = irregular (nothing usable was written), -5 with *out_len set = dst_cap too small, other negatives = errors.
// Blocks mode (the streaming hook): d_src holds the stream from the byte that contains bit `start_bit` (0..7) on; 1 = *out_len
// bytes of complete blocks at d_dst, *end_bit = where they end, *final = the BFINAL block is among them; 0 = irregular (the
// caller's host decoder in blocks mode takes the call); -5 with *out_len = dst_cap too small.
static int device_only(const LargeRequest &q, hipStream_t st, uint64_t *out_len, size_t *in_used, uint64_t *end_bit = nullptr,
                       int *final = nullptr) {
    inflate_large_forget_parts();
    Workspace *ws = workspace_for(st);                   // scratch is keyed by the caller's HIP stream (context.h)
    if (!ws) return ZNG_ROCM_ENOMEM;
    std::lock_guard<std::mutex> use(ws->mu);
    return one_pass(ws, q, st, out_len, in_used, end_bit, final);
}
int inflate_large_device_only(const uint8_t *d_src, size_t src_len, const uint8_t *d_window, uint32_t window_len, uint8_t *d_dst,
                              size_t dst_cap, uint64_t *out_len, size_t *in_used, hipStream_t st) {
    LargeRequest q;
    q.d_src = d_src;
    q.src_len = src_len;
    q.d_window = d_window;
    q.window_len = window_len;
    q.d_dst = d_dst;
    q.dst_cap = dst_cap;
    return device_only(q, st, out_len, in_used);
}
int inflate_large_blocks_device_only(const uint8_t *d_src, size_t src_len, unsigned start_bit, const uint8_t *d_window,
                                     uint32_t window_len, uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, uint64_t *end_bit,
                                     int *final, hipStream_t st) {
    LargeRequest q;
    q.d_src = d_src;
    q.src_len = src_len;
    q.d_window = d_window;
    q.window_len = window_len;
    q.d_dst = d_dst;
    q.dst_cap = dst_cap;
    q.start_bit = start_bit & 7u;
    q.blocks = true;
    return device_only(q, st, out_len, nullptr, end_bit, final);
}

}  // namespace zr

using namespace zr;

extern "C" {

int zng_rocm_inflate_large_last_parts(void) { return t_last.parts; }
int zng_rocm_inflate_large_last_subparts(void) { return t_last.subparts; }
int zng_rocm_inflate_large_last_substarts(void) { return t_last.substarts; }
int zng_rocm_inflate_large_last_pieces(void) { return t_last.pieces; }
uint64_t zng_rocm_inflate_large_last_host_bytes(void) { return t_last.host_bytes; }
#ifdef ZR_INFLATE_STATS
unsigned zng_rocm_debug_large_parts(unsigned long long *starts, uint32_t *res8, unsigned cap) {
    const unsigned n = (unsigned)std::min<size_t>(cap, g_dbg_starts.size());
    for (unsigned i = 0; i < n; ++i) {
        starts[i] = g_dbg_starts[i];
        for (int k = 0; k < 8; ++k) res8[8 * i + k] = g_dbg_res[8 * (size_t)i + k];
    }
    return (unsigned)g_dbg_starts.size();
}
#endif

}  // extern "C"

// a host copy of [d_src, d_src + len), complete when this returns (never empty: the decoders want a pointer)
static int host_copy(std::vector<uint8_t> &host, const uint8_t *d_src, size_t len, hipStream_t st) {
    host.resize(len ? len : 1);
    if (!len) return ZNG_ROCM_OK;
    ZR_HIP(hipMemcpyAsync(host.data(), d_src, len, hipMemcpyDeviceToHost, st));
    ZR_HIP(hipStreamSynchronize(st));
    return ZNG_ROCM_OK;
}

// zng_rocm_inflate_large_dev, and zng_rocm_inflate_large_ex_dev with `sub` = ZNG_ROCM_INFLATE_SUBBLOCK
static int inflate_large_call(const uint8_t *d_src, size_t src_len, const uint8_t *d_window, uint32_t window_len,
                              uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, size_t *in_used, void *stream, bool sub) {
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    if ((!d_src && src_len) || window_len > 32768u || (window_len && !d_window)) return ZNG_ROCM_EINVAL;
    DeviceGuard dev;
    hipStream_t st = (hipStream_t)stream;
    LargeRequest q;
    q.d_src = d_src;
    q.src_len = src_len;
    q.d_window = d_window;
    q.window_len = window_len;
    q.d_dst = d_dst;
    q.dst_cap = dst_cap;
    q.sub = sub;
    if (int rc = device_only(q, st, out_len, in_used)) return rc;
    // irregular: the sequential decoder on a host copy of the stream says exactly what the reference would
    std::vector<uint8_t> host;
    if (int rc = host_copy(host, d_src, src_len, st)) return rc;
    return inflate_raw_window_sequential(host.data(), src_len, d_window, window_len, d_dst, dst_cap, out_len, in_used, st);
}

// ---- pieces: zng_rocm_inflate_large_pieces_dev --------------------------------------------------------------------------
// The stream is decoded in passes over pieces of at most `piece_bytes` compressed bytes.  A pass that does not reach the
// stream's end takes the piece's end as the end of the input: the chain stops at the first part that ran out of it, the
// parts in front are delivered, and the next piece begins exactly at that part's start (a start the part in front landed
// on), with its key and the BFINAL the chain carried to it.  Each pass gets the 32 KiB in front of its output as history.
// A piece the device cannot do (no start behind its own is landed on, a data error on the chain, a truncated end) goes to
// the sequential decoder from the last block start delivered: complete blocks first, and the loop goes on behind them; a
// data error or the end of the input there is decoded once more in the stream form, whose status, message and counts
// are then the reference's.
// The loop's rules -- the state it carries, where a piece and its pass's buffer begin and end, how positions are re-based,
// which bytes are the history, what the sequential decoder is given -- are inflate_large_plan.h's (PiecesState); here are the
// splice, the pass, the host decoder and the uploads.  `c` counts the call (substarts: a pass repeated with half the piece
// does not count, every other pass does).  kPieceMin / kPieceDefault / kPieceMax: inflate_large_limits.h
static int inflate_pieces_call(const uint8_t *d_src, size_t src_len, const uint8_t *d_window, uint32_t window_len,
                               uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, size_t *in_used, size_t piece_bytes, bool sub,
                               hipStream_t st, LargeCounters &c) {
    Workspace *ws = workspace_for(st);                   // scratch is keyed by the caller's HIP stream (context.h)
    if (!ws) return ZNG_ROCM_ENOMEM;
    std::unique_lock<std::mutex> use(ws->mu);            // (let go while the sequential decoder works on the host)
    uint8_t *d_hist = nullptr;
    if (int rc = scratch_reserve(ws, kScrLargeHist, 32768 + 64, false, (void **)&d_hist)) return rc;
    // the history H (piece_history) as a pointer: where it lies, or spliced into d_hist (under the lock)
    auto history = [&](const PieceHistory &H, const uint8_t **h) -> int {
        *h = H.where == PieceHistory::kInDst ? d_dst + H.dst_off : d_window;
        if (H.where != PieceHistory::kSpliced) return ZNG_ROCM_OK;
        if (int rc = scratch_reserve(ws, kScrLargeHist, 32768 + 64, false, (void **)&d_hist)) return rc;
        ZR_HIP(hipMemcpyAsync(d_hist, d_window + H.window_off, H.from_window, hipMemcpyDeviceToDevice, st));
        ZR_HIP(hipMemcpyAsync(d_hist + H.from_window, d_dst, H.from_dst, hipMemcpyDeviceToDevice, st));
        *h = d_hist;
        return ZNG_ROCM_OK;
    };
    // the tail behind the sequential decoder, in either form: the tokens' bytes go behind the anchor (`aout`) with the history H
    // in front of them, *total = the output up to their end; -5 when that does not fit.  The tokens are freed.
    auto deliver = [&](zng_rocm_inflate_tokens *tk, uint64_t aout, const PieceHistory &H, uint64_t *total) -> int {
        *total = aout + tk->out_len;
        const uint8_t *h = nullptr;
        int rc = -5;
        if (*total > dst_cap) set_error("inflate output (%llu bytes) exceeds dst_cap", (unsigned long long)*total);
        else if ((rc = history(H, &h)) == ZNG_ROCM_OK) rc = inflate_tokens_to_device(tk, h, H.len, d_dst + aout, st);
        zng_rocm_inflate_tokens_free(tk);
        return rc;
    };
    PiecesState s = pieces_begin(piece_bytes);
    for (;;) {
        NextPiece np = piece_next(s, src_len, piece_bytes);
        if (np.any) {
            const PieceHistory H = piece_history(s.produced, window_len);
            LargeRequest q;
            q.d_src = d_src + np.base;
            q.src_len = (size_t)np.len();
            if (int rc = history(H, &q.d_window)) return rc;
            q.window_len = H.len;
            q.d_dst = d_dst + s.produced;
            q.dst_cap = dst_cap > s.produced ? dst_cap - s.produced : 0;
            q.start_bit = np.start_bit;
            q.sub = sub;
            q.pp = &np.pp;
            LargeAnswer a;
            const int rc = inflate_large_try(ws, q, a, st);
            if (rc == 0 && np.pp.halve && piece_halve(s)) continue;       // over a scratch cap: the same start with half the piece
            c.substarts += a.substarts;
            if (rc == 1) {
                ++c.pieces;
                c.parts += a.parts;
                c.subparts += a.subparts;
                if (t_index_sink) piece_cands(a.cands, np, s, t_index_sink->cands);
                const PieceStep step = piece_after_pass(s, np, a.produced, a.in_used, piece_bytes);
                if (step.done) {                          // the stream ended in this piece
                    *out_len = s.produced;
                    *in_used = (size_t)step.in_used;
                    return 1;
                }
                if (step.anchored && t_index_sink) t_index_sink->cands.emplace_back(s.abit, s.aout);
                continue;
            }
            if (rc == -5) {                               // the piece's output does not fit behind what is there
                *out_len = s.produced + a.produced;
                *in_used = (size_t)np.stream_byte(a.in_used);
                set_error("inflate output (%llu bytes) exceeds dst_cap", (unsigned long long)*out_len);
                return -5;
            }
            if (rc < 0) return rc;
        }
        // the sequential decoder from the anchor, with the history in front of it (seq_input: how much input, and when more).
        // The workspace is not used while it decodes: the lock is let go, and taken again to splice the history (d_hist) and
        // upload what was decoded.
        SeqInput in = seq_input(s);
        const PieceHistory H = piece_history(s.aout, window_len);
        use.unlock();
        std::vector<uint8_t> host;
        uint64_t len = 0, eb = in.sb;
        zng_rocm_inflate_tokens tk;
        int status = 0;
        for (;;) {
            len = in.len(src_len);
            if (int rc = host_copy(host, d_src + in.a0, (size_t)len, st)) return rc;
            status = zng_rocm_inflate_tokens_decode_blocks(host.data(), (size_t)len, in.sb, H.len, &tk, &eb);
            if (!seq_wants_more(in, src_len, status, eb)) break;
            zng_rocm_inflate_tokens_free(&tk);
        }
        // a data error, or the end of the input inside a block: the stream form from the same bit (still without the lock)
        const bool stream_form = seq_stream_form(status, eb, in.sb);
        if (stream_form) {
            zng_rocm_inflate_tokens_free(&tk);
            status = zr_inflate_decode_from(host.data(), (size_t)len, in.sb, H.len, &tk);
        }
        use.lock();
        // (sb <= 7 < 8 * len unless len = 0 and sb = 0: the decoder's ZNG_ROCM_EINVAL, which has the value of Z_DATA_ERROR,
        // cannot come back)
        if (status == -4) {
            zng_rocm_inflate_tokens_free(&tk);
            return ZNG_ROCM_ENOMEM;
        }
        const size_t tk_used = tk.in_used;
        if (stream_form && status < 0) set_error("%s", tk.msg);       // (a -5 below replaces it)
        uint64_t total = 0;
        const int rc = deliver(&tk, s.aout, H, &total);
        if (stream_form) {                               // its status, message and counts are the one-shot's
            c.host_bytes += tk_used;
            *out_len = total;
            *in_used = (size_t)in.stream_byte(tk_used);
            return rc != ZNG_ROCM_OK ? rc : status;
        }
        // complete blocks: delivered, and the device goes on behind them
        c.host_bytes += seq_blocks_bytes(eb);
        if (total > dst_cap) {                           // (deliver's -5)
            *out_len = total;
            *in_used = (size_t)in.stream_byte(seq_blocks_bytes(eb));
        }
        if (rc != ZNG_ROCM_OK) return rc;
        if (status == 1) {
            *out_len = total;
            *in_used = (size_t)in.stream_byte(tk_used);
            return 1;
        }
        piece_after_blocks(s, in, eb, total, piece_bytes);
        if (t_index_sink) t_index_sink->cands.emplace_back(s.abit, s.aout);
    }
}

extern "C" {

int zng_rocm_inflate_large_pieces_dev(const uint8_t *d_src, size_t src_len, const uint8_t *d_window, uint32_t window_len,
                                      uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, size_t *in_used, size_t piece_bytes,
                                      uint32_t flags, void *stream) {
    t_last = LargeCounters{};
    if (out_len) *out_len = 0;
    if (in_used) *in_used = 0;
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    if (flags & ~ZNG_ROCM_INFLATE_SUBBLOCK) {
        set_error("zng_rocm_inflate_large_pieces_dev: unknown flag bits 0x%x", flags & ~ZNG_ROCM_INFLATE_SUBBLOCK);
        return ZNG_ROCM_EINVAL;
    }
    if (piece_bytes && (piece_bytes < kPieceMin || piece_bytes > kPieceMax)) {
        set_error("zng_rocm_inflate_large_pieces_dev: piece_bytes %zu outside %zu .. %zu", piece_bytes, kPieceMin, kPieceMax);
        return ZNG_ROCM_EINVAL;
    }
    if ((!d_src && src_len) || window_len > 32768u || (window_len && !d_window) || !out_len || !in_used) return ZNG_ROCM_EINVAL;
    DeviceGuard dev;
    LargeCounters c;
    const int rc = inflate_pieces_call(d_src, src_len, d_window, window_len, d_dst, dst_cap, out_len, in_used,
                                       piece_bytes ? piece_bytes : kPieceDefault, flags != 0, (hipStream_t)stream, c);
    t_last = c;
    return rc;
}

int zng_rocm_inflate_large_dev(const uint8_t *d_src, size_t src_len, const uint8_t *d_window, uint32_t window_len,
                               uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, size_t *in_used, void *stream) {
    return inflate_large_call(d_src, src_len, d_window, window_len, d_dst, dst_cap, out_len, in_used, stream, false);
}

int zng_rocm_inflate_large_ex_dev(const uint8_t *d_src, size_t src_len, const uint8_t *d_window, uint32_t window_len,
                                  uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, size_t *in_used, uint32_t flags, void *stream) {
    if (flags & ~ZNG_ROCM_INFLATE_SUBBLOCK) {
        if (out_len) *out_len = 0;
        if (in_used) *in_used = 0;
        set_error("zng_rocm_inflate_large_ex_dev: unknown flag bits 0x%x", flags & ~ZNG_ROCM_INFLATE_SUBBLOCK);
        return ZNG_ROCM_EINVAL;
    }
    return inflate_large_call(d_src, src_len, d_window, window_len, d_dst, dst_cap, out_len, in_used, stream, flags != 0);
}

}  // extern "C"

// ---- many large streams: zng_rocm_inflate_large_streams_dev ---------------------------------------------------------------
// A ROUND of streams at once: ONE finder pass over a table of (stream, range) items whose survivors carry their stream,
// then ONE pass (pass_run: stream mode; no pieces, no blocks) over the parts of all the round's streams.  So the long parts
// of one stream run under the short parts of the others, and the host round trips between the kernels are paid per round.
// A stream the device path cannot do leaves the round and is decoded as zng_rocm_inflate_large_ex_dev does it (a host
// copy, the sequential decoder) behind the round's device work; the others do not notice.
// kRoundMin / kRoundEnd / kRoundDefault: inflate_large_limits.h
static thread_local int t_batch_rounds = 0;
static thread_local int t_batch_part_launches = 0;

namespace zr {
// framing_large.hip answers a wrapped member whose header it refuses without reaching the calls above: the calling
// thread's last_* counters then say that nothing ran
void inflate_large_reset_counters() {
    t_last = LargeCounters{};
    t_batch_rounds = t_batch_part_launches = 0;
}
}  // namespace zr

// One round: the jobs idx[0 .. *taken) (all of idx unless their parts together pass one launch's) through the finder and
// the pass.  Jobs done on the device have their output fields set; the others are appended to `host` (the caller
// decodes them sequentially, as zng_rocm_inflate_large_ex_dev does it, behind the round's device work).
// `counting`: pass_run's counting mode -- d_dst / dst_cap are not looked at, and `host` are the jobs to be sized whole.
static int round_run(Workspace *ws, zng_rocm_inflate_large_job *jobs, const std::vector<size_t> &idx, bool sub, hipStream_t st,
                     std::vector<size_t> &host, size_t *taken, bool counting = false) {
    std::vector<PassStream> ss(idx.size());
    std::vector<std::vector<unsigned long long>> good(idx.size());
    std::vector<size_t> scan;
    for (size_t k = 0; k < idx.size(); ++k) {
        const zng_rocm_inflate_large_job &J = jobs[idx[k]];
        PassStream &s = ss[k];
        s.d_src = J.d_src;
        s.src_len = J.src_len;
        s.d_window = J.d_window;
        s.window_len = J.window_len;
        s.d_dst = J.d_dst;
        s.dst_cap = J.dst_cap;
        s.job = (long)idx[k];
        if (large_length_ok(J.src_len)) scan.push_back(k);
        else if (!counting) s.left = true;                // (the counting mode takes it as one part: pass_run)
    }
    // ---- candidates: the byte patterns for every stream; F1 + F2 for those they do not cut ---------------------------
    if (int rc = find_starts(ws, ss, good, scan, sub, st)) return rc;
    for (size_t k : scan) {
        PassStream &s = ss[k];
        if (s.left) continue;
        if (good[k].size() > s.src_len / 512 + 4096) leave(s, "far more valid block headers than a deflate stream has");
        else thin_starts(good[k], 0, s.src_len, s.starts, s.heavy);
    }
    int launches = 0;
    const int rc = pass_run(ws, ss, sub, false, nullptr, st, taken, &launches, counting);
    t_batch_part_launches += launches;
    if (rc) return rc;
    for (size_t k = 0; k < *taken; ++k) {
        const PassStream &s = ss[k];
        zng_rocm_inflate_large_job &J = jobs[idx[k]];
        if (s.left) {
            host.push_back(idx[k]);
            continue;
        }
        J.status = s.status;
        J.out_len = s.chain.produced;
        J.in_used = (size_t)((s.chain.end_bit + 7) >> 3);
        J.msg = nullptr;
        J.parts = (uint32_t)(counting ? s.counted_parts : s.chain.copies.size());
        J.subparts = (uint32_t)s.chain.subparts;
    }
    return ZNG_ROCM_OK;
}

// a job that no device path answered: the status and counts given, no parts
static void job_answer(zng_rocm_inflate_large_job &j, int status, uint64_t n, size_t used, const char *msg) {
    j.status = status;
    j.out_len = n;
    j.in_used = used;
    j.msg = msg;
    j.parts = j.subparts = 0;
}

// The jobs `list` sized WHOLE, one wavefront each (inflate_size_stream_kernel), in one launch: every stream the counting chain
// cannot do.  The row is zng_rocm_inflate_sizes_dev's with a 64-bit count -- the decoder's verdict, message and consumed
// bytes -- so nothing of the stream comes to the host.
static int size_whole_streams(Workspace *ws, zng_rocm_inflate_large_job *jobs, const std::vector<size_t> &list, hipStream_t st) {
    const size_t n = list.size();
    if (!n) return ZNG_ROCM_OK;
    const PartTables T = part_tables(n, false, false, 0);                        // jobs | (starts: unused) | 8 result words
    uint8_t *sp = nullptr, *hq = nullptr;
    if (int rc = scratch_reserve(ws, kScrLargeParts, T.device_bytes, false, (void **)&sp)) return rc;
    if (int rc = scratch_reserve(ws, kScrLargePartsHost, T.mirror_bytes, true, (void **)&hq)) return rc;
    InflateJobDev *pj = (InflateJobDev *)(hq + T.jobs);
    const uint32_t *res = (const uint32_t *)(hq + T.res);
    for (size_t k = 0; k < n; ++k) {
        const zng_rocm_inflate_large_job &j = jobs[list[k]];
        pj[k] = InflateJobDev{j.d_src, nullptr, j.src_len, 0, j.window_len, 0u};
    }
    ZR_HIP(hipMemcpyAsync(sp + T.jobs, pj, n * sizeof(InflateJobDev), hipMemcpyHostToDevice, st));
    if (int rc = launch_inflate_size_streams_device((const InflateJobDev *)(sp + T.jobs), n, (uint32_t *)(sp + T.res), st)) return rc;
    ZR_HIP(hipMemcpyAsync(hq + T.res, sp + T.res, n * 32, hipMemcpyDeviceToHost, st));
    ZR_HIP(hipStreamSynchronize(st));
    for (size_t k = 0; k < n; ++k) {
        const LsRow r = ls_stream_row(res + 8 * k);
        const int status = (int)(int32_t)r.status;
        job_answer(jobs[list[k]], status, r.out_len, r.used, status == -3 && r.msg != kMsgNone ? zng_rocm_inflate_message(r.msg) : nullptr);
    }
    return ZNG_ROCM_OK;
}

// The rounds of zng_rocm_inflate_large_streams_dev, and (`counting`) of the sizing calls: the arguments have been checked.
static int rounds_run(zng_rocm_inflate_large_job *jobs, size_t njobs, size_t round_bytes, bool sub, bool counting, hipStream_t st) {
    if (!round_bytes) round_bytes = kRoundDefault;
    DeviceGuard dev;
    Workspace *ws = workspace_for(st);                   // scratch is keyed by the caller's HIP stream (context.h)
    if (!ws) return ZNG_ROCM_ENOMEM;
    int first_err = ZNG_ROCM_OK;
    size_t next = 0;
    while (next < njobs) {
        // a round: jobs in order until their compressed bytes would pass round_bytes (a larger job is a round of its own)
        std::vector<size_t> idx;
        size_t bytes = 0;
        for (size_t i = next; i < njobs; ++i) {
            if (!idx.empty() && bytes + jobs[i].src_len > round_bytes) break;
            idx.push_back(i);
            bytes += jobs[i].src_len;
        }
        std::vector<size_t> host;
        size_t taken = idx.size();
        int rc;
        {
            std::lock_guard<std::mutex> use(ws->mu);
            rc = round_run(ws, jobs, idx, sub, st, host, &taken, counting);
            // the jobs that left a counting round: sized whole on the device, behind the round's parts
            if (rc == ZNG_ROCM_OK && counting) rc = size_whole_streams(ws, jobs, host, st);
        }
        ++t_batch_rounds;
        if (rc != ZNG_ROCM_OK) {                         // a device error: the round's jobs have it, and the call ends
            for (size_t i = idx[0]; i < njobs; ++i) job_answer(jobs[i], rc, 0, 0, nullptr);
            return rc;
        }
        // the jobs that left the round: the sequential decoder on a host copy, exactly as zng_rocm_inflate_large_ex_dev
        if (counting) host.clear();                      // (sized above)
        for (size_t i : host) {
            zng_rocm_inflate_large_job &j = jobs[i];
            std::vector<uint8_t> copy;
            int s = host_copy(copy, j.d_src, j.src_len, st);
            if (s != ZNG_ROCM_OK) set_error("zng_rocm_inflate_large_streams_dev: copying job %zu to the host failed", i);
            uint64_t n = 0;
            size_t used = 0;
            const char *msg = nullptr;
            if (s == ZNG_ROCM_OK)
                s = inflate_raw_window_sequential_msg(copy.data(), j.src_len, j.d_window, j.window_len, j.d_dst, j.dst_cap, &n, &used,
                                                      &msg, st);
            job_answer(j, s, n, used, s == -3 ? msg : nullptr);
            if ((s == ZNG_ROCM_EHIP || s == ZNG_ROCM_ENOMEM) && first_err == ZNG_ROCM_OK) first_err = s;
        }
        next = idx[0] + taken;
    }
    return first_err;
}

namespace zr {
// zng_rocm_uncompress_large_size_dev / _sizes_dev (framing_large.hip) on raw payloads whose arguments have been checked:
// per job status / out_len / in_used / msg / parts as the decode batch sets them, d_dst / dst_cap not looked at.  `single`:
// the one-stream call, whose parts zng_rocm_inflate_large_last_parts() reports.
int inflate_large_sizes_raw(zng_rocm_inflate_large_job *jobs, size_t njobs, size_t round_bytes, bool single, hipStream_t st) {
    inflate_large_reset_counters();
    const int rc = rounds_run(jobs, njobs, round_bytes, false, true, st);
    if (single && njobs == 1 && jobs[0].status == 1) t_last.parts = (int)jobs[0].parts;
    return rc;
}
}  // namespace zr

extern "C" {

int zng_rocm_inflate_large_last_rounds(void) { return t_batch_rounds; }
int zng_rocm_inflate_large_last_part_launches(void) { return t_batch_part_launches; }

int zng_rocm_inflate_large_streams_dev(zng_rocm_inflate_large_job *jobs, size_t njobs, size_t round_bytes, uint32_t flags,
                                       void *stream) {
    t_batch_rounds = 0;
    t_batch_part_launches = 0;
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    if (flags & ~ZNG_ROCM_INFLATE_SUBBLOCK) {
        set_error("zng_rocm_inflate_large_streams_dev: unknown flag bits 0x%x", flags & ~ZNG_ROCM_INFLATE_SUBBLOCK);
        return ZNG_ROCM_EINVAL;
    }
    if (round_bytes && (round_bytes < kRoundMin || round_bytes >= kRoundEnd)) {
        set_error("zng_rocm_inflate_large_streams_dev: round_bytes %zu outside %zu .. 2 GiB", round_bytes, kRoundMin);
        return ZNG_ROCM_EINVAL;
    }
    if (njobs && !jobs) return ZNG_ROCM_EINVAL;
    for (size_t i = 0; i < njobs; ++i) {
        const zng_rocm_inflate_large_job &j = jobs[i];
        if ((!j.d_src && j.src_len) || j.window_len > 32768u || (j.window_len && !j.d_window) || (!j.d_dst && j.dst_cap)) {
            set_error("zng_rocm_inflate_large_streams_dev: job %zu: a null buffer with a length, or window_len above 32768", i);
            return ZNG_ROCM_EINVAL;
        }
    }
    if (!njobs) return ZNG_ROCM_OK;
    return rounds_run(jobs, njobs, round_bytes, flags != 0, false, (hipStream_t)stream);
}

}  // extern "C"
