// inflate_tables.h -- what the device inflaters share in front of their symbol loops (inflate_dev.hip's stream, part and sync
// kernels, inflate_sizes.hip's sizing kernel): the 16-bit table entry and its marks, the LDS layouts of a wave's tables, the
// base values and extra bits of the length and distance symbols, the wide distance and literal/length entries, and the
// wavefront's canonical-code builder with the lookup of a code longer than the root.  Device code; include it inside a HIP
// translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "deflate_dev.h"
#include "inflate_dev_types.h"

// (a diagnostic build of inflate_dev.hip checks every index: it defines ZR_IDX before this header)
#ifndef ZR_IDX
#define ZR_IDX(i, n) (i)
#endif

namespace zr {

// Table entry, 16 bits: code length in bits 0-3, SYMBOL in bits 4-15 (literal/length 0..287, distance 0..31, code-length
// symbol 0..18).  Base values and extra-bit counts are arithmetic in the symbol (length_of / distance_of), so nothing
// wider is needed: the three tables of a stream take 3.3 KiB of LDS, and LDS per wave is what bounds how many streams
// a CU decodes at once.  kLongMark: the code is longer than the table's root; kBadMark: no code has this prefix.
constexpr uint32_t kLongMark = (0xfffu << 4), kBadMark = (0xffeu << 4) | 1u;
__device__ __forceinline__ uint32_t make_entry(uint32_t nbits, uint32_t sym) { return nbits | (sym << 4); }

constexpr int kLitRootStream = 10, kLitRootPart = 10, kClRoot = 7;   // (a 9-bit literal root in part mode -- a 13th wave per CU -- was slower: 6.1 -> 6.8 ms, too many codes take the long path)
// root bits of the distance table: 9 for whole streams (16 per CU fit either way), 8 in part mode, where the 1 KiB it saves
// is the twelfth wave of a CU (part kernel 6.6 -> 6.1 ms; whole streams lose 2.5 % with 8: more codes take the long path)
constexpr int kDistRootStream = 9, kDistRootPart = 8;
// order in which the code-length code's lengths are sent (RFC 1951 3.2.7; inflate.c:832-833 holds the same permutation)
__device__ const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
constexpr int kCodeLit = 0, kCodeDist = 1, kCodeCl = 2;

// Whole streams, and the parts of a call with few of them: every table has its own place (9.9 KiB with a ring of bytes,
// exactly 16 streams per CU; 12.9 KiB with a ring of 16-bit symbols, 12 parts per CU).
template <int RING, typename T, int DR, int LR>
struct InflateLdsStream {
    uint16_t lit[1 << LR];
    uint32_t dist[1 << DR];             // wide entries: code length | extra bits << 4 | base distance << 8 (wide_distance)
    uint16_t cl_[1 << kClRoot];
    uint32_t cnt_[3][16], first_[3][16], offs_[3][16], run[16];
    uint16_t sorted_lit[288], sorted_dist[32], sorted_cl_[32];
    uint8_t  lens[320 + 8];
    uint8_t  cl_lens_[24];
    T        ring[RING] __attribute__((aligned(16)));
    __device__ __forceinline__ uint32_t *cnt(int which) { return cnt_[which]; }
    __device__ __forceinline__ uint32_t *first(int which) { return first_[which]; }
    __device__ __forceinline__ uint32_t *offs(int which) { return offs_[which]; }
    __device__ __forceinline__ uint16_t *cl() { return cl_; }
    __device__ __forceinline__ uint16_t *sorted_cl() { return sorted_cl_; }
    __device__ __forceinline__ uint8_t *cl_lens() { return cl_lens_; }
};
// The packed layout: LDS is what limits how many wavefronts decode at once.
// The code-length code -- root table, sorted symbols, counts, the 19 lengths -- only lives while a dynamic header is read,
// and the distance table is only built when that is over: one place for both; the builder's first-code and offset words
// are 16 bits.  LIT: the literal/length table's element, the builder's 16-bit entry or a wide one (wide_literal: the
// builder's entries then lie in the first half).
template <typename LIT, int DR, int LR>
struct InflateLdsPacked {
    LIT lit[1 << LR];
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
// Parts, when there are many (16-bit symbols: the ring alone is 8 KiB): the packed tables and the ring.  12.2 KiB: a 13th
// part per CU (part kernel of the cfg3 stream 6.0 -> 5.25 ms).  (The same layout for whole streams cost their kernel 5 %
// -- 42.1 -> 39.8 GB/s on the level-1 class's streams, with the LDS size padded back to what it was -- so they keep theirs.)
template <int RING, typename T, int DR, int LR>
struct InflateLdsPart : InflateLdsPacked<uint16_t, DR, LR> {
    T        ring[RING] __attribute__((aligned(16)));
};
// The sizing pass (inflate_sizes.hip): the packed tables with wide literal/length entries and no ring, 7.2 KiB against the
// stream decoder's 9.9 KiB.
template <int DR, int LR>
using SizesLds = InflateLdsPacked<uint32_t, DR, LR>;
static_assert(sizeof(((InflateLdsPart<4096, uint16_t, 8, 10> *)nullptr)->h) <= sizeof(uint32_t) << 8, "the header's tables must fit the distance table's place");
static_assert(sizeof(((SizesLds<kDistRootStream, kLitRootStream> *)nullptr)->h) <= sizeof(uint32_t) << kDistRootStream,
              "the header's tables must fit the distance table's place");

// base values / extra bits of the length and distance symbols (RFC 1951 3.2.5; inftrees.c:38-49 hold the same numbers)
__device__ __forceinline__ void length_of(uint32_t k, uint32_t *base, uint32_t *extra) {     // k = symbol - 257, 0..28
    if (k < 8) { *base = 3 + k; *extra = 0; }
    else if (k == 28) { *base = 258; *extra = 0; }
    else { const uint32_t e = (k - 4) >> 2; *extra = e; *base = 3 + ((4 + (k & 3)) << e); }
}
__device__ __forceinline__ void distance_of(uint32_t k, uint32_t *base, uint32_t *extra) {   // k = symbol, 0..29
    if (k < 4) { *base = 1 + k; *extra = 0; }
    else { const uint32_t e = (k - 2) >> 1; *extra = e; *base = 1 + ((2 + (k & 1)) << e); }
}

__device__ __forceinline__ void wave_sync() {            // LDS written by some lanes is read by others of the same wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
typedef uint32_t u32x4_v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the distance table's decode-loop form: base and extra-bit count ride in the entry (the loop is scalar-issue bound and
// the arithmetic of distance_of is 11 scalar instructions per match; 1 KiB more LDS per stream)
// kBadWide | n: an invalid code of n bits -- symbols 30, 31, or the unused entry of an incomplete set (1 bit).  The length
// matters at the end of a truncated stream: the reference reports an invalid code only when all of its bits are input
// (inflate.c's NEEDBITS / PULLBYTE loops ask for more first), and bits behind the input read as zeros here.
constexpr uint32_t kLongWide = 0xfffffff0u, kBadWide = 0xffffffe0u;
__device__ __forceinline__ uint32_t wide_distance(uint32_t e) {           // e: a 16-bit entry
    if (e == kLongMark) return kLongWide;
    const uint32_t sym = e >> 4;
    if (sym > 29u) return kBadWide | (e & 15u);                               // 30, 31 (inftrees.c:48-49), no code
    uint32_t b = 0, x = 0;
    distance_of(sym, &b, &x);
    return (e & 15u) | (x << 4) | (b << 8);
}

// the 16-bit distance entries the builder left in the first half of L.dist -> wide entries, through registers
template <int DR, typename LDS>
__device__ __forceinline__ void widen_distances(LDS &L, int lane) {
    uint32_t w[(1 << DR) / 64];
#pragma unroll
    for (int j = 0; j < (1 << DR) / 64; ++j) w[j] = wide_distance(reinterpret_cast<const uint16_t *>(L.dist)[lane + 64 * j]);
    wave_sync();
#pragma unroll
    for (int j = 0; j < (1 << DR) / 64; ++j) L.dist[lane + 64 * j] = w[j];
    wave_sync();
}

// The literal/length table's loop form in the sizing pass.  It never needs a literal's VALUE, so a literal's entry is its code
// length alone (1 .. 15: "entry < 16" is the literal test and the entry is the shift), and a length symbol's entry carries its
// base length and extra-bit count, as wide_distance's entries do: no arithmetic on the symbol in the loop.
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

// Canonical code from `n` code lengths (inftrees.c:32-297 re-thought for a wavefront): per-length counts, the
// over-subscribed / incomplete checks of inftrees.c:104-137, symbols sorted by (length, symbol), and the root-bit
// primary table, one entry per lane per pass, each found by the canonical comparison "code - first[L] < count[L]".
// Codes longer than the root get a kLong entry; the decode loop resolves those with the same comparison (they are the
// rare symbols by construction).  Returns 0, or 1 for an invalid set.
template <typename LDS>
__device__ __forceinline__ int build_code(LDS &L, int which, const uint8_t *lens, int n, int root, uint16_t *table,
                          uint16_t *sorted, int lane) {
    auto *cnt = L.cnt(which);
    auto *first = L.first(which);
    auto *offs = L.offs(which);
    if (lane < 16) cnt[lane] = 0;
    wave_sync();
    for (int s = lane; s < n; s += 64) atomicAdd(&cnt[ZR_IDX(lens[s], 16)], 1u);
    wave_sync();
    const uint32_t mine = lane < 16 ? cnt[lane] : 0u;
    int left = 1, max = 0;
    uint32_t code = 0, off = 0;
    bool over = false;
    for (int len = 1; len <= 15; ++len) {
        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)mine, len);
        left = (left << 1) - (int)c;
        if (left < 0) over = true;
        if (lane == 0) {
            first[len] = (std::remove_reference_t<decltype(first[0])>)code;      // (< 2^len for every set that is not rejected)
            offs[len] = (std::remove_reference_t<decltype(offs[0])>)off;
            L.run[len] = (std::remove_reference_t<decltype(L.run[0])>)off;
        }
        code = (code + c) << 1;
        off += c;
        if (c) max = len;
    }
    if (over) return 1;                                              // over-subscribed (inftrees.c:128-132)
    if (max == 0) {                                                  // no codes at all (inftrees.c:114-122): every entry invalid
        for (int e = lane; e < (1 << root); e += 64) table[e] = (uint16_t)(which == kCodeCl ? make_entry(1, 0) : kBadMark);
        if (lane == 0) cnt[0] = 0;
        wave_sync();
        return 0;
    }
    if (left > 0 && (which == kCodeCl || max != 1)) return 1;        // incomplete set (inftrees.c:133-134)
    wave_sync();
    // stable counting sort: rank of a symbol among the symbols of its length = lower lanes of the same ballot
    for (int base = 0; base < n; base += 64) {
        const int s = base + lane;
        const uint32_t l = s < n ? lens[s] : 0u;
        bool active = l != 0;
        unsigned long long m = __ballot(active);
        while (m) {
            const int f = __builtin_ctzll(m);
            const uint32_t lu = (uint32_t)__builtin_amdgcn_readlane((int)l, f);
            const bool hit = active && l == lu;
            const unsigned long long same = __ballot(hit);
            const uint32_t at = uni(L.run[ZR_IDX(lu, 16)]);
            if (hit) sorted[ZR_IDX(at + (uint32_t)__builtin_popcountll(same & ((1ull << lane) - 1ull)), which == kCodeLit ? 288 : 32)] = (uint16_t)s;
            if (lane == f) L.run[ZR_IDX(lu, 16)] = (std::remove_reference_t<decltype(L.run[0])>)(at + (uint32_t)__builtin_popcountll(same));
            active = active && !hit;
            m &= ~same;
            wave_sync();
        }
    }
    wave_sync();
    const int top = max < root ? max : root;
    for (int e = lane; e < (1 << root); e += 64) {
        const uint32_t rev = __builtin_bitreverse32((uint32_t)e) >> (32 - root);      // the root bits as a code prefix
        uint32_t ent = max > root ? kLongMark : kBadMark;
        for (int len = 1; len <= top; ++len) {
            const uint32_t d = (rev >> (root - len)) - first[len];
            if (d < cnt[len]) {
                ent = make_entry((uint32_t)len, sorted[ZR_IDX(offs[len] + d, which == kCodeLit ? 288 : 32)]);
                break;
            }
        }
        table[e] = (uint16_t)ent;
    }
    if (lane == 0) cnt[0] = (uint32_t)max;                           // slot 0 is unused by the comparison: keep max there
    wave_sync();
    return 0;
}

// A code longer than the root: the canonical comparison over the remaining lengths, wave-uniform.
template <typename LDS>
__device__ __forceinline__ uint32_t long_code(LDS &L, int which, int root, const uint16_t *sorted,
                                              unsigned long long hold) {
    const uint32_t rev15 = __builtin_bitreverse32((uint32_t)hold & 0x7fffu) >> 17;
    const int max = (int)uni(L.cnt(which)[0]);
    for (int len = root + 1; len <= max; ++len) {
        const uint32_t d = (rev15 >> (15 - len)) - uni(L.first(which)[len]);
        if (d < uni(L.cnt(which)[len])) return make_entry((uint32_t)len, uni(sorted[ZR_IDX(uni(L.offs(which)[len]) + d, which == kCodeLit ? 288 : 32)]));
    }
    return kBadMark;
}

}  // namespace zr
