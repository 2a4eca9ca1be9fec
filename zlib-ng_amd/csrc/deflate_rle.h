// deflate_rle.h -- the front end of the Z_RLE and Z_HUFFMAN_ONLY strategies (K1 of deflate_dyn.hip for those two):
// deflate_rle.c:30-86 and deflate_huff.c:16-45 of the reference, run on every segment of a device-resident stream at
// once.  It writes exactly what lz_rows_kernel writes -- the token-start bitmap, the u16 distance slots, the cumulative
// histogram snapshots per kSubBytes sub-block -- so that K2..K4 (emit_dynamic_kernel and the packing) run unchanged.
//
// Semantics (strategy codes of zlib-ng.h.in: 2 = Z_HUFFMAN_ONLY, 3 = Z_RLE; levels 1..9 make no difference to either):
//   Z_HUFFMAN_ONLY  every position of the segment is a literal.
//   Z_RLE           the greedy parse of deflate_rle.c, independently per segment [seg_start, seg_end):
//                   position p is a match iff in[p-1] == in[p] == in[p+1] == in[p+2] and p + 3 <= seg_end; its length is
//                   the number of bytes from p on that equal in[p-1], capped at 258 and at the segment end; its distance
//                   is 1.  Otherwise p is a literal.  in[p-1] may lie in the previous segment or in the dict_len history
//                   (what strstart > 0 allows); position 0 of a stream without history is a literal.
//
// The parse needs no serial loop.  A BREAK is a position whose byte differs from the one before it (also position 0, and
// every position outside the segment).  Inside a maximal run the greedy chain starts at o = (last break) + 1, or at
// seg_start when the run began in front of the segment; from o on the tokens are matches of 258 at o + 258 k, and the
// remainder r is one match if r >= 3, otherwise r literals.  So, with j = (p - o) mod 258 for a position p that is no
// break:  p starts a token iff j == 0, or j == 1 and p + 1 is a break (the chain point before it was a literal); it is a
// match iff j == 0 and neither p + 1 nor p + 2 is a break.  A break itself is a literal.  o comes from a workgroup max-scan
// of (break + 1) carried across batches, so runs longer than a batch need nothing special.
//
// Mapping: one workgroup of 4 waves per segment, batches of 4096 positions from the segment's first 1024-aligned position
// (where K1's bitmap begins), 16 positions per lane from one 16-byte load.  The bitmap goes out as one u16 per lane (four
// lanes make a 64-position word), the distance slots of a lane that starts a match as one 8-byte zero store.  The
// histogram is kept in LDS in 16 privatised copies (lane & 15, odd stride), summed into a snapshot every kSubBytes.
// A match's length is the distance to the next break, found by a second (suffix) scan; only the chain point that runs past
// the end of its batch reads ahead in memory (at most one per batch, at most 258 bytes).
#pragma once

namespace zr {

constexpr int      kRleThreads = 256;
constexpr uint32_t kRlePer = 16;                           // positions per lane
constexpr uint32_t kRleBatch = kRlePer * kRleThreads;     // 4096
constexpr int      kRleCopies = 16;                        // privatised histograms
constexpr int      kRleStride = kHistWords + 1;            // odd: one symbol's copies sit on different banks
constexpr uint32_t kRleNone = 0xffffffffu;
static_assert(kSubBytes % kRleBatch == 0, "a sub-block must end on a batch border");
static_assert(kRowBatch % kRlePer == 0, "the bitmap's first word must start at a lane's first position");

template <bool kHuffOnly>
__global__ __launch_bounds__(kRleThreads)
void rle_rows_kernel(const SegJob *__restrict__ jobs, unsigned long long *__restrict__ bm_base, uint16_t *__restrict__ d16_base,
                     uint32_t *__restrict__ hist_out) {
    __shared__ uint32_t hist[kRleCopies * kRleStride];
    __shared__ uint16_t brk_sh[2][kRleThreads + 1];        // per lane: its 16 break bits (+ the next batch's first two)
    __shared__ uint32_t wave_o[2][4], wave_nb[2][4];       // per wave: max (break + 1), min break

    const SegJob job = jobs[blockIdx.x];
    const uint8_t *in = job.in;
    const uint32_t a = job.seg_start, n = job.seg_end;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t first = a - a % kRowBatch;
    uint16_t *bm16 = reinterpret_cast<uint16_t *>(bm_base + job.bm_off);
    uint16_t *d16 = d16_base + job.d16_off;
    uint32_t *hist_seg = hist_out + (size_t)blockIdx.x * kMaxSub * kHistWords;
    uint32_t *my_hist = hist + (lane & (kRleCopies - 1)) * kRleStride;

    for (int i = t; i < kRleCopies * kRleStride; i += kRleThreads) hist[i] = 0;
    __syncthreads();

    auto snapshot = [&](uint32_t sub) {                    // between two barriers: every count is in, none of the next
        for (int s = t; s < kHistWords; s += kRleThreads) {
            uint32_t v = 0;
#pragma unroll
            for (int c = 0; c < kRleCopies; ++c) v += hist[c * kRleStride + s];
            hist_seg[(size_t)sub * kHistWords + s] = v;
        }
    };

    uint32_t carry_o = a;                                  // chain origin if no break has been seen yet
    uint32_t bi = 0;
    for (uint32_t P = first; P < n; P += kRleBatch, ++bi) {
        const int buf = (int)(bi & 1u);
        const uint32_t q0 = P + kRlePer * (uint32_t)t;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (q0 + kRlePer <= n) {
            const u32x4_unaligned raw = load_u128(in + q0);
            w[0] = raw.x; w[1] = raw.y; w[2] = raw.z; w[3] = raw.w;
        } else {
            for (uint32_t q = q0; q < n; ++q) w[(q - q0) >> 2] |= (uint32_t)in[q] << (8u * ((q - q0) & 3u));
        }
        // positions of this lane that belong to the segment, and those whose byte may be compared with the one before
        uint32_t seg_mask = 0, cmp_mask = 0;
        {
            const uint32_t lo = a > q0 ? a - q0 : 0u, hi = n > q0 ? (n - q0 < kRlePer ? n - q0 : kRlePer) : 0u;
            if (lo < hi) seg_mask = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
            cmp_mask = (q0 == 0u) ? (seg_mask & ~1u) : seg_mask;
        }
        uint32_t brk = 0xffffu;
        if (!kHuffOnly) {
            uint32_t prev = (uint32_t)__shfl_up((int)(w[3] >> 24), 1, 64);
            if (lane == 0) prev = (q0 >= 1u && q0 - 1u < n) ? (uint32_t)in[q0 - 1u] : 0u;
            uint32_t eq = 0;
#pragma unroll
            for (int i = 0; i < (int)kRlePer; ++i) {
                const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
                const uint32_t pb = i ? (w[(i - 1) >> 2] >> (8 * ((i - 1) & 3))) & 0xffu : prev;
                eq |= (uint32_t)(b == pb) << i;
            }
            brk = 0xffffu & ~(eq & cmp_mask);
        }
        uint32_t tok = seg_mask, mat = 0;                  // Z_HUFFMAN_ONLY: every position a literal
        uint32_t ext = brk, nb_after = kRleNone;
        if (!kHuffOnly) {
            // scans: o = max over breaks before a position of (break + 1); the first break behind a lane's positions
            const uint32_t my_o = brk ? q0 + (31u - (uint32_t)__clz((int)brk)) + 1u : 0u;
            const uint32_t my_nb = brk ? q0 + (uint32_t)__builtin_ctz(brk) : kRleNone;
            uint32_t inc_o = my_o, inc_nb = my_nb;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)inc_o, d, 64);
                const uint32_t dn = (uint32_t)__shfl_down((int)inc_nb, d, 64);
                if (lane >= d && up > inc_o) inc_o = up;
                if (lane + d < 64 && dn < inc_nb) inc_nb = dn;
            }
            brk_sh[buf][t] = (uint16_t)brk;
            if (t == kRleThreads - 1) {                    // the next batch's first two positions are breaks?
                uint32_t nx = 0;
                for (uint32_t k = 0; k < 2u; ++k) {
                    const uint32_t p = P + kRleBatch + k;
                    if (p >= n || in[p] != in[p - 1u]) nx |= 1u << k;
                }
                brk_sh[buf][kRleThreads] = (uint16_t)nx;
            }
            if (lane == 63) wave_o[buf][wave] = inc_o;
            if (lane == 0) wave_nb[buf][wave] = inc_nb;
            __syncthreads();
            uint32_t ex_o = (uint32_t)__shfl_up((int)inc_o, 1, 64);
            if (lane == 0) ex_o = 0u;
            uint32_t nb = (uint32_t)__shfl_down((int)inc_nb, 1, 64);
            if (lane == 63) nb = kRleNone;
            uint32_t batch_o = carry_o;
            for (int v = 0; v < 4; ++v) {
                const uint32_t wo = wave_o[buf][v], wn = wave_nb[buf][v];
                if (v < wave && wo > ex_o) ex_o = wo;
                if (v > wave && wn < nb) nb = wn;
                if (wo > batch_o) batch_o = wo;
            }
            if (carry_o > ex_o) ex_o = carry_o;
            nb_after = nb;
            carry_o = batch_o;
            ext = brk | ((uint32_t)brk_sh[buf][t + 1] << kRlePer);

            uint32_t j = q0 >= ex_o ? (q0 - ex_o) % 258u : 0u;
            tok = 0;
#pragma unroll
            for (int i = 0; i < (int)kRlePer; ++i) {
                if ((brk >> i) & 1u) {                     // a break: a literal, and the chain restarts behind it
                    tok |= 1u << i;
                    j = 0;
                    continue;
                }
                const bool b1 = (ext >> (i + 1)) & 1u, b2 = (ext >> (i + 2)) & 1u;
                if (j == 0u) {
                    tok |= 1u << i;
                    if (!b1 && !b2) mat |= 1u << i;
                } else if (j == 1u && b1) {
                    tok |= 1u << i;
                }
                j = j + 1u == 258u ? 0u : j + 1u;
            }
            tok &= seg_mask;
            mat &= seg_mask;
        }
        // every bitmap word that holds a position of the segment, nothing behind it (the segment's words end there)
        if ((q0 - first) / 64u <= (n - 1u - first) / 64u) bm16[(q0 - first) / kRlePer] = (uint16_t)tok;
        if (mat) *reinterpret_cast<unsigned long long *>(d16 + (q0 - first) / 4u) = 0ull;     // distance 1 in every slot

        // histogram of this lane's tokens
        const uint32_t lit = tok & ~mat;
#pragma unroll
        for (int i = 0; i < (int)kRlePer; ++i)
            if ((lit >> i) & 1u) atomicAdd(&my_hist[(w[i >> 2] >> (8 * (i & 3))) & 0xffu], 1u);
        if (!kHuffOnly) {
            for (uint32_t m = mat; m; m &= m - 1u) {
                const uint32_t i = (uint32_t)__builtin_ctz(m), p = q0 + i;
                const uint32_t later = (brk >> i) >> 1;    // (brk has no bits above the lane's 16)
                uint32_t e = later ? p + 1u + (uint32_t)__builtin_ctz(later) : nb_after;
                if (e == kRleNone) {                       // no break in the rest of the batch
                    const uint32_t bend = P + kRleBatch;
                    if (p + 258u <= bend) {
                        e = p + 258u;
                    } else {                               // the run goes on past the batch: read ahead
                        const uint32_t v = (w[i >> 2] >> (8 * (i & 3))) & 0xffu, lim = p + 258u < n ? p + 258u : n;
                        const uint32_t rep = v * 0x01010101u;
                        uint32_t q = bend;
                        while (q + 16u <= lim) {
                            const u32x4_unaligned r = load_u128(in + q);
                            const uint32_t x[4] = {r.x ^ rep, r.y ^ rep, r.z ^ rep, r.w ^ rep};
                            uint32_t k = 0;
                            while (k < 4u && x[k] == 0u) ++k;
                            if (k < 4u) {
                                q += 4u * k + ((uint32_t)__builtin_ctz(x[k]) >> 3);
                                break;
                            }
                            q += 16u;
                        }
                        if (q + 16u > lim)
                            while (q < lim && in[q] == v) ++q;
                        e = q;
                    }
                }
                const uint32_t len = e - p < 258u ? e - p : 258u;
                uint32_t sy, eb;
                rows_len_symbol(len, sy, eb);
                atomicAdd(&my_hist[sy], 1u);
                atomicAdd(&my_hist[288], 1u);              // distance 1 = distance symbol 0
            }
        }
        const uint32_t done = (P - first) / kRleBatch + 1u;
        if ((done * kRleBatch) % kSubBytes == 0u && P + kRleBatch < n) {
            __syncthreads();
            snapshot(done * kRleBatch / kSubBytes - 1u);
            __syncthreads();
        }
    }
    __syncthreads();
    const uint32_t span = n - first;                       // the totals: the last sub-block's snapshot
    snapshot(span ? (span + kSubBytes - 1u) / kSubBytes - 1u : 0u);
}

}  // namespace zr
