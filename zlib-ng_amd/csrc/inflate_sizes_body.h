// inflate_sizes_body.h -- the body of the sizing kernels, included INSIDE the kernels that share it: inflate_sizes_kernel
// (inflate_sizes.hip: one wavefront per small stream), inflate_size_stream_kernel and inflate_size_parts_kernel
// (inflate_large_size.hip: one wavefront per stream with a 64-bit count, one wavefront per PART of a large stream).  It is
// program text, not a header, as inflate_streams_body.h is for the decoders: the including function provides
//   WIDE     constexpr bool: the count is 64 bits and never saturates; false: 32 bits, saturating at kIsCountMax with
//            "output buffer too small", the decode's own end there (inflate_sizes_plan.h)
//   PARTS    constexpr bool: the wavefront is one part of a stream, as inflate_streams_kernel<PART> is: it begins at bit
//            starts[job], stops behind a block that is not the last when the bit position is exactly one of
//            starts[job + 1 .. jend) (`hit`), and tracks `reach`
//   starts, jend, job   PARTS: the launch's starts, one past the last start of this part's own stream, the part's index
//            (otherwise: null, 0 and anything -- they are named in text that is not compiled into the kernel)
//   J        the job (an InflateJobDev): J.in the stream, in = J.in as a byte pointer, in_len = its bytes; lane
//   hist     the length of the history in front of the output (a part that is not its stream's first: 32768)
//   L        the wave's tables, a SizesLds<kDistRoot, kLitRoot>; kLitRoot, kDistRoot
// and gets, behind the text,
//   count    what the decode's `op` would be (CountT: uint32_t, WIDE uint64_t);  sure: see below;  msg: the verdict
//   last     the BFINAL block was read;  bit_pos(): where the parse ended;  reach, hit (PARTS)
// Textual sharing keeps inflate_sizes_kernel the very function it was: same arguments, same attributes, same code.
    typedef typename std::conditional<WIDE, unsigned long long, uint32_t>::type CountT;
    constexpr bool SAT = !WIDE;
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
    if constexpr (PARTS) {
        const unsigned long long sb = starts[job];
        seek((uint32_t)(sb >> 3));
        hold >>= (uint32_t)(sb & 7ull);
        cnt -= (uint32_t)(sb & 7ull);
    } else {
        seek(0);
    }

    // `count`: what the decode's `op` would be.  `sure`: the count behind the last symbol whose bits were ALL input -- the zero
    // bits behind a truncated stream decode to something too, and the row of such a stream carries this count instead: the
    // bytes inflate() itself delivers for that input, where the decoder's partial count depends on where its flush tests fall.
    // While whole words of input are still to come nothing needs a look (`sure` follows `count` where a word enters the bit
    // buffer); once the last word is in (`tail`), every symbol goes through the general path and is held against the input's end.
    CountT count = 0, sure = 0;
    uint32_t tail = 0;
    uint32_t msg = kMsgNone;
    bool last = false;
    // PARTS: the furthest a distance reached in front of the part; the start the part ended on (inflate_streams_body.h)
    [[maybe_unused]] uint32_t reach = 0, hit = 0xffffffffu;
    // PARTS: does the block that just ended end exactly on a later start of this stream?  (binary search, wave-uniform)
    [[maybe_unused]] auto block_end_stop = [&]() __attribute__((always_inline)) -> bool {
        const unsigned long long b = bit_pos();
        uint32_t lo = job + 1u, hi = jend;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (starts[mid] < b) lo = mid + 1u;
            else hi = mid;
        }
        if (lo < jend && starts[lo] == b) {
            hit = lo;
            return true;
        }
        return false;
    };
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
            if constexpr (PARTS) {
                if (!last && block_end_stop()) break;
            }
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
                    if (wnext > total_words + 2u || (SAT && count > kIsCountMax)) stop = halt = kLitHalt;
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
                msg = SAT && count > kIsCountMax ? kMsgOutFull : kMsgStarved;
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
                            } else if ((SAT && count > kIsCountMax) || is_count_add(&count, len)) {
                                msg = kMsgOutFull;
                                end = 2;
                            } else if constexpr (PARTS) {
                                // (`count` already holds the match: what stood in front of it is count - len)
                                const CountT before = count - len;
                                if (dist > before && dist - (uint32_t)before > reach) reach = dist - (uint32_t)before;
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
        if constexpr (PARTS) {
            if (!last && msg == kMsgNone && block_end_stop()) break;
        }
    }
    if (SAT && count > kIsCountMax) {                    // literals counted past the largest room (see the symbol loop)
        count = kIsCountMax;
        msg = kMsgOutFull;
    }
    if (SAT && sure > kIsCountMax) sure = kIsCountMax;
    // bits that do not exist were consumed: whatever happened after that point, the stream ended early
    if (bit_pos() > 8ull * in_len) msg = kMsgStarved;
