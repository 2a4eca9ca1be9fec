// inflate_streams_body.h -- the body of inflate_streams_kernel (inflate_dev.hip), included INSIDE the kernels that share it.
// It is program text, not a header in the usual sense: the including function provides
//   RING, PART, COMPACT, SUB   the template parameters described in front of inflate_streams_kernel
//   DICT                       constexpr bool: the history of a job is the tail of one shared window that ends at hist_end
//                              (inflate_streams_dict_kernel) instead of the bytes in front of its `out`
//   SPAN                       constexpr bool: the history of a job is ITS OWN window, which ends at spans[job].hist_end, the
//                              decode starts spans[job].start_bit bits (0..7) into the first byte, and reaching out_cap is the
//                              expected end (inflate_streams_span_kernel: one span of an indexed stream)
//   jobs, njobs, results, starts, marks, hist_end, spans   the kernel's arguments (null where a form has none)
// It includes two more pieces of program text, which the sizing kernel (inflate_sizes.hip) includes too: the word fetcher and
// bit buffer (inflate_bits_body.h) and the tables of a fixed-code or dynamic block (inflate_block_tables_body.h).
// Textual sharing keeps every existing instantiation the very function it was: same arguments, same attributes, same code.
// The fast loop leaves for any source in front of the stream (ZR_INFLATE_BEFORE_STREAM); the general copy path is the one
// place that reads such a byte, and it reads hist_end[sp] instead of out[sp] in the dictionary form.
    typedef typename std::conditional<PART, uint16_t, uint8_t>::type T;
    constexpr uint32_t E = 16u / (uint32_t)sizeof(T);   // elements per 16-byte store
    constexpr uint32_t M = RING - 1;
    constexpr uint32_t kFlushAt = RING >= 4096 ? RING / 2 : RING / 4;   // unflushed bytes that trigger a flush
    constexpr uint32_t kPrioStep = 128u << 10;                          // part mode: symbols produced per step of wave priority
    constexpr uint32_t kStoredPiece = RING >= 4096 ? 1024u : RING / 4;  // a stored block enters the ring in pieces of this
    constexpr uint32_t kNear = RING - 258;               // a source this close is still in the ring while the match is written
    // bytes not yet flushed never exceed kFlushAt + 16 + max(258, kStoredPiece); a match of 258 more must not overwrite them
    static_assert(kFlushAt + 16 + kStoredPiece + 258 <= RING - 258, "ring too small for the flush / stored-chunk sizes");
    static_assert(kFlushAt + 258 < kNear, "a source beyond kNear must have left the ring (the fast loop reads it from HBM)");
    constexpr int kDistRoot = PART ? kDistRootPart : kDistRootStream, kLitRoot = PART ? kLitRootPart : kLitRootStream;
    __shared__ typename std::conditional<COMPACT, InflateLdsPart<RING, T, kDistRoot, kLitRoot>, InflateLdsStream<RING, T, kDistRoot, kLitRoot>>::type L;
    const int lane = threadIdx.x;
    const uint32_t job = blockIdx.x;
    if (job >= njobs) return;
    const InflateJobDev J = jobs[job];
    const ZR_GLOBAL uint8_t *const in = (const ZR_GLOBAL uint8_t *)J.in;
    ZR_GLOBAL T *const out = (ZR_GLOBAL T *)J.out;
    const uint32_t in_len = (uint32_t)J.in_len, out_cap = (uint32_t)J.out_cap, dict_len = J.dict_len;
    if (PART && out_cap == 0) return;                    // a part whose earlier result stands (inflate_large.hip reruns only some)
    const uint32_t a0 = (uint32_t)((uintptr_t)J.out & 15u) / (uint32_t)sizeof(T);   // ring slot of position p is (p + a0) & M

#include "inflate_bits_body.h"
    uint32_t reach = 0, hit = 0xffffffffu;               // PART: furthest source in front of the part; the start it ended on
    // SUB: the part's own key; the identity of the block being decoded (1 fixed, H + 2 dynamic) and the next sub-start of
    // that identity ahead (its bit, its index; ~0 = none); handed off; a fixed-code sub-part still in its first block
    const unsigned long long *const keys = starts + njobs;
    // one past the last start of this part's own stream: njobs, or (a batch of streams in one launch, their starts one
    // stream behind the other) what the job carries in `flags` -- a block end or a sub-start is looked for in front of it only
    const uint32_t jend = PART && J.flags ? J.flags : njobs;
    uint32_t *const side = marks;
    unsigned long long entry = 0, cur_id = 0, nextB = ~0ull;
    uint32_t pidx = 0;
    bool handed = false, entering = false, first_open = false;
    if constexpr (SUB) {
        entry = keys[job];
        entering = entry != 0;
        first_open = entry == 1;
        if (lane == 0) side[8 * job + 0] = 0xffffffffu;
    }
    if (PART) {
        const unsigned long long sb = SUB && entry >= 2 ? entry - 2 : starts[job];     // (a dynamic sub-part reads its header first)
        seek((uint32_t)(sb >> 3));
        hold >>= (uint32_t)(sb & 7ull);
        cnt -= (uint32_t)(sb & 7ull);
    } else {
        seek(0);
    }
    const uint8_t *span_hist = nullptr;                  // SPAN: the end of this job's own window
    if constexpr (SPAN) {
        const InflateSpanDev S = spans[job];
        span_hist = S.hist_end;
        hold >>= S.start_bit & 7u;
        cnt -= S.start_bit & 7u;
    }

    uint32_t op = 0, flushed = 0;
    uint32_t msg = kMsgNone;
#ifdef ZR_INFLATE_STATS
    unsigned long long zr_tasm = 0;
    const unsigned long long zr_tstart = __builtin_readcyclecounter();
#endif
    // A run of literals waits in ONE vector register, literal j in lane j (a compare and a select per literal,
    // no LDS access, no EXEC juggling); the run goes to the ring in one ds_write when a match, a flush or the 64th
    // literal comes.  `op` already counts the waiting literals.
    uint32_t litbuf = 0, npend = 0;
    auto dump = [&]() __attribute__((always_inline)) {
        if (npend) {
            if ((uint32_t)lane < npend) L.ring[(a0 + op - npend + (uint32_t)lane) & M] = (T)litbuf;
            npend = 0;
        }
    };
    // ring -> HBM: everything below `limit` (all of it when `final`), in aligned 16-byte stores
    auto flush = [&](uint32_t limit, bool final) __attribute__((always_inline)) {
        if (((a0 + flushed) & (E - 1u)) && flushed < limit) {
            uint32_t h = E - ((a0 + flushed) & (E - 1u));
            if (h > limit - flushed) h = limit - flushed;
            if ((uint32_t)lane < h) out[flushed + lane] = L.ring[(a0 + flushed + lane) & M];
            flushed += h;
        }
        const uint32_t chunks = (limit - flushed) / E;
        for (uint32_t c = (uint32_t)lane; c < chunks; c += 64) {
            const uint32_t p = flushed + E * c;
            *(ZR_GLOBAL u32x4_v *)(out + p) = *reinterpret_cast<const u32x4_v *>(&L.ring[(a0 + p) & M]);
        }
        flushed += E * chunks;
        if (final && flushed < limit) {
            if ((uint32_t)lane < limit - flushed) out[flushed + lane] = L.ring[(a0 + flushed + lane) & M];
            flushed = limit;
        }
        // a later far match may read these bytes back from HBM: have the stores acknowledged first
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_s_waitcnt(0);
        if constexpr (PART) {
            // A call lasts as long as its longest part, and a part that has produced several times what the others do (a
            // block of long copies: 1.4 M symbols from 28 KB) is that part: it gets its instructions issued in front of the
            // waves it shares a SIMD with (tools/micro/copy_cost.py: a copy costs a lone wave 0.49 us, one among twelve 0.66).
            if (flushed >= kPrioStep * 3u) __builtin_amdgcn_s_setprio(3);
            else if (flushed >= kPrioStep * 2u) __builtin_amdgcn_s_setprio(2);
            else if (flushed >= kPrioStep) __builtin_amdgcn_s_setprio(1);
        }
    };
    // Everything that is not decoding happens when the literal run is written out, i.e. once per match or per 64
    // literals: the run goes to the ring (clipped at out_cap: a run may have decoded past it), a flush when one is due,
    // and the test that ends the decode of a truncated stream (the zero bits behind the input decode to something for ever).
    auto service = [&]() __attribute__((always_inline)) {
        if (op > out_cap) {
            const uint32_t fit = npend - (op - out_cap);
            if ((uint32_t)lane < fit) L.ring[(a0 + op - npend + (uint32_t)lane) & M] = (T)litbuf;
            op = out_cap;
            npend = 0;
            msg = kMsgOutFull;
            return;
        }
        dump();
        if (wnext > total_words + 2u) msg = kMsgStarved;     // whole words past the end of the input are in the bit buffer
        if (op - flushed >= kFlushAt) {
            wave_sync();
            flush(op, false);
        }
    };

    // the 16-bit distance entries the builder left in the first half of L.dist -> wide entries, through registers
    auto tables_ready = [&]() __attribute__((always_inline)) { widen_distances<kDistRoot>(L, lane); };

    // (Every lambda above is always_inline: one that is called out of line gets its captures through the stack -- the
    // whole bit-parse state would live in scratch memory.)
    // The control flow below is kept to single-exit loops with an error word (no jumps out of nested loops): every branch
    // here is wave-uniform, and anything else makes the compiler carry loop-exit conditions as lane masks through the
    // hot loop (the first version of this kernel executed 73 scalar instructions per symbol, most of them that).
    // PART: does the block that just ended end exactly on a later start?  (binary search, wave-uniform)
    auto block_end_stop = [&]() __attribute__((always_inline)) -> bool {
        const unsigned long long b = bit_pos();
        uint32_t lo = job + 1u, hi = jend;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (starts[mid] < b) lo = mid + 1u;
            else hi = mid;
        }
        if (lo < jend && starts[lo] == b && (!SUB || keys[lo] == 0)) {     // (a block start sorts first among equal bits)
            hit = lo;
            return true;
        }
        return false;
    };
    // SUB: the first start at index >= i with the current block's identity and a bit >= b (a bounded look: the starts of
    // one identity are consecutive but for a noise candidate now and then; one that is missed only makes a part longer)
    auto next_sub = [&](uint32_t i, unsigned long long b) __attribute__((always_inline)) {
        nextB = ~0ull;
        for (uint32_t k = 0; k < 32u && i < jend; ++k, ++i) {
            const unsigned long long sbit = starts[i];
            if (sbit >= b && keys[i] == cur_id) {
                nextB = sbit;
                pidx = i;
                break;
            }
        }
    };
    // SUB, at a symbol boundary: move past a pending sub-start that lies behind, then hand off when the boundary is it
    auto lands = [&]() __attribute__((always_inline)) -> bool {
        if (nextB == ~0ull) return false;
        const unsigned long long b = bit_pos();
        if (b > nextB) next_sub(pidx + 1u, b);
        if (b != nextB) return false;
        hit = pidx;
        handed = true;
        return true;
    };
    bool last = false;
    while (!last && msg == kMsgNone) {
        if constexpr (SPAN) {
            // a span that is complete at a block end stops in front of the next block: it never looks at bytes it does not need
            // (the waiting literals go to the ring first, clipped at out_cap: service())
            if (op >= out_cap) {
                service();
                if (msg == kMsgNone) msg = kMsgOutFull;
                break;
            }
        }
        if constexpr (PART) {
            // a block starts here: everything in front of it is complete, if the bits it took are all input (the zero bits
            // behind a truncated stream decode to something too).  Stored once per block, so no register holds it.
            if (!SUB && marks) {
                const unsigned long long b = bit_pos();
                if (b <= 8ull * in_len && lane == 0) {
                    marks[4 * job + 0] = op;
                    marks[4 * job + 1] = (uint32_t)b;
                    marks[4 * job + 2] = (uint32_t)(b >> 32);
                    marks[4 * job + 3] = reach;
                }
            }
        }
        uint32_t type = 1;
        unsigned long long hdr_bit = 0;
        if (!(SUB && entering && entry == 1)) {          // (a fixed-code sub-part starts behind a header it never sees)
            if constexpr (SUB) hdr_bit = bit_pos();
            if (cnt < 32) append();
            last = hold & 1u;
            type = (uint32_t)(hold >> 1) & 3u;
            hold >>= 3;
            cnt -= 3;
        }
        if (type == 3) { msg = kMsgBlockType; break; }
        if (SUB && entering && type != (entry == 1 ? 1u : 2u)) { msg = kMsgBlockType; break; }
        if (type == 0) {
            // stored block (inflate.c:759-800): LEN / NLEN at the next byte boundary, then LEN raw bytes
            service();
            if (msg != kMsgNone) break;
            wave_sync();
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
            uint32_t n = len < avail ? len : avail;
            if (n > out_cap - op) n = out_cap - op;
            for (uint32_t done_n = 0; done_n < n;) {
                if (op - flushed >= kFlushAt) flush(op, false);
                const uint32_t piece = n - done_n < kStoredPiece ? n - done_n : kStoredPiece;
                const uint32_t lo = 16u * (uint32_t)lane;
                if (lo < piece) {
                    const ZR_GLOBAL uint8_t *src = in + from + done_n + lo;
                    if (lo + 16u <= piece) {
                        const u32x4_unaligned v = *(const ZR_GLOBAL u32x4_unaligned *)src;
                        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int k = 0; k < 16; ++k) L.ring[(a0 + op + lo + k) & M] = (T)(uint8_t)(w[k >> 2] >> (8 * (k & 3)));
                    } else {
                        for (uint32_t k = 0; lo + k < piece; ++k) L.ring[(a0 + op + lo + k) & M] = src[k];
                    }
                }
                op += piece;
                done_n += piece;
                wave_sync();
            }
            if (len > avail) { msg = kMsgStarved; break; }
            if (n < len) { msg = kMsgOutFull; break; }
            seek(from + len);
            if (PART && !last && block_end_stop()) break;
            continue;
        }
#include "inflate_block_tables_body.h"
        if constexpr (SUB) {
            cur_id = type == 1 ? 1ull : hdr_bit + 2ull;
            if (entering) {                              // into the block at the sub-start's bit
                entering = false;
                const unsigned long long sb = starts[job];
                if (bit_pos() > sb) { msg = kMsgBlockType; break; }
                if (type == 2) {
                    seek((uint32_t)(sb >> 3));
                    hold >>= (uint32_t)(sb & 7ull);
                    cnt -= (uint32_t)(sb & 7ull);
                }
            }
            // the first later start of this block's identity (binary search for the bit, then a short look)
            const unsigned long long b = bit_pos();
            uint32_t lo = job + 1u, hi = jend;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (starts[mid] < b) lo = mid + 1u;
                else hi = mid;
            }
            next_sub(lo, b);
        }

        // ---- symbol loop: the decode AND store halves of inflate_fast (inffast_tpl.h:140-300) -----------------------
        // Each round: the hand-written fast loop (ZR_INFLATE_FAST_LOOP) runs until a symbol needs more than it does, then
        // that ONE symbol is finished here, from the stage the fast loop left it in.
        const uint32_t lds_lit = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)L.lit,
                       lds_dist = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)L.dist,
                       lds_ring = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)L.ring;
        for (;;) {
            if constexpr (SUB) {
                if (lands()) break;                     // a symbol boundary
            }
            if (npend == 64) {
                service();
                if (msg != kMsgNone) break;
            }
            uint32_t stage, len = 0, dist = 0;
            // SUB: the fast loop must not start a symbol at or behind a pending sub-start: it takes no word that ends more
            // than 31 bits behind it (it starts a symbol only with 32 bits in the buffer), and is skipped when the buffer
            // already holds such a word -- those symbols go one at a time through the code below
            bool fast = true;
            uint32_t wlim = 64;
            if constexpr (SUB) {
                if (nextB != ~0ull) {
                    const unsigned long long wB = (nextB + 31ull + 8ull * lead) >> 5;
                    if (wB <= (unsigned long long)wnext) fast = false;
                    else if (wB - cbase < 64ull) wlim = (uint32_t)(wB - cbase);
                }
            }
            if (!fast) {
                stage = 0;
            } else {
                uint32_t widx = wnext - cbase, opb = op - npend + 64u, t0, t1, t2, ee, opx, va, vb, vr, vd0, vd1, vd2, vd3, vd4;
                // no flush is due and the match fits `out` while op + len <= oplim (what service() would test)
                const uint32_t fl = flushed + kFlushAt - 1u, oplim = out_cap < fl ? out_cap : fl;
                const unsigned long long out_addr = (unsigned long long)(uintptr_t)J.out;
                const uint32_t laneb = (uint32_t)lane - 64u;
                cnt -= 32u;                                       // the loop's biased forms (ZR_INFLATE_FAST_LOOP)
                npend -= 64u;
#ifdef ZR_INFLATE_STATS
                const unsigned long long zr_t0 = __builtin_readcyclecounter();
#endif
                if constexpr (SUB) {
                    asm volatile(ZR_INFLATE_FAST_LOOP("ds_read_u16", "ds_write_b16", "global_load_ushort", ZR_INFLATE_BEFORE_PART, "%[wlim]")
                                 : "+{s[40:41]}"(hold), [cnt] "+s"(cnt), [widx] "+s"(widx), [npend] "+s"(npend), [opb] "+s"(opb),
                                   [lit] "+v"(litbuf), [reach] "+s"(reach), [stage] "=&s"(stage), [len] "=&s"(len), [dist] "=&s"(dist), [e] "=&s"(ee),
                                   [t0] "=&s"(t0), [t1] "=&s"(t1), [t2] "=&s"(t2), [op] "=&s"(opx), [va] "=&v"(va), [vb] "=&v"(vb), [vr] "=&v"(vr), [vd0] "=&v"(vd0), [vd1] "=&v"(vd1),
                                   [vd2] "=&v"(vd2), [vd3] "=&v"(vd3), [vd4] "=&v"(vd4)
                                 : [lane] "v"(lane), [laneb] "v"(laneb), [cur] "v"(cur), [a0] "s"(a0), [a0m] "s"(a0 - 64u), [oplim] "s"(oplim), [litb] "s"(lds_lit),
                                   [distb] "s"(lds_dist), [ringb] "s"(lds_ring), [outp] "s"(out_addr), [dictlen] "s"(dict_len), [near] "n"(kNear), [mask] "n"(M), [sh] "n"(1),
                                   [litroot] "n"(kLitRoot), [distroot] "n"(kDistRoot), [o1] "n"(64 * sizeof(T)), [o2] "n"(128 * sizeof(T)),
                                   [o3] "n"(192 * sizeof(T)), [o4] "n"(256 * sizeof(T)), [wlim] "s"(wlim)
                                 : "scc", "vcc", "memory", "s42", "s43", "s44", "s45");
                } else if constexpr (sizeof(T) == 1) {
                    asm volatile(ZR_INFLATE_FAST_LOOP("ds_read_u8", "ds_write_b8", "global_load_ubyte", ZR_INFLATE_BEFORE_STREAM, "64")
                                 : "+{s[40:41]}"(hold), [cnt] "+s"(cnt), [widx] "+s"(widx), [npend] "+s"(npend), [opb] "+s"(opb),
                                   [lit] "+v"(litbuf), [reach] "+s"(reach), [stage] "=&s"(stage), [len] "=&s"(len), [dist] "=&s"(dist), [e] "=&s"(ee),
                                   [t0] "=&s"(t0), [t1] "=&s"(t1), [t2] "=&s"(t2), [op] "=&s"(opx), [va] "=&v"(va), [vb] "=&v"(vb), [vr] "=&v"(vr), [vd0] "=&v"(vd0), [vd1] "=&v"(vd1),
                                   [vd2] "=&v"(vd2), [vd3] "=&v"(vd3), [vd4] "=&v"(vd4)
                                 : [lane] "v"(lane), [laneb] "v"(laneb), [cur] "v"(cur), [a0] "s"(a0), [a0m] "s"(a0 - 64u), [oplim] "s"(oplim), [litb] "s"(lds_lit),
                                   [distb] "s"(lds_dist), [ringb] "s"(lds_ring), [outp] "s"(out_addr), [dictlen] "s"(dict_len), [near] "n"(kNear), [mask] "n"(M), [sh] "n"(0),
                                   [litroot] "n"(kLitRoot), [distroot] "n"(kDistRoot), [o1] "n"(64 * sizeof(T)), [o2] "n"(128 * sizeof(T)),
                                   [o3] "n"(192 * sizeof(T)), [o4] "n"(256 * sizeof(T))
                                 : "scc", "vcc", "memory", "s42", "s43", "s44", "s45");
                } else {
                    asm volatile(ZR_INFLATE_FAST_LOOP("ds_read_u16", "ds_write_b16", "global_load_ushort", ZR_INFLATE_BEFORE_PART, "64")
                                 : "+{s[40:41]}"(hold), [cnt] "+s"(cnt), [widx] "+s"(widx), [npend] "+s"(npend), [opb] "+s"(opb),
                                   [lit] "+v"(litbuf), [reach] "+s"(reach), [stage] "=&s"(stage), [len] "=&s"(len), [dist] "=&s"(dist), [e] "=&s"(ee),
                                   [t0] "=&s"(t0), [t1] "=&s"(t1), [t2] "=&s"(t2), [op] "=&s"(opx), [va] "=&v"(va), [vb] "=&v"(vb), [vr] "=&v"(vr), [vd0] "=&v"(vd0), [vd1] "=&v"(vd1),
                                   [vd2] "=&v"(vd2), [vd3] "=&v"(vd3), [vd4] "=&v"(vd4)
                                 : [lane] "v"(lane), [laneb] "v"(laneb), [cur] "v"(cur), [a0] "s"(a0), [a0m] "s"(a0 - 64u), [oplim] "s"(oplim), [litb] "s"(lds_lit),
                                   [distb] "s"(lds_dist), [ringb] "s"(lds_ring), [outp] "s"(out_addr), [dictlen] "s"(dict_len), [near] "n"(kNear), [mask] "n"(M), [sh] "n"(1),
                                   [litroot] "n"(kLitRoot), [distroot] "n"(kDistRoot), [o1] "n"(64 * sizeof(T)), [o2] "n"(128 * sizeof(T)),
                                   [o3] "n"(192 * sizeof(T)), [o4] "n"(256 * sizeof(T))
                                 : "scc", "vcc", "memory", "s42", "s43", "s44", "s45");
                }
#ifdef ZR_INFLATE_STATS
                zr_tasm += __builtin_readcyclecounter() - zr_t0;
#endif
                cnt += 32u;
                npend += 64u;
                opb -= 64u;
                wnext = cbase + widx;
                if (widx == 64) {                                                     // the 64 fetched words are used up
                    cbase += 64;
                    cur = nxt;
                    nxt = fetch(cbase + 64);
                }
                op = opb + npend;
                ZR_STAT(0);
                if (stage == 0) ZR_STAT(npend == 64 ? 1 : widx == 64 ? 2 : 3);          // 64 literals wait / the fetched words are used up / EOB, long or bad code
                if (stage == 1) ZR_STAT(widx == 64 ? 4 : 5);                          // words used up / long or bad distance code
                if (stage == 2) ZR_STAT(len > 64 ? 6 : op + len > oplim ? 7 : dist > op ? 8 : dist < len ? 9 : 10);
                if (stage == 0 && npend == 64) continue;
                if constexpr (SUB) {
                    // the word limit stops the fast loop at the last boundary in front of the pending sub-start's word,
                    // and that boundary is often the sub-start itself: compare before the symbol there is decoded
                    if (stage == 0 && lands()) break;
                }
            }
            if (stage == 0) {
                if (cnt < 32) append();
                uint32_t e = uni(L.lit[(uint32_t)hold & ((1u << kLitRoot) - 1u)]);
                if (e == kLongMark) e = long_code(L, kCodeLit, kLitRoot, L.sorted_lit, hold);
                if (e < (256u << 4)) {                                                // a literal (here: one with a long code)
                    const uint32_t nb = e & 15u;
                    hold >>= nb;
                    cnt -= nb;
                    litbuf = (uint32_t)lane == npend ? (e >> 4) : litbuf;
                    ++npend;
                    ++op;
                    continue;
                }
                const uint32_t sym = e >> 4, nb = e & 15u;
                if (sym > 285u) {                                                     // 286, 287 (inftrees.c:44-45), no code
                    msg = bit_pos() + nb > 8ull * in_len ? kMsgStarved : kMsgLitLenCode;   // (its bits must all be input)
                    break;
                }
                hold >>= nb;
                cnt -= nb;
                if (sym == 256u) {                                                    // end of block
                    if constexpr (SUB) {
                        if (first_open) {                    // a fixed-code sub-part's first block: where it ended
                            first_open = false;
                            const unsigned long long b = bit_pos();
                            if (lane == 0) {
                                side[8 * job + 0] = op;
                                side[8 * job + 1] = (uint32_t)b;
                                side[8 * job + 2] = (uint32_t)(b >> 32);
                                side[8 * job + 3] = reach;
                            }
                        }
                    }
                    break;
                }
                // length: base and extra bits from the symbol (RFC 1951 3.2.5; inftrees.c:38-45 tabulate the same)
                const uint32_t k = sym - 257u;
                if (k < 8u) {
                    len = 3u + k;
                } else if (k == 28u) {
                    len = 258u;
                } else {
                    const uint32_t xb = (k - 4u) >> 2;
                    len = 3u + ((4u + (k & 3u)) << xb) + ((uint32_t)hold & ((1u << xb) - 1u));
                    hold >>= xb;
                    cnt -= xb;
                }
            }
            if (stage <= 1) {
                if (cnt < 32) append();
                uint32_t d = uni(L.dist[(uint32_t)hold & ((1u << kDistRoot) - 1u)]);
                if (d >= kBadWide) {
                    if (d == kLongWide) d = wide_distance(long_code(L, kCodeDist, kDistRoot, L.sorted_dist, hold));
                    if (d >= kBadWide) {
                        msg = bit_pos() + (d & 15u) > 8ull * in_len ? kMsgStarved : kMsgDistCode;
                        break;
                    }
                }
                const uint32_t dnb = d & 15u, dxb = (d >> 4) & 15u;
                hold >>= dnb;
                dist = (d >> 8) + ((uint32_t)hold & ((1u << dxb) - 1u));
                hold >>= dxb;
                cnt -= dnb + dxb;
            }
            if (dist > op + dict_len) { msg = kMsgTooFar; break; }                    // inffast_tpl.h:203-210
            if (PART && dist > op && dist - op > reach) reach = dist - op;
            service();
            if (msg != kMsgNone) break;
            [[maybe_unused]] bool span_full = false;
            if constexpr (SPAN) {
                // the span ends inside this copy: its front is copied, and that is the end
                if (len > out_cap - op) {
                    len = out_cap - op;
                    span_full = true;
                }
            } else {
                if (len > out_cap - op) { msg = kMsgOutFull; break; }
            }
            wave_sync();                                                              // earlier literals are in the ring
            const int src0 = (int)op - (int)dist;
            if (dist <= kNear && dist <= op && dist >= len && len <= 64u) {
                // the common shape, one pass, no loop: a short match that does not overlap itself, source in the ring
                if ((uint32_t)lane < len)
                    L.ring[(a0 + op + (uint32_t)lane) & M] = L.ring[(a0 + (uint32_t)src0 + (uint32_t)lane) & M];
            } else if (dist <= kNear && dist <= op) {
                // ring to ring.  Every source byte was produced before this match began (with dist < len the
                // sources are the `dist` bytes before op, repeated): the passes of the copy are independent.
                if (dist >= len) {
                    for (uint32_t i = (uint32_t)lane; i < len; i += 64)
                        L.ring[(a0 + op + i) & M] = L.ring[(a0 + (uint32_t)src0 + i) & M];
                } else if (dist == 1) {
                    const T v = L.ring[(a0 + (uint32_t)src0) & M];
                    for (uint32_t i = (uint32_t)lane; i < len; i += 64) L.ring[(a0 + op + i) & M] = v;
                } else {
                    const float inv = 1.0f / (float)dist;
                    for (uint32_t i = (uint32_t)lane; i < len; i += 64) {
                        uint32_t q = (uint32_t)((float)i * inv);
                        int r = (int)i - (int)(q * dist);
                        if (r < 0) r += (int)dist;
                        if (r >= (int)dist) r -= (int)dist;
                        L.ring[(a0 + op + i) & M] = L.ring[(a0 + (uint32_t)src0 + (uint32_t)r) & M];
                    }
                }
            } else {
                // a source beyond the ring's reach, or in the history in front of `out`: HBM, except for the bytes
                // that have not left the ring yet (a match that starts in the dictionary and runs into this stream)
                const float inv = 1.0f / (float)dist;
                for (uint32_t i = (uint32_t)lane; i < len; i += 64) {
                    uint32_t j = i;
                    if (dist < len) {
                        uint32_t q = (uint32_t)((float)i * inv);
                        int r = (int)i - (int)(q * dist);
                        if (r < 0) r += (int)dist;
                        if (r >= (int)dist) r -= (int)dist;
                        j = (uint32_t)r;
                    }
                    const int sp = src0 + (int)j;
                    T v;
                    if (sp >= (int)flushed) v = L.ring[(a0 + (uint32_t)sp) & M];
                    else if (PART && sp < 0) v = (T)(256 + 32768 + sp);      // a byte of the 32 KiB in front of this part
                    else if (DICT && sp < 0) v = (T)hist_end[sp];            // a byte of the shared window
                    else if (SPAN && sp < 0) v = (T)span_hist[sp];           // a byte of the job's own window
                    else v = out[sp];
                    L.ring[(a0 + op + i) & M] = v;
                }
            }
            op += len;
            if constexpr (SPAN) {
                if (span_full) { msg = kMsgOutFull; break; }
            }
        }
        if (SUB && handed) break;
        if (PART && !last && msg == kMsgNone && block_end_stop()) break;
    }
#ifdef ZR_INFLATE_STATS
    if (lane == 0) {
        const unsigned long long zr_tend = __builtin_readcyclecounter();
        atomicAdd(&g_inflate_stats[11], zr_tasm);
        atomicAdd(&g_inflate_stats[12], zr_tend - zr_tstart);
        if (job < 16384u) {
            g_inflate_span[2 * job] = zr_tstart;
            g_inflate_span[2 * job + 1] = zr_tend;
        }
    }
#endif
    // bits that do not exist were consumed: whatever happened after that point, the stream ended early
    if (msg != kMsgOutFull) service();                   // (an out-of-room exit has clipped the run already)
    // (a part keeps its out-of-room exit: inflate_large.hip gives it a larger slot and runs it again)
    if (!(PART && msg == kMsgOutFull) && bit_pos() > 8ull * in_len) msg = kMsgStarved;
    wave_sync();
    flush(op, true);
    if (PART) {
        if (lane == 0) {
            const unsigned long long b = bit_pos();
            results[8 * job + 0] = op;
            results[8 * job + 1] = (uint32_t)b;
            results[8 * job + 2] = (uint32_t)(b >> 32);
            results[8 * job + 3] = msg == kMsgNone ? (last && !handed ? 1u : 0u) : (msg == kMsgStarved || msg == kMsgOutFull) ? (uint32_t)-5 : (uint32_t)-3;
            results[8 * job + 4] = msg;
            results[8 * job + 5] = reach;
            results[8 * job + 6] = hit;
            results[8 * job + 7] = last ? 1u : 0u;
            if constexpr (SUB) {
                side[8 * job + 4] = handed ? 1u : 0u;
                side[8 * job + 5] = first_open ? 2u : last ? 1u : 0u;
            }
        }
        return;
    }
    if constexpr (SPAN) {
        if (msg == kMsgOutFull) msg = kMsgNone;         // out_cap bytes are in place: the span's expected end, status 1
    }
    if (lane == 0) {
        const unsigned long long used = (bit_pos() + 7ull) >> 3;
        results[4 * job + 0] = op;
        results[4 * job + 1] = used > in_len ? in_len : (uint32_t)used;
        results[4 * job + 2] = msg == kMsgNone ? 1u : (msg == kMsgStarved || msg == kMsgOutFull) ? (uint32_t)-5 : (uint32_t)-3;
        results[4 * job + 3] = msg;
    }
