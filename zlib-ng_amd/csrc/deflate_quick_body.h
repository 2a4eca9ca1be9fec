// deflate_quick_body.h -- the body of deflate_quick_kernel (deflate_stream.hip), included INSIDE the kernels that share it.
// It is program text, not a header in the usual sense: the including function provides
//   jobs, results   the kernel's arguments
//   DICT            constexpr bool: the dictionary form (deflate_quick_dict_kernel, zng_rocm_compress_streams_dict_dev).  The
//                   history is ONE window shared by every stream of the launch (dwin: `start` bytes, zero padded behind) and
//                   its primed head table (dhead: dict_plan.h) is loaded instead of zeroing and priming; position start + i
//                   names plaintext byte i, so job.in is the plaintext's address minus `start` and nothing below in + start
//                   is ever read.  Everything else -- the distance rule, the emit, the checksum -- is the same code.
//   dhead, dwin     the dictionary object's head table and window (null without DICT)
// Textual sharing keeps deflate_quick_kernel the very function it was: same arguments, same attributes, same code.
    __shared__ QuickShared sh;

    const StreamJobDev job = jobs[blockIdx.x];
    const uint8_t *in = job.in;
    const uint32_t n = job.n, start = job.start;
    const bool final_block = (job.flags & ZNG_ROCM_BLOCK_NOT_FINAL) == 0;
    uint32_t *outw = reinterpret_cast<uint32_t *>(job.out);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;

    if constexpr (DICT) {
        for (int i = t; i < (1 << kQuickHashBits) / 4; i += 256)
            reinterpret_cast<uint4 *>(sh.lz.head)[i] = reinterpret_cast<const uint4 *>(dhead)[i];
    } else {
        for (int i = t; i < (1 << kQuickHashBits); i += 256) sh.lz.head[i] = 0;
    }
    // block header: BFINAL, BTYPE = 01 (deflate_quick.c:30-34 emits it through zng_tr_emit_tree(s, STATIC_TREES, last))
    for (int i = t; i < (int)kRingWords; i += 256) sh.ring[i] = i == 0 ? (final_block ? 3u : 2u) : 0u;
    if (t == 0) sh.lz.cover = start;     // nothing below the first plaintext byte is ever produced
    __syncthreads();

    // dictionary priming: the whole batches below `start` only enter their positions into the hash
    uint32_t P0 = DICT ? start : 0u;     // (the shared window is primed already: the first batch begins on the plaintext)
    if constexpr (!DICT) {
        for (; P0 + 256u <= start; P0 += 256u) {
            const uint32_t p = P0 + (uint32_t)t;
            lz_insert_batch<kQuickHashBits, 4>(n, P0, p + kLzMinMatch <= n ? load_u32(in + p) : 0u, &sh.lz, t);
        }
    }

    uint32_t cursor = 3;                 // bits placed so far, modulo 2^32 (uniform over the workgroup)
    uint32_t flushed = 0;                // whole words already written to `out`: the true count (deflate_quick_plan.h)
    uint32_t pend_code = 0, pend_nb = 0, pend_pre = 0;     // this lane's token of the previous batch, not yet placed
    bool have_pending = false;
    unsigned long long accA = 0, accB = 0;                 // Adler-32, linear form: B += (n - pos) * byte

    // place the pending batch: every lane ORs its token at cursor + (bits of the waves before it) + (its wave prefix)
    auto place = [&](int parity) {
        const uint4 wb = sh.wave_bits[parity];
        const uint32_t before = (wave > 0 ? wb.x : 0u) + (wave > 1 ? wb.y : 0u) + (wave > 2 ? wb.z : 0u);
        if (pend_nb) {
            const uint32_t at = cursor + before + pend_pre;
            const uint32_t word = at >> 5;
            const unsigned long long wide = (unsigned long long)pend_code << (at & 31u);     // <= 31 + 31 bits
            atomicOr(&sh.ring[word & (kRingWords - 1u)], (uint32_t)wide);
            atomicOr(&sh.ring[(word + 1) & (kRingWords - 1u)], (uint32_t)(wide >> 32));
        }
        cursor += wb.x + wb.y + wb.z + wb.w;
    };
    // stream out complete words (quick_flush_words, deflate_quick_plan.h); everything below `cursor` was ORed before the last barrier
    auto flush = [&](uint32_t keep_below) {
        const uint32_t bits = quick_pending_bits(cursor, flushed);
        if (quick_flush_due(bits, keep_below)) {
            const uint32_t cnt = quick_flush_count(bits, keep_below);
            const uint32_t end = flushed + cnt;                  // true word indices: below 2^30
            for (uint32_t w = flushed + (uint32_t)t; w < end; w += 256) {
                const uint32_t slot = w & (kRingWords - 1u);
                __builtin_nontemporal_store(sh.ring[slot], outw + w);
                sh.ring[slot] = 0;
            }
            flushed = end;
        }
    };

    u32x4_unaligned own = load_16_guarded(in, P0 + (uint32_t)t, n);  // this lane's 16 bytes of the current batch
    int parity = 0;
    for (uint32_t P = P0; P < n; P += 256) {
        // every position of the NEXT batch has its 16 bytes inside the stream / of this batch its whole lookahead
        const uint32_t pn = P + 256u + (uint32_t)t;
        const bool full = n >= 256u + kStdMaxMatch + 4u && P <= n - (256u + kStdMaxMatch + 4u);
        const bool next_inside = n >= 512u + 16u && P <= n - (512u + 16u);
        u32x4_unaligned own_next = {0u, 0u, 0u, 0u};                           // prefetch of the next batch
        if (next_inside) own_next = load_u128(in + pn);
        else if (pn >= P) own_next = load_16_guarded(in, pn, n);
        const LzPick r = full ? lz_batch<kQuickHashBits, 4, true, DICT>(in, n, P, own, &sh.lz, t, dwin, start)
                              : lz_batch<kQuickHashBits, 4, false, DICT>(in, n, P, own, &sh.lz, t, dwin, start);
        // (lz_batch ended behind barriers: the wave totals and the ORs of the previous iteration are visible)
        flush(kFlushWords);
        if (have_pending) place(parity ^ 1);
        const uint32_t p = P + (uint32_t)t;
        const uint32_t byte = p >= start ? own.x & 0xffu : 0u;   // zero beyond the end of the stream; the dictionary
        accA += byte;                                            // is not part of the checksum
        accB += (unsigned long long)(n - p) * byte;
        // both codes are computed and one is selected: no branch (lanes without a token carry r.len = r.dist = 0,
        // which the match coder turns into harmless garbage that the select drops)
        uint32_t mcode, mnb, lcode, lnb;
        static_match(r.kind == 2u ? r.len : 3u, r.kind == 2u ? r.dist : 1u, mcode, mnb);
        static_literal(byte, lcode, lnb);
        const uint32_t code = r.kind == 2u ? mcode : (r.kind == 1u ? lcode : 0u);
        const uint32_t nb = r.kind == 2u ? mnb : (r.kind == 1u ? lnb : 0u);
        uint32_t incl = nb;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) reinterpret_cast<uint32_t *>(&sh.wave_bits[parity])[wave] = incl;
        pend_code = code;
        pend_nb = nb;
        pend_pre = incl - nb;
        have_pending = true;
        parity ^= 1;
        own = own_next;
    }
    __syncthreads();
    if (have_pending) place(parity ^ 1);
    __syncthreads();
    flush(1);                                                // every complete word

    // Adler-32: every lane reduced before lanes are added (quick_adler_lane: a wave's plain sum passes 2^64 from 726 MiB of 0xff on)
    uint32_t redA = quick_adler_lane(accA), redB = quick_adler_lane(accB);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        redA += (uint32_t)__shfl_xor((int)redA, m, 64);
        redB += (uint32_t)__shfl_xor((int)redB, m, 64);
    }
    if (lane == 0) {
        sh.red_a[wave] = redA;
        sh.red_b[wave] = redB;
    }
    __syncthreads();
    // end-of-block code 256 = seven 0 bits (zng_emit_end_block, trees_emit.h:169-180), then pad to a byte
    if (t == 0) {
        uint8_t *outb = job.out;
        const bool sync = !final_block && (job.flags & ZNG_ROCM_BLOCK_SYNC_FLUSH) != 0;
        const QuickTail tail = quick_tail(cursor, flushed, sync);    // tail.word == flushed: flush(1) wrote every complete word
        uint32_t cw = sh.ring[tail.word & (kRingWords - 1u)];        // the partial word + EOB
        if (tail.spill) {
            outw[tail.word] = cw;
            cw = 0;
        }
        uint32_t bytes = tail.first;
        for (uint32_t k = 0; k < tail.nbytes; ++k) outb[bytes++] = (uint8_t)((unsigned long long)cw >> (8 * k));   // up to 34 bits
        if (sync) {                                          // header of an empty stored block (BFINAL = 0, BTYPE = 00: three 0 bits),
            outb[bytes++] = 0x00;                            // byte aligned, LEN = 0, NLEN = 0xffff: what Z_SYNC_FLUSH
            outb[bytes++] = 0x00;                            // appends (deflate.c:1064-1076, zng_tr_stored_block)
            outb[bytes++] = 0xff;
            outb[bytes++] = 0xff;
        }
        results[2 * blockIdx.x] = tail.bytes;
        results[2 * blockIdx.x + 1] = quick_adler_row(sh.red_a[0] + sh.red_a[1] + sh.red_a[2] + sh.red_a[3],
                                                      sh.red_b[0] + sh.red_b[1] + sh.red_b[2] + sh.red_b[3], n - start);
    }
