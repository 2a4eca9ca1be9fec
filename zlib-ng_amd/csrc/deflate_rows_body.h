// deflate_rows_body.h -- the body of lz_rows_kernel (deflate_dyn.hip), included INSIDE the kernels that share it.  It is
// program text, not a header in the usual sense: the including function provides
//   sh                       __shared__ RowShared
//   jobs, bm_base, d16_base, hist_out, max_cand, stamp_out     the kernel's arguments
//   DICT                     constexpr bool: the dictionary form (lz_rows_dict_kernel, zng_rocm_compress_streams2_dict_dev).  The
//                            history of every stream's FIRST segment (seg_start == dW) is ONE window shared by the launch:
//                            position q < dW names window byte q, position dW + i plaintext byte i, so job.in is the
//                            plaintext's address minus dW and nothing below in + dW is ever read.  Such a segment loads the
//                            row tables the priming of [0, T) leaves (T = dict_rows_primed(dW), dict_plan.h) and the ring
//                            from the object and begins its batches at T; everything behind that -- the priming batch that
//                            may be left, the searches, the parse, the tokens -- is the same code on the same state, so the
//                            tokens are those of lz_rows_kernel over the window copied in front of the plaintext.
//   dwin, dtab, dW           the object's window (16-byte aligned, zero padded), its tables (pos | tag | cnt) and W; null / 0
//                            without DICT
//   wdist, wprime            the window: the furthest a match reaches back (MAX_DIST(s), deflate.h:410-415; read in rows_compare
//                            alone) and the bytes of history a segment enters in front of itself.  lz_rows_kernel and
//                            lz_rows_dict_kernel define them as the compile-time constants kLzMaxDist and kPrime; the window form
//                            (lz_rows_win_kernel, windowBits 9..14) takes them as arguments: (1 << w) - 262 and 1 << w.
// Textual sharing keeps lz_rows_kernel the very function it was: same arguments, same attributes, same code.
    const SegJob job = jobs[blockIdx.x];
    const uint8_t *in = job.in;
    const uint32_t n = job.seg_end;                 // matches never run past the segment
    const int t = threadIdx.x, lane = t & 63;

    // DICT: is this a stream's first segment, behind the shared window?  Then the tables come from the object.
    if constexpr (DICT) {
        if (dW != 0u && job.seg_start == dW) {
            const uint4 *src = dtab;
            for (int i = t; i < (int)(kDictRowsPosBytes / 16u); i += kRowBatch) reinterpret_cast<uint4 *>(sh.pos)[i] = src[i];
            src += kDictRowsPosBytes / 16u;
            for (int i = t; i < (int)(kDictRowsTagBytes / 16u); i += kRowBatch) reinterpret_cast<uint4 *>(sh.tag)[i] = src[i];
            src += kDictRowsTagBytes / 16u;
            for (int i = t; i < (int)(kDictRowsCntBytes / 16u); i += kRowBatch) reinterpret_cast<uint4 *>(sh.cnt)[i] = src[i];
        } else {
            for (int i = t; i < kRows * kRowEnt / 2; i += kRowBatch) reinterpret_cast<uint32_t *>(sh.pos)[i] = 0;
            for (int i = t; i < kRows * kRowEnt / 4; i += kRowBatch) reinterpret_cast<uint32_t *>(sh.tag)[i] = 0;
            for (int i = t; i < kRows / 4; i += kRowBatch) sh.cnt[i] = 0;
        }
    } else {
        for (int i = t; i < kRows * kRowEnt / 2; i += kRowBatch) reinterpret_cast<uint32_t *>(sh.pos)[i] = 0;
        for (int i = t; i < kRows * kRowEnt / 4; i += kRowBatch) reinterpret_cast<uint32_t *>(sh.tag)[i] = 0;
        for (int i = t; i < kRows / 4; i += kRowBatch) sh.cnt[i] = 0;
    }
    if (t < 288) {
        sh.hist_l[t] = 0;
        // before the segment has tokens of its own: 8 bits per literal, 7 per length symbol, 5 per distance symbol
        sh.cost_l[t] = (uint16_t)((t < 256 ? 8u : 7u) * kCostBit);
    } else if (t < 320) {
        sh.hist_d[t - 288] = 0;
        sh.cost_d[t - 288] = (uint16_t)(5u * kCostBit);
    }
    if (t == 0) {
        sh.cover = job.seg_start;
        sh.tot_l = sh.tot_d = 0;
    }

    uint32_t P0 = job.seg_start > wprime ? job.seg_start - wprime : 0u;
    P0 -= P0 % kRowBatch;
    const uint32_t first = job.seg_start - job.seg_start % kRowBatch;   // batch holding the segment's first byte
    unsigned long long *bm = bm_base + job.bm_off;
    uint16_t *d16 = d16_base + job.d16_off;

    // chunk [F, F + 1024) of the plaintext, one dword per lane of the first four waves; bytes at or beyond n read 0
    auto fetch = [&](uint32_t F) -> uint32_t {
        const uint32_t q = F + 4u * (uint32_t)t;
        if (t >= 256 || q >= n) return 0u;
        if constexpr (DICT) {
            if (q < dW) {                           // (dW <= n: the window lies in front of every segment)
                if (q + 4u <= dW) return load_u32(dwin + q);
                uint32_t v = 0;                     // the dword that straddles the window's end
                for (uint32_t j = 0; j < 4u && q + j < n; ++j)
                    v |= (uint32_t)load_u8(q + j < dW ? dwin + q + j : in + q + j) << (8u * j);
                return v;
            }
        }
        if (q + 4u <= n) return load_u32(in + q);
        uint32_t v = 0;
        for (uint32_t j = 0; q + j < n; ++j) v |= (uint32_t)load_u8(in + q + j) << (8u * j);
        return v;
    };
    auto put = [&](uint32_t F, uint32_t v) {
        if (t < 256) {
            const uint32_t idx = (F + 4u * (uint32_t)t) & (kRingBytes - 1u);
            *reinterpret_cast<uint32_t *>(sh.ring + idx) = v;
            if (idx < kRingMirror) *reinterpret_cast<uint32_t *>(sh.ring + kRingBytes + idx) = v;
        }
    };
    // The 2 KiB in front of the loop's first batch.  DICT, a first segment: the loop begins at T with P0 = 0 -- the ring holds
    // the window from its first byte, as if the batches [0, T) had run.  The whole 1 KiB chunks inside the window come in
    // 16-byte pieces from all lanes, the rest as every batch brings its chunks.
    [[maybe_unused]] uint32_t Pstart = P0, Pfill = P0;
    if constexpr (DICT) {
        if (dW != 0u && job.seg_start == dW) {
            Pstart = dict_rows_primed(dW);
            Pfill = dW - dW % kRowBatch;
            for (uint32_t i = (uint32_t)t; i < Pfill / 16u; i += kRowBatch) {
                const uint4 v = reinterpret_cast<const uint4 *>(dwin)[i];
                reinterpret_cast<uint4 *>(sh.ring)[i] = v;
                if (i < kRingMirror / 16u) reinterpret_cast<uint4 *>(sh.ring + kRingBytes)[i] = v;
            }
        }
    }
    uint32_t chunk;
    if constexpr (DICT) {
        for (uint32_t F = Pfill; F < Pstart + kRingAhead; F += 1024u) put(F, fetch(F));
        chunk = fetch(Pstart + kRingAhead);          // stored at the top of the FIRST batch: [Pstart + 2048, Pstart + 3072)
    } else {                                         // (the plain kernel's own three lines: its code stays what it was)
        put(P0, fetch(P0));
        put(P0 + 1024u, fetch(P0 + 1024u));
        chunk = fetch(P0 + 2048u);
    }
    __syncthreads();

    // the tokens of a finished batch: bitmap word, distances, histogram
    auto emit_tokens = [&](uint32_t Pb, const RowsToken &r, unsigned long long starts) __attribute__((always_inline)) {
        const uint32_t p = Pb + (uint32_t)t;
        const unsigned long long matches = __ballot(r.kind == 2u);
        if (lane == 0) {
            bm[(Pb - first) / 64u + (uint32_t)(t >> 6)] = starts;
            const uint32_t nt = (uint32_t)__popcll(starts), nm = (uint32_t)__popcll(matches);
            if (nt) atomicAdd(&sh.tot_l, nt);
            if (nm) atomicAdd(&sh.tot_d, nm);
        }
        if (r.kind == 2u) {
            uint32_t sy, eb;
            rows_len_symbol(r.len, sy, eb);
            atomicAdd(&sh.hist_l[sy], 1u);
            rows_dist_symbol(r.dist, sy, eb);
            atomicAdd(&sh.hist_d[sy], 1u);
            d16[(p - first) >> 2] = (uint16_t)(r.dist - 1u);
        } else if (r.kind == 1u) {
            atomicAdd(&sh.hist_l[sh.ring[p & (kRingBytes - 1u)]], 1u);
        }
    };

    // Two batches in flight: the compares of batch P (LDS-bound) run beside the parse of the batch before it (VALU-bound);
    // waves 4-7 and 12-15 take the two in the opposite order, so every SIMD has both kinds of work at any time.
    const int wave_id = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool parse_first = ((wave_id >> 2) & 1) != 0;
    int since_refresh = 0, snap_due = -1;            // a histogram snapshot (sub-block index) to write once every wave's counts are in
    uint32_t *hist_seg = hist_out + (size_t)blockIdx.x * kMaxSub * kHistWords;
    bool have_prev = false;
    uint32_t P_prev = 0;
    RowsMatch prev;
    prev.L = prev.dist = prev.val = 0;
    for (uint32_t P = Pstart;; P += kRowBatch) {
        const bool live = P < n;                    // one more round after the last batch: its parse
        if (!live && !have_prev) break;
        if (live) {
            put(P + kRingAhead, chunk);             // [P + 2048, P + 3072): what the NEXT batch reads beyond its own positions
            chunk = fetch(P + kRingAhead + 1024u);
        }
        const uint32_t p = P + (uint32_t)t;
        if (live && P < first) {                    // priming: enter the positions, nothing else
            const bool can = p + kLzMinMatch <= n;
            uint32_t row, tag;
            row_key(ring_u32(sh.ring, p & (kRingBytes - 1u)), row, tag);
            rows_insert(&sh, can, row, tag, p, wave_id);
            continue;
        }
        RowsFront f;
        uint32_t cover_in;
        if (live) {
            const bool refresh = since_refresh >= kRefreshBatches;
            since_refresh = refresh ? 1 : since_refresh + 1;
            rows_front(n, P, &sh, t, refresh, f, &cover_in);
        } else {
            rows_barrier();
            cover_in = sh.cover;
        }
        if (snap_due >= 0) {                        // the barriers above are behind the last batch's histogram updates
            if (t < kHistWords) hist_seg[(size_t)snap_due * kHistWords + t] = t < 288 ? sh.hist_l[t] : sh.hist_d[t - 288];
            snap_due = -1;
        }
        RowsMatch cur;
        cur.L = cur.dist = cur.val = 0;
        uint32_t CH = 1u;
#pragma nounroll
        for (int ph = 0; ph < 2; ++ph) {            // ONE copy of each piece in the code, the order a run-time matter
            if ((ph == 0) == parse_first) {
                if (have_prev) CH = rows_parse(n, P_prev, &sh, t, prev);
            } else if (live) {
                cur = rows_compare(n, P, P0, &sh, t, max_cand, f, wdist);       // P0: the lowest position the ring holds
            }
        }
        if (have_prev) {
            unsigned long long starts;
            const RowsToken r = rows_finish(n, P_prev, &sh, t, CH, prev.dist, cover_in, &starts);
            emit_tokens(P_prev, r, starts);
            const uint32_t done_batches = (P_prev - first) / kRowBatch + 1u;
            if (done_batches % kSubBatches == 0) snap_due = (int)(done_batches / kSubBatches) - 1;
        }
#ifdef ZR_ROWS_STAMPS
        if (lane == 0) sh.stamps[t >> 6][8] = __builtin_amdgcn_s_memtime();
        if (blockIdx.x == 3 && stamp_out && lane < 9 && live && P >= first + 64u * kRowBatch && P < first + 96u * kRowBatch)
            stamp_out[(((P - first) / kRowBatch - 64u) * kRowWaves + (uint32_t)(t >> 6)) * 9u + (uint32_t)lane] = sh.stamps[t >> 6][lane];
#endif
        if (!live) break;
        prev = cur;
        P_prev = P;
        have_prev = true;
    }
    __syncthreads();
    {                                                // the totals: the last sub-block's snapshot
        const uint32_t span = n - first;
        const uint32_t nsub = span ? (span + kSubBytes - 1) / kSubBytes : 1u;
        if (t < kHistWords) hist_seg[(size_t)(nsub - 1u) * kHistWords + t] = t < 288 ? sh.hist_l[t] : sh.hist_d[t - 288];
    }
