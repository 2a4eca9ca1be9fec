// inflate_block_tables_body.h -- the tables of one fixed-code or dynamic block: the fixed lengths, or the whole dynamic block
// header (HLIT / HDIST / HCLEN, the code-length code, the run coder), through the canonical-code builder of inflate_tables.h.
// Included INSIDE the block loop of the kernels that share it (inflate_streams_body.h, inflate_sizes_kernel), behind the test
// that sends a stored block elsewhere.  Program text, not a header: the including loop provides
//   type                       the block's type, 1 or 2
//   L                          the wave's tables (an InflateLds* of inflate_tables.h)
//   kLitRoot, kDistRoot        the root bits of L.lit and L.dist
//   hold, cnt, append(), bit_pos(), in_len   the bit reader (inflate_bits_body.h)
//   msg, lane                  msg: the verdict word; a refused header sets it and leaves the block loop with `break`
//   tables_ready()             an always-inline lambda, called once the builder's 16-bit entries of both codes are in place:
//                              it turns them into the forms the includer's symbol loop reads
// One text for every reader means the same bits are consumed in front of every fault, in the same order of tests.
        if (type == 1) {
            // fixed codes (RFC 1951 3.2.6, inflate.c:801-813): the same builder, from the fixed lengths
            for (int s = lane; s < 288; s += 64) L.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
            if (lane < 32) L.lens[288 + lane] = 5;
            wave_sync();
            build_code(L, kCodeLit, L.lens, 288, kLitRoot, reinterpret_cast<uint16_t *>(L.lit), L.sorted_lit, lane);
            build_code(L, kCodeDist, L.lens + 288, 32, kDistRoot, reinterpret_cast<uint16_t *>(L.dist), L.sorted_dist, lane);
            tables_ready();
        } else {
            // dynamic block header (inflate.c:814-917)
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
                // an empty code-length code yields one-bit entries of value 0: each reads as length 0
                // (inftrees.c:114-122 + inflate.c:846-849)
                const uint32_t nb = e & 15u, sym = e >> 4;
                hold >>= nb;
                cnt -= nb;
                if (sym < 16) {
                    if (lane == 0) L.lens[ZR_IDX(have, 320)] = (uint8_t)sym;
                    ++have;
                    continue;
                }
                uint32_t rep, val = 0;
                if (sym == 16) {
                    rep = 3u + ((uint32_t)hold & 3u);                 // NEEDBITS(here.bits + 2) comes first (inflate.c:856-864):
                    hold >>= 2;                                       // at the end of a truncated stream the answer is
                    cnt -= 2;                                         // "input ended", not this error
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
                for (uint32_t k = (uint32_t)lane; k < rep; k += 64) L.lens[ZR_IDX(have + k, 320)] = (uint8_t)val;
                have += rep;
            }
            if (msg != kMsgNone) break;
            wave_sync();
            if (bit_pos() > 8ull * in_len) { msg = kMsgStarved; break; }
            if (uni(L.lens[256]) == 0) { msg = kMsgNoEob; break; }
            if (uni((uint32_t)build_code(L, kCodeLit, L.lens, (int)nlen, kLitRoot, reinterpret_cast<uint16_t *>(L.lit), L.sorted_lit, lane))) { msg = kMsgLitLenSet; break; }
            if (uni((uint32_t)build_code(L, kCodeDist, L.lens + nlen, (int)ndist, kDistRoot, reinterpret_cast<uint16_t *>(L.dist),
                                         L.sorted_dist, lane))) {
                msg = kMsgDistSet;
                break;
            }
            tables_ready();
        }
