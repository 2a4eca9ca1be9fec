// inflate_bits_body.h -- the compressed-word fetcher and bit buffer of a wavefront that reads ONE deflate stream, included
// INSIDE the kernels that share it (inflate_streams_body.h, inflate_sizes_kernel).  Program text, not a header: the including
// function provides J (the job, an InflateJobDev), in = J.in as a byte pointer, in_len = the stream's bytes, and lane; it gets
//   hold, cnt    the bit buffer (the next bit is bit 0 of hold) and the number of valid bits in it
//   append()     32 more bits, when cnt <= 32; words behind the end of the input read as zeros
//   seek(b)      restart the buffer at byte b of the stream
//   bit_pos()    stream bits consumed so far
//   lead, total_words, fetch(), cbase, cur, nxt, wnext   the state beneath, for the symbol loops that handle words themselves
    // ---- compressed words: 64 per fetch, the next 64 prefetched -------------------------------------------------
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
