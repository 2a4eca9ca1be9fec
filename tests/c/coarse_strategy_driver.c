/* tests/c/coarse_strategy_driver.c -- TEST: zlib's strategies through integration/arch/rocm/rocm_deflate.c, driven the
 * way deflate() and deflateParams() drive an arch backend.  As in coarse_driver.c only the control flow around the hook
 * macros is restated (deflate.c:826-846 pending bytes, :868-892 / :898-925 zlib / gzip header, :1036-1083 DEFLATE_HOOK
 * and what follows each block_state, :1091-1120 trailers; deflateParams deflate.c:640-672: DEFLATE_PARAMS_HOOK, then a
 * Z_BLOCK flush, then the new level / strategy).  There is no software deflate here: where the reference would continue
 * in software the driver prints "fallback".
 *   coarse_strategy_driver p
 *        a stream the device has begun: archrocm_deflate_params(level 6, strategy) for strategies 0..4 -> "params r0 .. r4"
 *   coarse_strategy_driver d <level> <wrap> <in_chunk> <strategies> <infile> <outfile>
 *        chunk k of the input is compressed at strategy strategies[k % len] (a string of digits, e.g. "30241"), the
 *        strategy changed between chunks as deflateParams does -> "device <bytes in> <bytes out>" or "fallback". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zng_rocm.h"
#include "zlibng_coarse_min.h"
#include "rocm_functions.h"
#include "rocm_deflate.h"

static uint32_t cpu_adler(uint32_t adler, const uint8_t *buf, size_t len) {
    uint32_t s1 = adler & 0xffff, s2 = (adler >> 16) & 0xffff;
    for (size_t i = 0; i < len; ++i) {
        s1 = (s1 + buf[i]) % 65521u;
        s2 = (s2 + s1) % 65521u;
    }
    return s1 | (s2 << 16);
}
static uint32_t cpu_crc(uint32_t crc, const uint8_t *buf, size_t len) {
    crc = ~crc;
    for (size_t i = 0; i < len; ++i) {
        crc ^= buf[i];
        for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0xedb88320u & (0u - (crc & 1u)));
    }
    return ~crc;
}

static uint8_t pend[32];
static unsigned npend, header_done, finish_state;

static void flush_pending(zng_stream *strm) {                   /* deflate.c:786-812 */
    unsigned n = npend < strm->avail_out ? npend : strm->avail_out;
    memcpy(strm->next_out, pend, n);
    memmove(pend, pend + n, npend - n);
    npend -= n;
    strm->next_out += n;
    strm->avail_out -= n;
    strm->total_out += n;
}

static void put32le(uint32_t v) {
    for (int k = 0; k < 4; ++k) pend[npend++] = (uint8_t)(v >> (8 * k));
}

static int driver_deflate(zng_stream *strm, int flush) {
    deflate_state *s = strm->state;
    if (!header_done && s->wrap == 1) {                         /* deflate.c:868-892 */
        pend[npend++] = 0x78;
        pend[npend++] = 0x9c;
        strm->adler = 1;
    } else if (!header_done && s->wrap == 2) {                  /* deflate.c:898-925, no extra fields */
        static const uint8_t gz[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
        memcpy(pend + npend, gz, 10);
        npend += 10;
        s->crc_fold.value = 0;
    }
    header_done = 1;
    if (npend) {                                                /* deflate.c:826-846 */
        flush_pending(strm);
        if (strm->avail_out == 0) return Z_OK;
    }
    if (strm->avail_in != 0 || (flush != Z_NO_FLUSH && !finish_state)) {      /* deflate.c:1036 */
        block_state bstate;
        if (!DEFLATE_HOOK(strm, flush, &bstate)) return -100;   /* the reference would call deflate_* here */
        if (bstate == finish_started || bstate == finish_done) finish_state = 1;
        if (bstate == need_more || bstate == finish_started) return Z_OK;
        if (bstate == block_done) {
            if (flush != Z_PARTIAL_FLUSH && flush != Z_BLOCK) { /* zng_tr_stored_block(s, NULL, 0, 0) with bi_valid == 0 */
                static const uint8_t marker[5] = {0x00, 0x00, 0x00, 0xff, 0xff};
                memcpy(pend + npend, marker, 5);
                npend += 5;
            }
            flush_pending(strm);
            if (strm->avail_out == 0) return Z_OK;
        }
    }
    if (flush != Z_FINISH) return Z_OK;
    if (s->wrap == 1) {                                         /* deflate.c:1091-1100 */
        pend[npend++] = (uint8_t)(strm->adler >> 24);
        pend[npend++] = (uint8_t)(strm->adler >> 16);
        pend[npend++] = (uint8_t)(strm->adler >> 8);
        pend[npend++] = (uint8_t)strm->adler;
        s->wrap = -1;
    } else if (s->wrap == 2) {                                  /* deflate.c:1101-1120 */
        put32le(s->crc_fold.value);
        put32le((uint32_t)strm->total_in);
        s->wrap = -1;
    }
    flush_pending(strm);
    return npend ? Z_OK : Z_STREAM_END;
}

/* deflateParams (deflate.c:640-672) with the hook in front: a Z_BLOCK flush of what is pending, then the new settings */
static int driver_params(zng_stream *strm, int level, int strategy) {
    deflate_state *s = strm->state;
    int hook_flush = Z_NO_FLUSH;
    DEFLATE_PARAMS_HOOK(strm, level, strategy, &hook_flush);
    if ((s->strategy != strategy || s->level != level) && strm->total_in) {
        const int rc = driver_deflate(strm, Z_BLOCK);
        if (rc == -100) return rc;
        if (rc < 0 || strm->avail_in != 0) return Z_BUF_ERROR;
    }
    s->level = level;
    s->strategy = strategy;
    return Z_OK;
}

static uint8_t *read_file(const char *path, size_t *n) {
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    *n = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *b = malloc(*n + 1);
    if (fread(b, 1, *n, f) != *n) return NULL;
    fclose(f);
    return b;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    rocm_remember_cpu_tier(cpu_adler, cpu_crc);
    zng_stream strm;
    memset(&strm, 0, sizeof strm);
    deflate_state st;
    memset(&st, 0, sizeof st);
    st.strm = &strm;
    st.w_bits = 15;
    strm.state = &st;
    if (argv[1][0] == 'p') {
        st.level = 6;
        st.arch.used = 1;                                       /* the device has produced part of this stream */
        printf("params");
        for (int strategy = ROCM_Z_DEFAULT_STRATEGY; strategy <= ROCM_Z_FIXED; ++strategy)
            printf(" %d", PREFIX(archrocm_deflate_params)(&strm, 6, strategy, NULL));
        printf("\n");
        return 0;
    }
    if (argc < 8) return 2;
    st.level = atoi(argv[2]);
    st.wrap = atoi(argv[3]);
    const size_t in_chunk = (size_t)atol(argv[4]);
    const char *strategies = argv[5];
    const size_t nstrat = strlen(strategies);
    if (!in_chunk || !nstrat) return 2;
    st.strategy = strategies[0] - '0';
    size_t n = 0;
    uint8_t *in = read_file(argv[6], &n);
    if (!in) return 2;
    const size_t cap = n + n / 4 + (n / in_chunk + 4) * 4096 + 65536;
    uint8_t *out = malloc(cap);
    DEFLATE_RESET_KEEP_HOOK(&strm);
    size_t fed = 0;
    int rc = Z_OK;
    strm.next_out = out;
    strm.avail_out = (uint32_t)cap;
    for (size_t k = 0; rc != Z_STREAM_END; ++k) {
        if (k) {
            rc = driver_params(&strm, st.level, strategies[k % nstrat] - '0');
            if (rc == -100) {
                printf("fallback\n");
                return 0;
            }
            if (rc != Z_OK) return 4;
        }
        const size_t c = n - fed < in_chunk ? n - fed : in_chunk;
        strm.next_in = in + fed;
        strm.avail_in = (uint32_t)c;
        fed += c;
        rc = driver_deflate(&strm, fed == n ? Z_FINISH : Z_NO_FLUSH);
        if (rc == -100) {
            printf("fallback\n");
            return 0;
        }
        if (rc < 0 || strm.avail_in != 0) return 5;
        if (fed == n && rc != Z_STREAM_END) return 6;           /* the output buffer holds everything */
    }
    if (strm.total_in != n) return 7;
    if (!DEFLATE_DONE(&strm, Z_FINISH)) return 8;
    DEFLATE_END_HOOK(&strm);
    FILE *fo = fopen(argv[7], "wb");
    if (!fo || fwrite(out, 1, strm.total_out, fo) != strm.total_out) return 9;
    fclose(fo);
    printf("device %zu %zu\n", n, (size_t)strm.total_out);
    return 0;
}
