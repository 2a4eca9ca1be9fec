/* tests/c/coarse_window_driver.c -- TEST: streams opened with a window below 32 KiB (deflateInit2's windowBits 9..14) through
 * integration/arch/rocm/rocm_deflate.c, driven the way deflate(), deflateSetDictionary() and deflateGetDictionary() drive an
 * arch backend.  As in coarse_driver.c only the control flow around the hook macros is restated (deflate.c:826-846 pending
 * bytes, :868-886 the zlib header from s->w_bits, :898-925 the gzip header, :1036-1083 DEFLATE_HOOK and what follows each
 * block_state, :1091-1120 trailers; :456-466 DEFLATE_SET_DICTIONARY_HOOK, :515-522 DEFLATE_GET_DICTIONARY_HOOK).  There is no
 * software deflate here: where the reference would continue in software the driver prints "fallback".
 *   coarse_window_driver d <level> <wrap> <w_bits> <in_chunk> <dict_len> <infile> <outfile>
 *        the first dict_len bytes of the file go to deflateSetDictionary (raw streams only: the driver writes no DICTID), the
 *        rest is compressed in calls of in_chunk bytes -> "device <bytes in> <bytes out>" or "fallback"
 *   coarse_window_driver g <w_bits> <buf_len> <infile> <outfile>
 *        the file is compressed with one Z_SYNC_FLUSH call, then deflateGetDictionary fills a buffer of buf_len bytes that
 *        stands in front of 64 canary bytes -> "dict <length> canary <ok|hit>", the bytes returned in outfile, or "fallback" */
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
    if (!header_done && s->wrap == 1) {                         /* deflate.c:868-886: CINFO from s->w_bits */
        unsigned header = (8u + ((s->w_bits - 8u) << 4)) << 8;
        const unsigned level_flags = (s->strategy >= ROCM_Z_HUFFMAN_ONLY || s->level < 2) ? 0u : s->level < 6 ? 1u : s->level == 6 ? 2u : 3u;
        header |= level_flags << 6;
        header += 31u - header % 31u;
        pend[npend++] = (uint8_t)(header >> 8);
        pend[npend++] = (uint8_t)header;
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

/* deflateSetDictionary / deflateGetDictionary up to their hooks (deflate.c:456-466, :515-522): the hook returns for them */
static int driver_set_dictionary(zng_stream *strm, const uint8_t *dict, unsigned len) {
    DEFLATE_SET_DICTIONARY_HOOK(strm, dict, len);
    return -100;
}
static int driver_get_dictionary(zng_stream *strm, uint8_t *dict, unsigned *len) {
    DEFLATE_GET_DICTIONARY_HOOK(strm, dict, len);
    return -100;
}

static uint8_t *read_file(const char *path, size_t *n) {
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    *n = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *b = malloc(*n + 1);
    if (!b || fread(b, 1, *n, f) != *n) return NULL;
    fclose(f);
    return b;
}

static int write_file(const char *path, const uint8_t *b, size_t n) {
    FILE *fo = fopen(path, "wb");
    if (!fo || fwrite(b, 1, n, fo) != n) return 0;
    return fclose(fo) == 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    rocm_remember_cpu_tier(cpu_adler, cpu_crc);
    zng_stream strm;
    memset(&strm, 0, sizeof strm);
    deflate_state st;
    memset(&st, 0, sizeof st);
    st.strm = &strm;
    strm.state = &st;
    if (argv[1][0] == 'g') {
        if (argc < 6) return 2;
        st.level = 6;
        st.w_bits = (unsigned)atoi(argv[2]);
        const size_t buf_len = (size_t)atol(argv[3]);
        size_t n = 0;
        uint8_t *in = read_file(argv[4], &n);
        if (!in || !buf_len) return 2;
        uint8_t *out = malloc(n + n / 4 + 65536);
        uint8_t *buf = malloc(buf_len + 64);
        if (!out || !buf) return 2;
        memset(buf, 0xA5, buf_len + 64);
        DEFLATE_RESET_KEEP_HOOK(&strm);
        strm.next_in = in;
        strm.avail_in = (uint32_t)n;
        strm.next_out = out;
        strm.avail_out = (uint32_t)(n + n / 4 + 65536);
        int rc = driver_deflate(&strm, Z_SYNC_FLUSH);
        if (rc == -100) {
            printf("fallback\n");
            return 0;
        }
        if (rc != Z_OK || strm.avail_in != 0) return 5;
        unsigned len = 0;
        rc = driver_get_dictionary(&strm, buf, &len);
        if (rc != Z_OK) return 6;
        int canary = 1;
        for (size_t i = 0; i < 64; ++i) canary &= buf[buf_len + i] == 0xA5;
        unsigned only_len = 0;                                  /* dictionary == NULL: the length alone (deflate.c:527-530) */
        if (driver_get_dictionary(&strm, NULL, &only_len) != Z_OK || only_len != len) return 7;
        if (len > buf_len || !write_file(argv[5], buf, len)) return 9;
        DEFLATE_END_HOOK(&strm);
        printf("dict %u canary %s\n", len, canary ? "ok" : "hit");
        return 0;
    }
    if (argv[1][0] != 'd' || argc < 9) return 2;
    st.level = atoi(argv[2]);
    st.wrap = atoi(argv[3]);
    st.w_bits = (unsigned)atoi(argv[4]);
    const size_t in_chunk = (size_t)atol(argv[5]);
    const size_t dict_len = (size_t)atol(argv[6]);
    if (!in_chunk || (dict_len && st.wrap != 0)) return 2;
    size_t n = 0;
    uint8_t *file = read_file(argv[7], &n);
    if (!file || dict_len > n) return 2;
    const uint8_t *in = file + dict_len;
    n -= dict_len;
    const size_t cap = n + n / 4 + (n / in_chunk + 4) * 4096 + 65536;
    uint8_t *out = malloc(cap);
    if (!out) return 2;
    DEFLATE_RESET_KEEP_HOOK(&strm);
    if (dict_len) {
        const int rc = driver_set_dictionary(&strm, file, (unsigned)dict_len);
        if (rc == -100) {
            printf("fallback\n");
            return 0;
        }
        if (rc != Z_OK) return 3;
    }
    size_t fed = 0;
    int rc = Z_OK;
    strm.next_out = out;
    strm.avail_out = (uint32_t)cap;
    while (rc != Z_STREAM_END) {
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
    if (!write_file(argv[8], out, strm.total_out)) return 9;
    printf("device %zu %zu\n", n, (size_t)strm.total_out);
    return 0;
}
