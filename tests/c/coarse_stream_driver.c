/* tests/c/coarse_stream_driver.c -- TEST: drives integration/arch/rocm/rocm_inflate.c the way inflate() drives an arch
 * backend, with the input handed over in pieces that end at given offsets (a request / response peer reading a
 * sync-flushed stream).  driver_inflate() restates only the control flow around INFLATE_TYPEDO_HOOK (inflate.c:509-555
 * zlib header, :728 TYPEDO, :1105-1147 CHECK), as tests/c/coarse_driver.c does; there is no software inflate here: where
 * the reference would continue in software the driver prints "fallback" and stops.
 *   coarse_stream_driver <wrap> <out_chunk> <infile> <cutsfile> <outfile> [tailfile]
 * cutsfile: ascending byte offsets (text, one per line) into infile + tailfile at which pieces end.  After each piece
 * inflate() is called until it makes no more progress, then "piece <fed> <produced> <in_cap> <parts>" is printed
 * (parts: of the last device call, zng_rocm_inflate_large_last_parts).  At the end:
 * "end <total_in> <avail_in> <produced>" after Z_STREAM_END, or "data error: <msg>"; the plaintext goes to outfile.
 * COARSE_STREAM_PASSES=n (environment): the whole feed n times over, the hook reset in between as inflateReset() does,
 * each pass timed ("seconds <wall time of the pass>", printed in front of the final line; tools/hook_stream_rate.py). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "zng_rocm.h"
#include "zlibng_coarse_min.h"
#include "rocm_functions.h"
#include "rocm_inflate.h"

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

#define RESTORE() do { } while (0)
#define LOAD() do { } while (0)
enum { D_HEAD = 1 };

static int driver_inflate(zng_stream *strm, int flush) {
    struct inflate_state *state = (struct inflate_state *)strm->state;
    int ret = Z_OK;
    const uint32_t in0 = strm->avail_in, out0 = strm->avail_out;
    for (;;) {
        switch ((int)state->mode) {
        case D_HEAD:                                            /* inflate.c:509-555, zlib wrapper only */
            if (state->wrap == 0) {
                state->mode = TYPEDO;
                break;
            }
            if (strm->avail_in < 2) goto inf_leave;
            if (((strm->next_in[0] << 8) + strm->next_in[1]) % 31 || (strm->next_in[0] & 0xf) != 8) {
                strm->msg = "incorrect header check";
                state->mode = BAD;
                break;
            }
            strm->next_in += 2;
            strm->avail_in -= 2;
            strm->adler = state->check = 1;
            state->mode = TYPEDO;
            break;
        case TYPEDO:
            INFLATE_TYPEDO_HOOK(strm, flush);
            return -100;                                        /* the reference would decode the block in software here */
        case CHECK:                                             /* inflate.c:1105-1147 */
            if (state->wrap) {
                if (strm->avail_in < 4) goto inf_leave;
                const uint32_t want = ((uint32_t)strm->next_in[0] << 24) | ((uint32_t)strm->next_in[1] << 16) |
                                      ((uint32_t)strm->next_in[2] << 8) | strm->next_in[3];
                strm->next_in += 4;
                strm->avail_in -= 4;
                if (want != state->check) {
                    strm->msg = "incorrect data check";
                    state->mode = BAD;
                    break;
                }
            }
            state->mode = DONE;
            break;
        case DONE:
            ret = Z_STREAM_END;
            goto inf_leave;
        case BAD:
            ret = Z_DATA_ERROR;
            goto inf_leave;
        default:
            return Z_STREAM_ERROR;
        }
    }
inf_leave:
    strm->total_in += in0 - strm->avail_in;                     /* inflate.c:1185-1188 */
    strm->total_out += out0 - strm->avail_out;
    if (((in0 == strm->avail_in && out0 == strm->avail_out) || flush == Z_FINISH) && ret == Z_OK) ret = Z_BUF_ERROR;
    return ret;
}

static uint8_t *read_file(const char *path, size_t *n, size_t extra) {
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    *n = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *b = malloc(*n + extra + 1);
    if (!b || fread(b, 1, *n, f) != *n) return NULL;
    fclose(f);
    return b;
}

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    rocm_remember_cpu_tier(cpu_adler, cpu_crc);
    const int wrap = atoi(argv[1]);
    const size_t out_chunk = (size_t)atol(argv[2]);
    size_t n = 0, tail_n = 0;
    uint8_t *tail = argc > 6 ? read_file(argv[6], &tail_n, 0) : NULL;
    if (argc > 6 && !tail) return 2;
    uint8_t *in = read_file(argv[3], &n, tail_n);
    if (!in) return 2;
    if (tail_n) memcpy(in + n, tail, tail_n);
    n += tail_n;
    FILE *fc = fopen(argv[4], "r");
    if (!fc) return 2;
    size_t ncuts = 0, cuts_cap = 1024;
    size_t *cuts = malloc(cuts_cap * sizeof *cuts);
    unsigned long long v;
    while (fscanf(fc, "%llu", &v) == 1) {
        if (ncuts == cuts_cap) cuts = realloc(cuts, (cuts_cap *= 2) * sizeof *cuts);
        if ((size_t)v > n || (ncuts && (size_t)v < cuts[ncuts - 1])) return 2;
        cuts[ncuts++] = (size_t)v;
    }
    fclose(fc);
    if (!ncuts || cuts[ncuts - 1] != n) {
        if (ncuts == cuts_cap) cuts = realloc(cuts, (cuts_cap + 1) * sizeof *cuts);
        cuts[ncuts++] = n;
    }

    zng_stream strm;
    memset(&strm, 0, sizeof strm);
    struct inflate_state st;
    memset(&st, 0, sizeof st);
    st.strm = &strm;
    st.wrap = wrap ? 5 : 0;                                     /* inflate.h: bit 0 zlib, bit 2 validate the check value */
    st.wbits = 15;
    st.mode = (inflate_mode)D_HEAD;
    strm.state = (struct internal_state *)&st;
    size_t cap = out_chunk, produced = 0;
    uint8_t *out = malloc(cap);
    const char *passes_env = getenv("COARSE_STREAM_PASSES");
    int passes = passes_env ? atoi(passes_env) : 1;
    if (passes < 1) passes = 1;
    if (passes > 64) passes = 64;
    double seconds[64];
    int rc = Z_OK;
    for (int pass = 0; pass < passes; ++pass) {
        st.mode = (inflate_mode)D_HEAD;
        strm.total_in = strm.total_out = 0;
        strm.msg = NULL;
        produced = 0;
        INFLATE_RESET_KEEP_HOOK(&strm);
        strm.next_in = in;
        rc = Z_OK;
        struct timespec t0, t1;
        timespec_get(&t0, TIME_UTC);
        for (size_t c = 0; c < ncuts && rc != Z_STREAM_END; ++c) {
            strm.avail_in = (uint32_t)(cuts[c] - (size_t)(strm.next_in - in));        /* what is left of earlier pieces, and this one */
            for (;;) {
                if (produced + out_chunk > cap) {
                    cap = 2 * cap + out_chunk;
                    out = realloc(out, cap);
                    if (!out) return 3;
                }
                strm.next_out = out + produced;
                strm.avail_out = (uint32_t)out_chunk;
                const uint32_t in0 = strm.avail_in;
                rc = driver_inflate(&strm, Z_NO_FLUSH);
                if (rc == -100) {
                    printf("fallback\n");
                    return 0;
                }
                produced += out_chunk - strm.avail_out;
                if (rc == Z_DATA_ERROR || rc == Z_STREAM_END) break;
                if (rc < 0 && rc != Z_BUF_ERROR) return 4;
                if (strm.avail_out == out_chunk && strm.avail_in == in0) break;       /* no progress: wait for the next piece */
            }
            if (pass + 1 == passes) printf("piece %zu %zu %zu %d\n", cuts[c], produced, st.arch.in_cap, zng_rocm_inflate_large_last_parts());
            if (rc == Z_DATA_ERROR) break;
        }
        timespec_get(&t1, TIME_UTC);
        seconds[pass] = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    }
    for (int pass = 0; passes > 1 && pass < passes; ++pass) printf("seconds %.6f\n", seconds[pass]);
    FILE *fo = fopen(argv[5], "wb");
    if (!fo || (produced && fwrite(out, 1, produced, fo) != produced)) return 9;
    fclose(fo);
    if (strm.total_out != produced) return 6;
    if (rc == Z_DATA_ERROR) printf("data error: %s\n", strm.msg ? strm.msg : "?");
    else if (rc == Z_STREAM_END) printf("end %zu %u %zu\n", (size_t)strm.total_in, strm.avail_in, produced);
    else printf("incomplete %zu %zu\n", (size_t)strm.total_in, produced);
    printf("parts %d\n", zng_rocm_inflate_large_last_parts());
    INFLATE_END_HOOK(&strm);
    return 0;
}
