/* tests/c/coarse_copy_driver.c -- TEST: deflateCopy() / inflateCopy() over streams that integration/arch/rocm/rocm_deflate.c and
 * rocm_inflate.c hold, two or three streams alive at once.  As in coarse_driver.c only the control flow around the hook macros
 * is restated (deflate.c:826-846 pending bytes, :868-886 zlib header, :1036-1083 DEFLATE_HOOK, :1091-1100 trailer,
 * :1131-1181 deflateCopy; inflate.c:509-555 zlib header, :728 INFLATE_TYPEDO_HOOK, :1105-1147 CHECK, :1379-1413 inflateCopy),
 * with the pending / header state per stream.  The copy functions: the stream memcpy, a fresh state block from the stream's
 * zalloc, the state memcpy, then DEFLATE_COPY_HOOK / INFLATE_COPY_HOOK; a hook that fails is followed by ...End(dest).
 * Every stream allocates through a counting zalloc / zfree: what is still allocated at the end is reported ("live"), and
 * COPY_DRIVER_FAIL_ALLOC=<k> makes the k-th allocation inside a copy fail.  The source's arch block is compared byte for byte
 * across every copy.  There is no software deflate / inflate here: a stream the hooks do not take reports "fallback".
 *
 *   coarse_copy_driver d <level> <wrap> <w_bits> <strategy> <point> <order> <P> <A> <B> <out_src> <out_copy>
 *        P is fed, the stream is copied at <point>, then the source gets tail A and the copy tail B, both with Z_FINISH
 *        point  first   before the first deflate(): P goes to both afterwards
 *               gather  300000 bytes in with Z_NO_FLUSH: they wait in in_buf, nothing has been produced
 *               sync    behind a Z_SYNC_FLUSH of all of P, everything delivered
 *               drain   inside that Z_SYNC_FLUSH: one call with avail_out 1000, out_buf holds bytes both still owe
 *               finish  P and A with Z_FINISH, one call with avail_out 1000: both streams only drain afterwards (no B)
 *               copy2   as sync, and the copy is copied again: the first copy ends at once, the second gets B
 *        order  0: the source finishes and ends before the copy continues; 1: the copy first
 *   coarse_copy_driver i <wrap> <wbits> <at> <last_avail_out> <order> <in_chunk> <file> <alt> <out_src> <out_copy> <plain bytes>
 *        the first <at> bytes of <file> are fed in calls of <in_chunk> bytes (the last of them with avail_out =
 *        <last_avail_out> when that is not 0), the stream is copied, the source gets the rest of <file> and the copy the
 *        rest of <alt> (a file of the same length; "-" = <file>)
 * prints
 *   copy in_len=<n> owed=<n> carry_bit=<n> hook=<0|1> [parts=<n>]     the source's arch block at the (first) copy
 *   copy failed <code>                                                the hook's value, after ...End(dest)
 *   src|copy device <bytes in> <bytes out> after <bytes written behind the copy point>
 *   src|copy data error: <msg>
 *   src|copy fallback <bytes in> <bytes out>                           where the reference would go on in software; what the
 *                                                                     stream wrote until then is in its output file
 *   live <allocations not released>                                   always 0 unless something leaked */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zng_rocm.h"
#include "zlibng_coarse_min.h"
#include "rocm_functions.h"
#include "rocm_deflate.h"
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

/* ---- the streams' allocator -------------------------------------------------------------------------------- */
static long live, fail_at, in_copy, copy_allocs;

static void *count_alloc(void *opaque, unsigned items, unsigned size) {
    (void)opaque;
    if (in_copy && ++copy_allocs == fail_at) return NULL;
    void *p = malloc((size_t)items * size);
    if (p) ++live;
    return p;
}
static void count_free(void *opaque, void *p) {
    (void)opaque;
    if (p) --live;
    free(p);
}

typedef struct {
    uint8_t *data;
    size_t   len, cap;
} obuf;

static int obuf_room(obuf *o, size_t more) {
    if (o->len + more <= o->cap) return 1;
    const size_t cap = (o->len + more) * 2;
    uint8_t *n = realloc(o->data, cap);
    if (!n) return 0;
    o->data = n;
    o->cap = cap;
    return 1;
}
static int obuf_copy(obuf *d, const obuf *s) {
    d->data = NULL;
    d->len = d->cap = 0;
    if (!obuf_room(d, s->len + 1)) return 0;
    if (s->len) memcpy(d->data, s->data, s->len);
    d->len = s->len;
    return 1;
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
static int write_file(const char *path, const obuf *o) {
    FILE *fo = fopen(path, "wb");
    if (!fo || fwrite(o->data, 1, o->len, fo) != o->len) return 0;
    return fclose(fo) == 0;
}

/* ---- deflate() around DEFLATE_HOOK, state per stream ------------------------------------------------------- */
typedef struct {
    zng_stream strm;
    uint8_t  pend[32];                                          /* s->pending_buf, as far as the driver needs one */
    unsigned npend, header_done, finish_state;
    obuf     out;
    size_t   mark;                                              /* total_out at the copy point */
    int      fallback, ended;
} dstream;

static void flush_pending(dstream *d) {                         /* deflate.c:786-812 */
    zng_stream *strm = &d->strm;
    unsigned n = d->npend < strm->avail_out ? d->npend : strm->avail_out;
    memcpy(strm->next_out, d->pend, n);
    memmove(d->pend, d->pend + n, d->npend - n);
    d->npend -= n;
    strm->next_out += n;
    strm->avail_out -= n;
    strm->total_out += n;
}

static int driver_deflate(dstream *d, int flush) {
    zng_stream *strm = &d->strm;
    deflate_state *s = strm->state;
    if (!d->header_done && s->wrap == 1) {                      /* deflate.c:868-886: CINFO from s->w_bits */
        unsigned header = (8u + ((s->w_bits - 8u) << 4)) << 8;
        const unsigned level_flags = (s->strategy >= ROCM_Z_HUFFMAN_ONLY || s->level < 2) ? 0u : s->level < 6 ? 1u : s->level == 6 ? 2u : 3u;
        header |= level_flags << 6;
        header += 31u - header % 31u;
        d->pend[d->npend++] = (uint8_t)(header >> 8);
        d->pend[d->npend++] = (uint8_t)header;
        strm->adler = 1;
    }
    d->header_done = 1;
    if (d->npend) {                                             /* deflate.c:826-846 */
        flush_pending(d);
        if (strm->avail_out == 0) return Z_OK;
    }
    if (strm->avail_in != 0 || (flush != Z_NO_FLUSH && !d->finish_state)) {    /* deflate.c:1036 */
        block_state bstate;
        if (!DEFLATE_HOOK(strm, flush, &bstate)) return -100;   /* the reference would call deflate_* here */
        if (bstate == finish_started || bstate == finish_done) d->finish_state = 1;
        if (bstate == need_more || bstate == finish_started) return Z_OK;
        if (bstate == block_done) {
            if (flush != Z_PARTIAL_FLUSH && flush != Z_BLOCK) { /* zng_tr_stored_block(s, NULL, 0, 0) with bi_valid == 0 */
                static const uint8_t marker[5] = {0x00, 0x00, 0x00, 0xff, 0xff};
                memcpy(d->pend + d->npend, marker, 5);
                d->npend += 5;
            }
            flush_pending(d);
            if (strm->avail_out == 0) return Z_OK;
        }
    }
    if (flush != Z_FINISH) return Z_OK;
    if (s->wrap == 1) {                                         /* deflate.c:1091-1100 */
        d->pend[d->npend++] = (uint8_t)(strm->adler >> 24);
        d->pend[d->npend++] = (uint8_t)(strm->adler >> 16);
        d->pend[d->npend++] = (uint8_t)(strm->adler >> 8);
        d->pend[d->npend++] = (uint8_t)strm->adler;
        s->wrap = -1;
    }
    flush_pending(d);
    return d->npend ? Z_OK : Z_STREAM_END;
}

static void driver_deflate_end(dstream *d) {                    /* deflateEnd(): the END hook, then free_deflate() */
    if (d->ended) return;
    DEFLATE_END_HOOK(&d->strm);
    count_free(NULL, d->strm.state);
    d->strm.state = NULL;
    d->ended = 1;
}

/* deflateCopy(), deflate.c:1131-1181.  The hook stands behind the state memcpy and `ds->strm = dest` (:1150), once the copy
 * owns its own allocation record (:1152) -- deflateEnd(dest) releases through it -- and in front of every later failure
 * path (:1158-1161), so none of them can run the END hook on the source's pointers. */
static int driver_deflate_copy(dstream *dest, dstream *source) {
    deflate_state *ss = source->strm.state;
    memcpy(dest, source, sizeof *dest);                         /* the stream; with it the driver's pending bytes (:1164) */
    dest->fallback = 0;                                         /* the copy asks its hooks itself */
    in_copy = 1;
    deflate_state *ds = count_alloc(NULL, 1, sizeof *ds);       /* alloc_deflate(), :1143 */
    if (!ds) {
        in_copy = 0;
        dest->strm.state = NULL;
        dest->ended = 1;
        return Z_MEM_ERROR;
    }
    dest->strm.state = ds;
    memcpy(ds, ss, sizeof *ds);
    ds->strm = &dest->strm;
    const int rc = DEFLATE_COPY_HOOK(&dest->strm, &source->strm);
    in_copy = 0;
    if (rc != Z_OK) {
        driver_deflate_end(dest);
        return rc;
    }
    return obuf_copy(&dest->out, &source->out) ? Z_OK : -101;
}

/* deflate() until the input is used up and next_out has room left (the caller's loop); in == NULL: continue with what the
 * stream still holds.  once != 0: a single call with avail_out = once */
static int run_deflate(dstream *d, const uint8_t *in, size_t n, int flush, size_t once) {
    if (d->fallback) return 0;
    if (in) {
        d->strm.next_in = in;
        d->strm.avail_in = (uint32_t)n;
    }
    const size_t out_chunk = once ? once : 65536;
    for (;;) {
        if (!obuf_room(&d->out, out_chunk)) return 3;
        d->strm.next_out = d->out.data + d->out.len;
        d->strm.avail_out = (uint32_t)out_chunk;
        const int rc = driver_deflate(d, flush);
        d->out.len += out_chunk - d->strm.avail_out;
        if (rc == -100) {
            d->fallback = 1;
            return 0;
        }
        if (rc < 0) return 4;
        if (once || rc == Z_STREAM_END) return 0;
        if (d->strm.avail_out != 0) {
            if (flush == Z_FINISH) continue;
            if (d->strm.avail_in != 0) return 5;                /* deflate() must use all input or all output */
            return 0;
        }
    }
}

static void report_deflate(const char *who, const dstream *d, int finished) {
    if (d->fallback) printf("%s fallback %zu %zu\n", who, d->strm.total_in, d->strm.total_out);
    else if (finished) printf("%s device %zu %zu after %zu\n", who, d->strm.total_in, d->strm.total_out, d->strm.total_out - d->mark);
}

static int main_deflate(int argc, char **argv) {
    if (argc < 13) return 2;
    const char *point = argv[6];
    const int order = atoi(argv[7]);
    size_t np = 0, na = 0, nb = 0;
    uint8_t *P = read_file(argv[8], &np), *A = read_file(argv[9], &na), *B = read_file(argv[10], &nb);
    if (!P || !A || !B) return 2;

    dstream src, cpy, mid;
    memset(&src, 0, sizeof src);
    memset(&cpy, 0, sizeof cpy);
    memset(&mid, 0, sizeof mid);
    src.strm.zalloc = count_alloc;
    src.strm.zfree = count_free;
    deflate_state *st = count_alloc(NULL, 1, sizeof *st);
    if (!st) return 2;
    memset(st, 0, sizeof *st);
    st->strm = &src.strm;
    st->level = atoi(argv[2]);
    st->wrap = atoi(argv[3]);
    st->w_bits = (unsigned)atoi(argv[4]);
    st->strategy = atoi(argv[5]);
    src.strm.state = st;
    DEFLATE_RESET_KEEP_HOOK(&src.strm);

    /* up to the copy point */
    int rc = 0, both_get_p = 0, tails = 1;
    if (!strcmp(point, "first")) {
        both_get_p = 1;
    } else if (!strcmp(point, "gather")) {
        if (np <= 300000) return 2;
        rc = run_deflate(&src, P, 300000, Z_NO_FLUSH, 65536);
    } else if (!strcmp(point, "sync") || !strcmp(point, "copy2")) {
        rc = run_deflate(&src, P, np, Z_SYNC_FLUSH, 0);
    } else if (!strcmp(point, "drain")) {
        rc = run_deflate(&src, P, np, Z_SYNC_FLUSH, 1000);
    } else if (!strcmp(point, "finish")) {
        rc = run_deflate(&src, P, np, Z_NO_FLUSH, 0);
        if (!rc) rc = run_deflate(&src, A, na, Z_FINISH, 1000);
        tails = 0;
    } else {
        return 2;
    }
    if (rc) return 10 + rc;

    /* the copy: the source's arch block must come out of it as it went in */
    arch_deflate_state before;
    memcpy(&before, &st->arch, sizeof before);
    printf("copy in_len=%zu owed=%zu carry_bit=0 hook=%d\n", st->arch.in_len, st->arch.out_len - st->arch.out_pos, st->arch.hook != NULL);
    dstream *last = &cpy;
    if (!strcmp(point, "copy2")) {
        rc = driver_deflate_copy(&mid, &src);
        if (rc == Z_OK) {
            rc = driver_deflate_copy(&cpy, &mid);
            driver_deflate_end(&mid);                           /* the one in the middle leaves first */
            free(mid.out.data);
        }
    } else {
        rc = driver_deflate_copy(&cpy, &src);
    }
    if (memcmp(&before, &st->arch, sizeof before)) return 20;
    if (rc != Z_OK) {
        printf("copy failed %d\n", rc);
        last = NULL;
    }
    src.mark = src.strm.total_out;
    cpy.mark = src.mark;

    /* behind it: each stream its own way, in the order asked for */
    for (int turn = 0; turn < 2; ++turn) {
        dstream *d = (turn == order) ? &src : last;
        if (!d) continue;
        const int is_src = d == &src;
        rc = 0;
        if (both_get_p) rc = run_deflate(d, P, np, Z_NO_FLUSH, 0);
        else if (!strcmp(point, "gather")) rc = run_deflate(d, P + 300000, np - 300000, Z_NO_FLUSH, 0);
        else if (!strcmp(point, "drain")) rc = run_deflate(d, NULL, 0, Z_SYNC_FLUSH, 0);
        if (!rc) rc = tails ? run_deflate(d, is_src ? A : B, is_src ? na : nb, Z_FINISH, 0) : run_deflate(d, NULL, 0, Z_FINISH, 0);
        if (rc) return 30 + rc;
        if (d->strm.total_out != d->out.len) return 6;
        if (!d->fallback) {
            const size_t want = tails ? np + (is_src ? na : nb) : np + na;
            if (d->strm.total_in != want) return 6;
            if (!DEFLATE_DONE(&d->strm, Z_FINISH)) return 7;
        }
        if (!write_file(is_src ? argv[11] : argv[12], &d->out)) return 9;
        report_deflate(is_src ? "src" : "copy", d, 1);
        driver_deflate_end(d);
        free(d->out.data);
    }
    printf("live %ld\n", live);
    free(P);
    free(A);
    free(B);
    return live ? 8 : 0;
}

/* ---- inflate() around INFLATE_TYPEDO_HOOK ----------------------------------------------------------------- */
#define RESTORE() do { } while (0)
#define LOAD() do { } while (0)
enum { D_HEAD = 1 };

typedef struct {
    zng_stream strm;
    obuf   out;
    size_t mark;
    int    fallback, ended, status;                             /* status: Z_STREAM_END or Z_DATA_ERROR once reached */
} istream;

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

static void driver_inflate_end(istream *s) {                    /* inflateEnd(): the END hook, then free_inflate() */
    if (s->ended) return;
    INFLATE_END_HOOK(&s->strm);
    count_free(NULL, s->strm.state);
    s->strm.state = NULL;
    s->ended = 1;
}

/* inflateCopy(), inflate.c:1379-1413.  The hook stands behind the state memcpy and `copy->strm = dest` (:1399), once the copy
 * owns its own allocation record (:1406) and dest->state points at it (:1411, moved up): inflateEnd(dest) needs both. */
static int driver_inflate_copy(istream *dest, istream *source) {
    struct inflate_state *state = (struct inflate_state *)source->strm.state;
    memcpy(dest, source, sizeof *dest);
    dest->fallback = 0;                                         /* the copy asks its hooks itself */
    in_copy = 1;
    struct inflate_state *copy = count_alloc(NULL, 1, sizeof *copy);     /* alloc_inflate(), :1392 */
    if (!copy) {
        in_copy = 0;
        dest->strm.state = NULL;
        dest->ended = 1;
        return Z_MEM_ERROR;
    }
    memcpy(copy, state, sizeof *copy);
    copy->strm = &dest->strm;
    dest->strm.state = (struct internal_state *)copy;
    const int rc = INFLATE_COPY_HOOK(&dest->strm, &source->strm);
    in_copy = 0;
    if (rc != Z_OK) {
        driver_inflate_end(dest);
        return rc;
    }
    return obuf_copy(&dest->out, &source->out) ? Z_OK : -101;
}

/* inflate() over in[from, to) in calls of in_chunk bytes; last_out != 0: the call that brings the last piece has that much
 * room and is the only one for it */
static int run_inflate(istream *s, const uint8_t *in, size_t from, size_t to, size_t in_chunk, size_t last_out, size_t plain) {
    size_t fed = from;
    const size_t out_chunk = 1u << 20;
    if (s->fallback || s->status) return 0;
    for (;;) {
        int last_piece = 0;
        if (s->strm.avail_in == 0 && fed < to) {
            const size_t c = to - fed < in_chunk ? to - fed : in_chunk;
            s->strm.next_in = in + fed;
            s->strm.avail_in = (uint32_t)c;
            fed += c;
            last_piece = fed == to;
        }
        const size_t room = (last_piece && last_out) ? last_out : out_chunk;
        if (s->out.len + room > plain + out_chunk + room) return 3;         /* more plaintext than there can be */
        if (!obuf_room(&s->out, room)) return 3;
        s->strm.next_out = s->out.data + s->out.len;
        s->strm.avail_out = (uint32_t)room;
        const int rc = driver_inflate(&s->strm, Z_NO_FLUSH);
        if (rc == -100) {
            s->fallback = 1;
            return 0;
        }
        s->out.len += room - s->strm.avail_out;
        if (rc == Z_STREAM_END || rc == Z_DATA_ERROR) {
            s->status = rc;
            return 0;
        }
        if (rc < 0 && rc != Z_BUF_ERROR) return 4;
        if (last_piece && last_out) return 0;
        if (fed == to && s->strm.avail_in == 0 && s->strm.avail_out != 0) return 0;    /* everything given is used and delivered */
        if (rc == Z_BUF_ERROR && s->strm.avail_out == room) return 8;                   /* stuck */
    }
}

static void report_inflate(const char *who, const istream *s) {
    if (s->fallback) printf("%s fallback %zu %zu\n", who, s->strm.total_in, s->strm.total_out);
    else if (s->status == Z_STREAM_END) printf("%s device %zu %zu after %zu\n", who, s->strm.total_in, s->strm.total_out, s->strm.total_out - s->mark);
    else if (s->status == Z_DATA_ERROR) printf("%s data error: %s\n", who, s->strm.msg ? s->strm.msg : "?");
    else printf("%s unfinished %zu %zu\n", who, s->strm.total_in, s->strm.total_out);
}

static int main_inflate(int argc, char **argv) {
    if (argc < 13) return 2;
    const size_t at = (size_t)atol(argv[4]), last_out = (size_t)atol(argv[5]);
    const int order = atoi(argv[6]);
    const size_t in_chunk = (size_t)atol(argv[7]), plain = (size_t)atol(argv[12]);
    size_t n = 0, nalt = 0;
    uint8_t *in = read_file(argv[8], &n);
    uint8_t *alt = strcmp(argv[9], "-") ? read_file(argv[9], &nalt) : in;
    if (!in || !alt || !in_chunk || at > n || (alt != in && nalt != n)) return 2;

    istream src, cpy;
    memset(&src, 0, sizeof src);
    memset(&cpy, 0, sizeof cpy);
    src.strm.zalloc = count_alloc;
    src.strm.zfree = count_free;
    struct inflate_state *st = count_alloc(NULL, 1, sizeof *st);
    if (!st) return 2;
    memset(st, 0, sizeof *st);
    st->strm = &src.strm;
    st->wrap = atoi(argv[2]) ? 5 : 0;                           /* inflate.h: bit 0 zlib, bit 2 validate the check value */
    st->wbits = (unsigned)atoi(argv[3]);
    st->mode = (inflate_mode)D_HEAD;
    src.strm.state = (struct internal_state *)st;
    INFLATE_RESET_KEEP_HOOK(&src.strm);

    int rc = at ? run_inflate(&src, in, 0, at, in_chunk, last_out, plain) : 0;
    if (rc) return 10 + rc;

    arch_inflate_state before;
    memcpy(&before, &st->arch, sizeof before);
    printf("copy in_len=%zu owed=%zu carry_bit=%u hook=%d", st->arch.in_len, st->arch.out_len - st->arch.out_pos, st->arch.carry_bit,
           st->arch.hook != NULL);
    if (getenv("COARSE_DRIVER_PARTS")) printf(" parts=%d", zng_rocm_inflate_large_last_parts());
    printf("\n");
    istream *other = &cpy;
    rc = driver_inflate_copy(&cpy, &src);
    if (memcmp(&before, &st->arch, sizeof before)) return 20;
    if (rc != Z_OK) {
        printf("copy failed %d\n", rc);
        other = NULL;
    }
    src.mark = cpy.mark = src.strm.total_out;

    for (int turn = 0; turn < 2; ++turn) {
        istream *s = (turn == order) ? &src : other;
        if (!s) continue;
        const int is_src = s == &src;
        rc = run_inflate(s, is_src ? in : alt, at, n, in_chunk, 0, plain);
        if (rc) return 30 + rc;
        if (s->strm.total_out != s->out.len) return 6;
        if (!write_file(is_src ? argv[10] : argv[11], &s->out)) return 9;
        report_inflate(is_src ? "src" : "copy", s);
        driver_inflate_end(s);
        free(s->out.data);
    }
    printf("live %ld\n", live);
    if (alt != in) free(alt);
    free(in);
    return live ? 8 : 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    rocm_remember_cpu_tier(cpu_adler, cpu_crc);
    const char *fa = getenv("COPY_DRIVER_FAIL_ALLOC");
    fail_at = fa ? atol(fa) : 0;
    return argv[1][0] == 'd' ? main_deflate(argc, argv) : argv[1][0] == 'i' ? main_inflate(argc, argv) : 2;
}
