/* arch/rocm/rocm_inflate.c -- INFLATE_TYPEDO_HOOK backend of arch/rocm (inflate.c:728; precedent
 * arch/s390/dfltcc_inflate.c:52-114).  inflate() keeps the wrapper (zlib / gzip header and trailer, inflate.c:509-700,
 * :1105-1147) and the zng_stream bookkeeping; the deflate data between them is decoded by libzng_rocm (blocks found and
 * decoded in parts on the device from 4 MiB of input on, token decode on the host below that, every match copy on the
 * device) and its check value comes back with it (INFLATE_NEED_CHECKSUM = 0).
 * The unit of work is the COMPLETE block: a call that brings input decodes every block whose end lies inside the bytes it
 * has, delivers their plaintext, and keeps only the compressed bytes of the first incomplete block (from its start bit
 * on) for the next call -- so whatever a Z_SYNC_FLUSH put in front of its marker comes out as soon as the marker is in
 * (zlib-ng.h.in:285-288), and per call the work and the memory are one piece plus one incomplete block.  The call that
 * completes the BFINAL block consumes only the bytes up to its end: whatever lies behind it (the trailer, a next member)
 * stays in next_in.  Anything the device path cannot do leaves the stream to software BEFORE a byte is consumed. */
#ifdef ZNG_ROCM_STANDALONE_CHECK
#  include "zlibng_coarse_min.h"
#else
#  include "zbuild.h"
#  include "inflate.h"
#endif
#include <assert.h>
#include <stdlib.h>
#include <string.h>
#include "zng_rocm.h"
#include "rocm_functions.h"
#include "rocm_inflate.h"

#ifndef ROCM_INFLATE_MIN_BYTES
#  define ROCM_INFLATE_MIN_BYTES (1u << 20)     /* a first call with less input than this stays in software */
#endif

static void *arch_alloc(PREFIX3(streamp) strm, size_t n) {
    return strm->zalloc ? strm->zalloc(strm->opaque, 1, (unsigned)n) : malloc(n);
}
static void arch_free(PREFIX3(streamp) strm, void *p) {
    if (!p) return;
    if (strm->zfree) strm->zfree(strm->opaque, p);
    else free(p);
}

void Z_INTERNAL PREFIX(archrocm_reset_inflate_state)(PREFIX3(streamp) strm) {      /* INFLATE_RESET_KEEP_HOOK, inflate.c:87 */
    arch_inflate_state *a = &((struct inflate_state *)strm->state)->arch;
    a->in_len = a->out_pos = a->out_len = 0;
    a->carry_bit = 0;
    arch_free(strm, a->out_own);
    a->out = a->out_own = NULL;
    a->msg = NULL;
    a->used = a->done = a->bad = 0;
    if (a->hook && zng_rocm_hook_reset(a->hook) != ZNG_ROCM_OK) a->disabled = 1;
}

void Z_INTERNAL PREFIX(archrocm_inflate_end)(PREFIX3(streamp) strm) {              /* INFLATE_END_HOOK, in inflateEnd() */
    arch_inflate_state *a = &((struct inflate_state *)strm->state)->arch;
    zng_rocm_hook_destroy(a->hook);
    arch_free(strm, a->in_buf);
    arch_free(strm, a->out_own);
    memset(a, 0, sizeof *a);
}

/* INFLATE_COPY_HOOK, in inflateCopy() behind the memcpy of the state block (inflate.c:1398-1406): dest's arch block is
 * source's, pointer for pointer, and none of the pointers may stay (one hook, one carry, and `out` inside the SOURCE's
 * hook, which its next decode overwrites).  The carry is copied with dest's zalloc, the hook is cloned (history device to
 * device), and plaintext next_out has not had room for moves into out_own, memory dest owns until it is delivered.  A
 * stream whose history is on the device cannot continue without it, so unlike deflateCopy every failure is Z_MEM_ERROR,
 * with dest's block zeroed first: the inflateEnd(dest) that follows in inflateCopy finds nothing to release.  source is
 * only read. */
int Z_INTERNAL PREFIX(archrocm_inflate_copy)(PREFIX3(streamp) dest, PREFIX3(streamp) source) {
    const arch_inflate_state *sa = &((struct inflate_state *)source->state)->arch;
    arch_inflate_state *da = &((struct inflate_state *)dest->state)->arch;
    const size_t owed = sa->out_len - sa->out_pos;
    memset(da, 0, sizeof *da);
    if (sa->in_len) {
        if (!(da->in_buf = (uint8_t *)arch_alloc(dest, sa->in_len))) goto fail;
        memcpy(da->in_buf, sa->in_buf, sa->in_len);
        da->in_len = da->in_cap = sa->in_len;
    }
    da->carry_bit = sa->carry_bit;
    if (owed) {
        if (!(da->out_own = (uint8_t *)arch_alloc(dest, owed))) goto fail;
        memcpy(da->out_own, sa->out + sa->out_pos, owed);
        da->out = da->out_own;
        da->out_len = owed;
    }
    da->check = sa->check;
    da->msg = sa->msg;
    da->used = sa->used;
    da->done = sa->done;
    da->bad = sa->bad;
    da->disabled = sa->disabled;
    /* (a disabled stream never comes back to its hook, archrocm_can_inflate: it needs none) */
    if (sa->hook && !sa->disabled && zng_rocm_hook_clone(sa->hook, &da->hook) != ZNG_ROCM_OK) goto fail;
    return Z_OK;
fail:
    arch_free(dest, da->in_buf);
    arch_free(dest, da->out_own);
    memset(da, 0, sizeof *da);
    return Z_MEM_ERROR;
}

int Z_INTERNAL PREFIX(archrocm_can_inflate)(PREFIX3(streamp) strm) {
    struct inflate_state *state = (struct inflate_state *)strm->state;
    arch_inflate_state *a = &state->arch;
    if (a->disabled || state->wbits != 15) return 0;
    if (a->used) return 1;
    /* a stream begins here: whole bytes only (a block that starts inside a byte follows blocks software has decoded), and
     * enough input to be worth the launches */
    if (state->bits != 0 || strm->avail_in < ROCM_INFLATE_MIN_BYTES) return 0;
    if (!a->hook) {
        if (zng_rocm_device_count() <= 0 || zng_rocm_init(-1) != ZNG_ROCM_OK ||
            zng_rocm_hook_create(&a->hook, 1u << 20) != ZNG_ROCM_OK) {
            a->hook = NULL;
            a->disabled = 1;
            return 0;
        }
    }
    return 1;
}

int Z_INTERNAL PREFIX(archrocm_was_inflate_used)(PREFIX3(streamp) strm) {
    return ((struct inflate_state *)strm->state)->arch.used;
}

int Z_INTERNAL PREFIX(archrocm_inflate_disable)(PREFIX3(streamp) strm) {           /* inflatePrime: bit granular, software only */
    arch_inflate_state *a = &((struct inflate_state *)strm->state)->arch;
    if (a->used) return 1;                              /* too late: the caller gets Z_STREAM_ERROR */
    a->disabled = 1;
    return 0;
}

static void drain(PREFIX3(streamp) strm, arch_inflate_state *a) {
    size_t n = a->out_len - a->out_pos;
    if (n > strm->avail_out) n = strm->avail_out;
    if (n) {
        memcpy(strm->next_out, a->out + a->out_pos, n);
        strm->next_out += n;
        strm->avail_out -= (uint32_t)n;
        a->out_pos += n;                                /* total_out: inflate() adds what avail_out lost, inflate.c:1186-1188 */
    }
}

rocm_inflate_action Z_INTERNAL PREFIX(archrocm_inflate)(PREFIX3(streamp) strm, int flush, int *ret) {
    struct inflate_state *state = (struct inflate_state *)strm->state;
    arch_inflate_state *a = &state->arch;

    if (flush == Z_BLOCK || flush == Z_TREES) {         /* stopping at block boundaries: software only */
        if (a->used) {
            *ret = Z_STREAM_ERROR;
            return ROCM_INFLATE_BREAK;
        }
        a->disabled = 1;
        return ROCM_INFLATE_SOFTWARE;
    }
    drain(strm, a);                                     /* plaintext of earlier blocks first */
    if (a->out_pos < a->out_len) {                      /* next_out is full: no input is taken */
        *ret = Z_OK;
        return ROCM_INFLATE_BREAK;
    }
    if (a->done) {
        if (state->wrap & 4) strm->adler = state->check = a->check;
        state->last = 1;
        state->mode = CHECK;                            /* the trailer is inflate()'s, inflate.c:1105-1147 */
        return ROCM_INFLATE_CONTINUE;
    }
    if (a->bad) {                                       /* Z_DATA_ERROR with the reference's text (inflate_p.h:130-134) */
        strm->msg = a->msg;
        state->mode = BAD;
        return ROCM_INFLATE_CONTINUE;
    }
    if (strm->avail_in == 0 || strm->avail_out == 0) {  /* no input, or no room for what a decode would produce */
        *ret = Z_OK;                                    /* inflate() turns "no progress" into Z_BUF_ERROR itself */
        return ROCM_INFLATE_BREAK;
    }
    /* the carry and this call's input, one buffer; nothing is marked consumed until the decode says where blocks end */
    const size_t taken = strm->avail_in, total = a->in_len + taken;
    if (a->in_cap < total) {
        const size_t want = total * 2;
        uint8_t *n = (uint8_t *)arch_alloc(strm, want);
        if (!n) {
            if (a->used) { *ret = Z_MEM_ERROR; return ROCM_INFLATE_BREAK; }
            a->disabled = 1;
            return ROCM_INFLATE_SOFTWARE;
        }
        if (a->in_len) memcpy(n, a->in_buf, a->in_len);
        arch_free(strm, a->in_buf);
        a->in_buf = n;
        a->in_cap = want;
    }
    memcpy(a->in_buf + a->in_len, strm->next_in, taken);

    const int kind = !(state->wrap & 4) ? 0 : state->flags ? 2 : 1;             /* inflate_p.h:47-49: gzip -> crc32, zlib -> adler32 */
    uint32_t cv = a->used ? a->check : state->check;
    const uint8_t *out = NULL;
    size_t out_len = 0;
    uint64_t end_bit = 0;
    const char *msg = NULL;
    const int rc = zng_rocm_hook_inflate_blocks(a->hook, a->in_buf, total, a->carry_bit, kind, &cv, &out, &out_len, &end_bit, &msg);
    if (rc == 1 || rc == 0 || (rc == Z_DATA_ERROR && msg)) {     /* (-3 without a text: a refused argument) */
        arch_free(strm, a->out_own);                    /* (a copy's inherited plaintext: all delivered, or no input is taken) */
        a->out_own = NULL;
        a->out = out;
        a->out_pos = 0;
        a->out_len = out_len;
        a->check = cv;
        a->used = 1;
        if (rc == 1) {                                  /* Z_STREAM_END: the deflate data ends at end_bit */
            /* every earlier call decoded every block that was complete, so the last one ends among this call's bytes */
            const size_t upto = (size_t)((end_bit + 7) >> 3);
            assert(upto > a->in_len && upto <= total);
            const size_t mine = upto > a->in_len ? upto - a->in_len : 0;
            strm->next_in += mine;
            strm->avail_in -= (uint32_t)mine;
            a->in_len = 0;
            a->carry_bit = 0;
            a->done = 1;
        } else {                                        /* all of it is taken; the first incomplete block is carried */
            const size_t from = (size_t)(end_bit >> 3);
            strm->next_in += taken;
            strm->avail_in = 0;
            if (from) memmove(a->in_buf, a->in_buf + from, total - from);
            a->in_len = total - from;
            a->carry_bit = (unsigned)(end_bit & 7);
            if (rc == Z_DATA_ERROR) {                   /* the blocks in front of the bad one go out first */
                a->bad = 1;
                a->msg = msg;
            }
        }
        return PREFIX(archrocm_inflate)(strm, flush, ret);  /* deliver */
    }
    /* device trouble: nothing of this call has been consumed; a stream that never needed a second call goes to software */
    if (!a->used) {
        a->disabled = 1;
        return ROCM_INFLATE_SOFTWARE;
    }
    *ret = Z_MEM_ERROR;
    return ROCM_INFLATE_BREAK;
}

int Z_INTERNAL PREFIX(archrocm_inflate_set_dictionary)(PREFIX3(streamp) strm, const unsigned char *dictionary, unsigned dict_length) {
    struct inflate_state *state = (struct inflate_state *)strm->state;
    if (zng_rocm_hook_set_history(state->arch.hook, dictionary, dict_length) != ZNG_ROCM_OK) return Z_STREAM_ERROR;
    return Z_OK;
}

int Z_INTERNAL PREFIX(archrocm_inflate_get_dictionary)(PREFIX3(streamp) strm, unsigned char *dictionary, unsigned *dict_length) {
    struct inflate_state *state = (struct inflate_state *)strm->state;
    uint32_t len = 0;
    if (zng_rocm_hook_get_history(state->arch.hook, dictionary, &len) != ZNG_ROCM_OK) return Z_STREAM_ERROR;
    if (dict_length) *dict_length = len;
    return Z_OK;
}
