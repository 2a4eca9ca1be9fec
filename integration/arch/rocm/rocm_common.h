/* arch/rocm/rocm_common.h -- extension blocks of deflate_state / inflate_state for the arch/rocm backend
 * (deflate.h:319-321 `arch_deflate_state arch`, inflate.h:160-162; precedent arch/s390/dfltcc_common.h:66-84).
 * The device side of both (history in HBM, staging, HIP stream) is one opaque zng_rocm_hook of libzng_rocm. */
#ifndef ROCM_COMMON_H_
#define ROCM_COMMON_H_
#include <stddef.h>
#include <stdint.h>
#include "zng_rocm.h"

#ifndef ROCM_DEFLATE_BLOCK_BYTES
#  define ROCM_DEFLATE_BLOCK_BYTES (8u << 20)   /* input gathered per device block when the caller does not flush */
#endif

typedef struct {
    zng_rocm_hook *hook;        /* created at the first deflate() the device takes; NULL = not tried yet */
    uint8_t *in_buf;            /* input gathered until it is worth a launch (deflate() may be called with a few bytes) */
    size_t   in_len, in_cap;
    uint8_t *out_buf;           /* compressed bytes next_out has not had room for yet */
    size_t   out_pos, out_len, out_cap;
    int      used;              /* the device has produced part of this stream */
    int      finished;          /* the BFINAL block has been produced */
    int      disabled;          /* no device, or it failed: software from here on */
} arch_deflate_state;

typedef struct {
    zng_rocm_hook *hook;
    uint8_t *in_buf;            /* the carry: compressed bytes from the start of the first incomplete block on */
    size_t   in_len, in_cap;
    unsigned carry_bit;         /* bit of in_buf[0] at which that block starts (0..7) */
    const uint8_t *out;         /* plaintext (memory of the hook, or out_own) next_out has not had room for yet */
    size_t   out_pos, out_len;
    uint8_t *out_own;           /* set by inflateCopy only: the source's undelivered plaintext, copied out of ITS hook's memory */
    uint32_t check;             /* check value of the plaintext so far, handed to state->check once the stream is delivered */
    const char *msg;            /* bad: the reference's text, reported once the blocks in front of the error are delivered */
    int      used, done, bad, disabled;
} arch_inflate_state;
#endif
