/* A C11 consumer of the batch inflate entry point: include/zng_rocm.h with the job struct compiles under -std=c11 -pedantic
 * -Werror, the struct has the documented members in the documented order, and a process that never called
 * zng_rocm_init() gets ZNG_ROCM_ENODEV with every output field of every job left as it was. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "zng_rocm.h"

_Static_assert(offsetof(zng_rocm_inflate_large_job, d_src) == 0, "d_src first");
_Static_assert(offsetof(zng_rocm_inflate_large_job, src_len) < offsetof(zng_rocm_inflate_large_job, d_window), "order");
_Static_assert(offsetof(zng_rocm_inflate_large_job, window_len) < offsetof(zng_rocm_inflate_large_job, d_dst), "order");
_Static_assert(offsetof(zng_rocm_inflate_large_job, dst_cap) < offsetof(zng_rocm_inflate_large_job, status), "order");
_Static_assert(offsetof(zng_rocm_inflate_large_job, status) < offsetof(zng_rocm_inflate_large_job, out_len), "order");
_Static_assert(offsetof(zng_rocm_inflate_large_job, out_len) < offsetof(zng_rocm_inflate_large_job, in_used), "order");
_Static_assert(offsetof(zng_rocm_inflate_large_job, in_used) < offsetof(zng_rocm_inflate_large_job, msg), "order");
_Static_assert(offsetof(zng_rocm_inflate_large_job, msg) < offsetof(zng_rocm_inflate_large_job, parts), "order");
_Static_assert(offsetof(zng_rocm_inflate_large_job, parts) < offsetof(zng_rocm_inflate_large_job, subparts), "order");
_Static_assert(sizeof(((zng_rocm_inflate_large_job *)0)->out_len) == 8 && sizeof(((zng_rocm_inflate_large_job *)0)->parts) == 4,
               "widths");

/* the declared signatures, as function pointer types */
static int (*const p_call)(zng_rocm_inflate_large_job *, size_t, size_t, uint32_t, void *) = zng_rocm_inflate_large_streams_dev;
static int (*const p_rounds)(void) = zng_rocm_inflate_large_last_rounds;
static int (*const p_launches)(void) = zng_rocm_inflate_large_last_part_launches;

int main(void) {
    static const char text[] = "untouched";
    static uint8_t src[64], dst[64];
    zng_rocm_inflate_large_job jobs[3];
    memset(jobs, 0, sizeof jobs);
    for (int i = 0; i < 3; ++i) {
        /* (host addresses: without a device nothing may look at them) */
        jobs[i].d_src = src;
        jobs[i].src_len = sizeof src;
        jobs[i].d_dst = dst;
        jobs[i].dst_cap = sizeof dst;
        jobs[i].status = 70 + i;
        jobs[i].out_len = 0x1122334455667788ull;
        jobs[i].in_used = 99;
        jobs[i].msg = text;
        jobs[i].parts = 5;
        jobs[i].subparts = 6;
    }
    const int rc = p_call(jobs, 3, 0, ZNG_ROCM_INFLATE_SUBBLOCK, NULL);
    if (rc != ZNG_ROCM_ENODEV) {
        fprintf(stderr, "expected ZNG_ROCM_ENODEV before zng_rocm_init(), got %d\n", rc);
        return 1;
    }
    for (int i = 0; i < 3; ++i) {
        if (jobs[i].status != 70 + i || jobs[i].out_len != 0x1122334455667788ull || jobs[i].in_used != 99 || jobs[i].msg != text ||
            jobs[i].parts != 5 || jobs[i].subparts != 6) {
            fprintf(stderr, "job %d: output fields written without a device\n", i);
            return 1;
        }
    }
    for (size_t k = 0; k < sizeof dst; ++k)
        if (dst[k]) return 1;
    if (p_rounds() != 0 || p_launches() != 0) return 1;
    if (p_call(NULL, 0, 0, 0, NULL) != ZNG_ROCM_ENODEV) return 1;
    puts("ok nodev");
    return 0;
}
