/* abi_compress_streams2.c -- a strict C11 consumer of zng_rocm_compress_streams2_dev / zng_rocm_compress_members_dev of
 * include/zng_rocm.h, run WITHOUT zng_rocm_init (tests/test_abi_compress_streams2.py): both calls return ZNG_ROCM_ENODEV and
 * write nothing, a refused argument is refused before the device is asked for, no jobs is no work, and the bound is
 * zng_rocm_compress_bound. */
#include <stdio.h>
#include <string.h>

#include "zng_rocm.h"

int main(void) {
    static uint8_t in[64], out[4096];
    uint32_t results[2] = {41u, 42u}, checks[1] = {43u};
    uint64_t offsets[2] = {44u, 45u};
    zng_rocm_stream_job j;
    int fmt;
    memset(&j, 0, sizeof j);
    j.in = in;
    j.in_len = sizeof in;
    j.out = out;
    j.out_cap = sizeof out;
    for (fmt = 0; fmt <= 2; ++fmt) {
        if (zng_rocm_compress_streams2_bound(1000, fmt) != zng_rocm_compress_bound(1000, fmt)) return 1;
        if (zng_rocm_compress_streams2_bound(sizeof in, fmt) > sizeof out) return 2;
        if (zng_rocm_compress_streams2_dev(fmt, 6, 0, &j, 1, 0, results, NULL) != ZNG_ROCM_ENODEV) return 3;
        if (zng_rocm_compress_members_dev(fmt, -1, 3, &j, 1, out, sizeof out, 0, offsets, checks, NULL) != ZNG_ROCM_ENODEV) return 4;
        if (zng_rocm_compress_members_dev(fmt, 0, 0, &j, 1, NULL, 0, 1, offsets, NULL, NULL) != ZNG_ROCM_ENODEV) return 5;
    }
    if (zng_rocm_compress_streams2_dev(3, 6, 0, &j, 1, 0, results, NULL) != ZNG_ROCM_EINVAL) return 6;
    if (zng_rocm_compress_streams2_dev(2, 10, 0, &j, 1, 0, results, NULL) != ZNG_ROCM_EINVAL) return 7;
    if (zng_rocm_compress_members_dev(2, 6, 5, &j, 1, out, sizeof out, 0, offsets, checks, NULL) != ZNG_ROCM_EINVAL) return 8;
    j.out_cap = (uint32_t)zng_rocm_compress_streams2_bound(sizeof in, 2) - 1u;
    if (zng_rocm_compress_streams2_dev(2, 6, 0, &j, 1, 0, results, NULL) != -5) return 9;
    if (zng_rocm_compress_streams2_dev(2, 6, 0, NULL, 0, 0, NULL, NULL) != ZNG_ROCM_OK) return 10;
    if (zng_rocm_compress_members_dev(2, 6, 0, NULL, 0, NULL, 0, 0, NULL, NULL, NULL) != ZNG_ROCM_OK) return 11;
    if (zng_rocm_compress_streams2_last_rounds() != 0) return 12;
    if (results[0] != 41u || results[1] != 42u || checks[0] != 43u || offsets[0] != 44u || offsets[1] != 45u) return 13;
    for (fmt = 0; fmt < (int)sizeof out; ++fmt)
        if (out[fmt]) return 14;
    puts("ok nodev");
    return 0;
}
