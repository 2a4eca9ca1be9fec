/* abi_compress_streams2_dict.c -- a strict C11 consumer of zng_rocm_compress_streams2_dict_bound / zng_rocm_compress_streams2_dict_dev
 * / zng_rocm_compress_members_dict_dev of include/zng_rocm.h, run WITHOUT zng_rocm_init (tests/test_abi_compress_streams2_dict.py):
 * a refused argument is refused before the device is asked for, then both calls return ZNG_ROCM_ENODEV (the dictionary object
 * is not looked into before that: none can exist without a device) and write nothing; no jobs is no work. */
#include <stdio.h>
#include <string.h>

#include "zng_rocm.h"

int main(void) {
    static uint8_t in[64], out[4096];
    static uint64_t not_an_object[8];
    const zng_rocm_dict *dict = (const zng_rocm_dict *)(const void *)not_an_object;
    uint32_t results[2] = {41u, 42u}, checks[1] = {43u};
    uint64_t offsets[2] = {44u, 45u};
    zng_rocm_stream_job j;
    int fmt, i;
    memset(&j, 0, sizeof j);
    j.in = in;
    j.in_len = sizeof in;
    j.out = out;
    j.out_cap = sizeof out;
    if (zng_rocm_compress_streams2_dict_bound(1000, 0) != zng_rocm_compress_streams2_bound(1000, 0)) return 1;
    if (zng_rocm_compress_streams2_dict_bound(1000, 1) != zng_rocm_compress_streams2_bound(1000, 1) + 4) return 2;
    if (zng_rocm_compress_streams2_dict_bound(1000, 2) != 0 || zng_rocm_compress_streams2_dict_bound(1000, -1) != 0) return 3;
    /* the refusals come first */
    if (zng_rocm_compress_streams2_dict_dev(2, 6, 0, dict, &j, 1, 0, results, NULL) != ZNG_ROCM_EINVAL) return 4;
    if (zng_rocm_compress_members_dict_dev(2, 6, 0, dict, &j, 1, out, sizeof out, 0, offsets, checks, NULL) != ZNG_ROCM_EINVAL) return 5;
    if (zng_rocm_compress_streams2_dict_dev(1, 6, 0, NULL, &j, 1, 0, results, NULL) != ZNG_ROCM_EINVAL) return 6;
    if (zng_rocm_compress_members_dict_dev(0, 6, 0, NULL, &j, 1, out, sizeof out, 0, offsets, checks, NULL) != ZNG_ROCM_EINVAL) return 7;
    if (zng_rocm_compress_streams2_dict_dev(1, 6, 2, dict, &j, 1, 0, results, NULL) != ZNG_ROCM_EINVAL) return 8;
    if (zng_rocm_compress_members_dict_dev(0, 6, 3, dict, &j, 1, out, sizeof out, 0, offsets, checks, NULL) != ZNG_ROCM_EINVAL) return 9;
    if (zng_rocm_compress_streams2_dict_dev(1, 10, 0, dict, &j, 1, 0, results, NULL) != ZNG_ROCM_EINVAL) return 10;
    if (zng_rocm_compress_streams2_dict_dev(1, 6, 0, dict, &j, 1, 0, NULL, NULL) != ZNG_ROCM_EINVAL) return 11;
    j.dict_len = 16;
    if (zng_rocm_compress_streams2_dict_dev(0, 6, 0, dict, &j, 1, 0, results, NULL) != ZNG_ROCM_EINVAL) return 12;
    j.dict_len = 0;
    j.flags = ZNG_ROCM_BLOCK_NOT_FINAL;
    if (zng_rocm_compress_streams2_dict_dev(1, 6, 0, dict, &j, 1, 0, results, NULL) != ZNG_ROCM_EINVAL) return 13;
    j.flags = 0;
    j.out_cap = (uint32_t)zng_rocm_compress_streams2_dict_bound(sizeof in, 1) - 1u;
    if (zng_rocm_compress_streams2_dict_dev(1, 6, 0, dict, &j, 1, 0, results, NULL) != -5) return 14;
    j.out_cap = sizeof out;
    /* no jobs is no work; then the device */
    if (zng_rocm_compress_streams2_dict_dev(1, 6, 0, dict, NULL, 0, 0, NULL, NULL) != ZNG_ROCM_OK) return 15;
    if (zng_rocm_compress_members_dict_dev(1, 6, 0, dict, NULL, 0, NULL, 0, 0, NULL, NULL, NULL) != ZNG_ROCM_OK) return 16;
    for (fmt = 0; fmt <= 1; ++fmt) {
        if (zng_rocm_compress_streams2_dict_bound(sizeof in, fmt) > sizeof out) return 17;
        if (zng_rocm_compress_streams2_dict_dev(fmt, 6, 0, dict, &j, 1, 0, results, NULL) != ZNG_ROCM_ENODEV) return 18;
        if (zng_rocm_compress_members_dict_dev(fmt, -1, 4, dict, &j, 1, out, sizeof out, 0, offsets, checks, NULL) != ZNG_ROCM_ENODEV) return 19;
        if (zng_rocm_compress_members_dict_dev(fmt, 0, 1, dict, &j, 1, NULL, 0, 1, offsets, NULL, NULL) != ZNG_ROCM_ENODEV) return 20;
    }
    if (zng_rocm_compress_streams2_last_rounds() != 0) return 21;
    if (results[0] != 41u || results[1] != 42u || checks[0] != 43u || offsets[0] != 44u || offsets[1] != 45u) return 22;
    for (i = 0; i < (int)sizeof out; ++i)
        if (out[i]) return 23;
    puts("ok nodev");
    return 0;
}
