/* abi_inflate_large_size.c -- a strict C11 consumer of zng_rocm_uncompress_large_size_dev and
 * zng_rocm_uncompress_large_sizes_dev (include/zng_rocm.h), run WITHOUT zng_rocm_init (tests/test_abi_inflate_large_size.py):
 * every refusal the header lists answers ZNG_ROCM_EINVAL, a call the checks accept answers ZNG_ROCM_ENODEV, and neither
 * writes a job field or an out-parameter. */
#include <stdio.h>
#include <string.h>

#include "zng_rocm.h"

static zng_rocm_inflate_large_job fresh(const uint8_t *src, size_t n) {
    zng_rocm_inflate_large_job j;
    memset(&j, 0, sizeof j);
    j.d_src = src;
    j.src_len = n;
    j.status = 77;
    j.out_len = 78u;
    j.in_used = 79u;
    j.parts = 80u;
    j.subparts = 81u;
    return j;
}

static int untouched(const zng_rocm_inflate_large_job *j) {
    return j->status == 77 && j->out_len == 78u && j->in_used == 79u && j->msg == NULL && j->parts == 80u && j->subparts == 81u;
}

int main(void) {
    static uint8_t bytes[64], dict[16];
    uint64_t out_len = 41u;
    size_t in_used = 42u;
    zng_rocm_inflate_large_job j = fresh(bytes, sizeof bytes);
    /* accepted: the device is asked for, and is not there */
    for (int format = 0; format <= 2; ++format) {
        if (zng_rocm_uncompress_large_size_dev(format, bytes, sizeof bytes, NULL, 0, &out_len, &in_used, 0, NULL) != ZNG_ROCM_ENODEV) return 1;
        if (zng_rocm_uncompress_large_sizes_dev(format, &j, 1, 0, 0, NULL) != ZNG_ROCM_ENODEV) return 2;
    }
    /* format 0: only the LENGTH of the history matters -- a null pointer with a length is accepted; an empty input too */
    if (zng_rocm_uncompress_large_size_dev(0, bytes, sizeof bytes, NULL, 32768u, &out_len, &in_used, 0, NULL) != ZNG_ROCM_ENODEV) return 3;
    if (zng_rocm_uncompress_large_size_dev(0, NULL, 0, NULL, 0, &out_len, &in_used, 0, NULL) != ZNG_ROCM_ENODEV) return 4;
    if (zng_rocm_uncompress_large_size_dev(1, bytes, sizeof bytes, dict, sizeof dict, &out_len, &in_used, 0, NULL) != ZNG_ROCM_ENODEV) return 5;
    if (zng_rocm_uncompress_large_sizes_dev(0, &j, 1, (size_t)4 << 20, 0, NULL) != ZNG_ROCM_ENODEV) return 6;
    /* refusals: the format, the flags, the history length, a null source with a length, the round size, 2 GiB and more */
    if (zng_rocm_uncompress_large_size_dev(3, bytes, sizeof bytes, NULL, 0, &out_len, &in_used, 0, NULL) != ZNG_ROCM_EINVAL) return 10;
    if (zng_rocm_uncompress_large_size_dev(-1, bytes, sizeof bytes, NULL, 0, &out_len, &in_used, 0, NULL) != ZNG_ROCM_EINVAL) return 11;
    if (zng_rocm_uncompress_large_size_dev(0, bytes, sizeof bytes, NULL, 0, &out_len, &in_used, ZNG_ROCM_INFLATE_SUBBLOCK, NULL) !=
        ZNG_ROCM_EINVAL)
        return 12;
    if (strstr(zng_rocm_last_error(), "0x1") == NULL) return 13;
    if (zng_rocm_uncompress_large_size_dev(0, bytes, sizeof bytes, NULL, 0, &out_len, &in_used, 0x80u, NULL) != ZNG_ROCM_EINVAL) return 14;
    if (strstr(zng_rocm_last_error(), "0x80") == NULL) return 15;
    if (zng_rocm_uncompress_large_size_dev(0, bytes, sizeof bytes, dict, 32769u, &out_len, &in_used, 0, NULL) != ZNG_ROCM_EINVAL) return 16;
    if (zng_rocm_uncompress_large_size_dev(0, NULL, sizeof bytes, NULL, 0, &out_len, &in_used, 0, NULL) != ZNG_ROCM_EINVAL) return 17;
    if (zng_rocm_uncompress_large_size_dev(0, bytes, (size_t)1 << 31, NULL, 0, &out_len, &in_used, 0, NULL) != ZNG_ROCM_EINVAL) return 18;
    if (zng_rocm_uncompress_large_size_dev(0, bytes, sizeof bytes, NULL, 0, NULL, &in_used, 0, NULL) != ZNG_ROCM_EINVAL) return 19;
    if (zng_rocm_uncompress_large_size_dev(0, bytes, sizeof bytes, NULL, 0, &out_len, NULL, 0, NULL) != ZNG_ROCM_EINVAL) return 20;
    /* zlib needs the dictionary's bytes for the DICTID; gzip takes no dictionary */
    if (zng_rocm_uncompress_large_size_dev(1, bytes, sizeof bytes, NULL, 16u, &out_len, &in_used, 0, NULL) != ZNG_ROCM_EINVAL) return 21;
    if (zng_rocm_uncompress_large_size_dev(2, bytes, sizeof bytes, dict, sizeof dict, &out_len, &in_used, 0, NULL) != ZNG_ROCM_EINVAL) return 22;
    /* the batch */
    if (zng_rocm_uncompress_large_sizes_dev(3, &j, 1, 0, 0, NULL) != ZNG_ROCM_EINVAL) return 30;
    if (zng_rocm_uncompress_large_sizes_dev(0, &j, 1, 0, ZNG_ROCM_INFLATE_SUBBLOCK, NULL) != ZNG_ROCM_EINVAL) return 31;
    if (strstr(zng_rocm_last_error(), "0x1") == NULL) return 32;
    if (zng_rocm_uncompress_large_sizes_dev(0, &j, 1, 0, 6u, NULL) != ZNG_ROCM_EINVAL) return 33;
    if (zng_rocm_uncompress_large_sizes_dev(0, &j, 1, ((size_t)4 << 20) - 1, 0, NULL) != ZNG_ROCM_EINVAL) return 34;
    if (zng_rocm_uncompress_large_sizes_dev(0, &j, 1, (size_t)1 << 31, 0, NULL) != ZNG_ROCM_EINVAL) return 35;
    if (zng_rocm_uncompress_large_sizes_dev(0, NULL, 1, 0, 0, NULL) != ZNG_ROCM_EINVAL) return 36;
    j.window_len = 32769u;
    if (zng_rocm_uncompress_large_sizes_dev(0, &j, 1, 0, 0, NULL) != ZNG_ROCM_EINVAL) return 37;
    j.window_len = 0;
    j.d_src = NULL;
    if (zng_rocm_uncompress_large_sizes_dev(0, &j, 1, 0, 0, NULL) != ZNG_ROCM_EINVAL) return 38;
    j.d_src = bytes;
    j.src_len = (size_t)1 << 31;
    if (zng_rocm_uncompress_large_sizes_dev(0, &j, 1, 0, 0, NULL) != ZNG_ROCM_EINVAL) return 39;
    j.src_len = sizeof bytes;
    j.d_window = dict;
    j.window_len = sizeof dict;
    if (zng_rocm_uncompress_large_sizes_dev(2, &j, 1, 0, 0, NULL) != ZNG_ROCM_EINVAL) return 40;
    j.d_window = NULL;
    if (zng_rocm_uncompress_large_sizes_dev(1, &j, 1, 0, 0, NULL) != ZNG_ROCM_EINVAL) return 41;
    if (zng_rocm_uncompress_large_sizes_dev(0, &j, 1, 0, 0, NULL) != ZNG_ROCM_ENODEV) return 42;   /* raw: the length alone */
    j.window_len = 0;
    /* nothing was written */
    if (!untouched(&j)) return 50;
    if (out_len != 41u || in_used != 42u) return 51;
    puts("ok nodev");
    return 0;
}
