/* abi_compress2_index.c -- a strict C11 consumer of zng_rocm_compress2_index_dev (include/zng_rocm.h), run WITHOUT
 * zng_rocm_init (tests/test_abi_compress2_index.py): a refused span_bytes or a null result pointer answers ZNG_ROCM_EINVAL
 * before anything else is looked at, a call that passes it answers ZNG_ROCM_ENODEV -- compress2_dev's first answer -- and
 * every return but 0 leaves *out = NULL and *dst_len as it was. */
#include <stdio.h>
#include <string.h>

#include "zng_rocm.h"

int main(void) {
    static uint8_t src[64], dst[4096];
    zng_rocm_inflate_index *idx;
    size_t dst_len;
    const uint64_t bad[4] = {1u, 65535u, ((uint64_t)1 << 30) + 1u, ~(uint64_t)0};
    const uint64_t good[4] = {0u, 65536u, (uint64_t)1 << 20, (uint64_t)1 << 30};
    /* the call's own refusal: before the missing device, before null buffers, a bad format, a bad level */
    for (int k = 0; k < 4; ++k) {
        idx = (zng_rocm_inflate_index *)src;
        dst_len = sizeof dst;
        if (zng_rocm_compress2_index_dev(dst, &dst_len, src, sizeof src, 6, 2, bad[k], &idx, NULL) != ZNG_ROCM_EINVAL) return 1;
        if (idx != NULL || dst_len != sizeof dst) return 2;
        if (strstr(zng_rocm_last_error(), "span_bytes") == NULL) return 3;
        idx = (zng_rocm_inflate_index *)src;
        if (zng_rocm_compress2_index_dev(NULL, NULL, NULL, 5, 77, 9, bad[k], &idx, NULL) != ZNG_ROCM_EINVAL) return 4;
        if (idx != NULL) return 5;
    }
    dst_len = sizeof dst;
    if (zng_rocm_compress2_index_dev(dst, &dst_len, src, sizeof src, 6, 2, 0, NULL, NULL) != ZNG_ROCM_EINVAL) return 6;
    if (zng_rocm_compress2_index_dev(NULL, NULL, NULL, 5, 77, 9, 65536u, NULL, NULL) != ZNG_ROCM_EINVAL) return 7;
    if (dst_len != sizeof dst) return 8;
    /* past it: compress2_dev's order, whose first answer is the missing device -- whatever else is wrong */
    for (int k = 0; k < 4; ++k) {
        for (int format = 0; format <= 2; ++format) {
            idx = (zng_rocm_inflate_index *)src;
            dst_len = sizeof dst;
            if (zng_rocm_compress2_index_dev(dst, &dst_len, src, sizeof src, -1, format, good[k], &idx, NULL) != ZNG_ROCM_ENODEV) return 10;
            if (idx != NULL || dst_len != sizeof dst) return 11;
            if (zng_rocm_compress2_dev(dst, &dst_len, src, sizeof src, -1, format, NULL) != ZNG_ROCM_ENODEV) return 12;
        }
        idx = (zng_rocm_inflate_index *)src;
        if (zng_rocm_compress2_index_dev(NULL, NULL, NULL, 5, 77, 9, good[k], &idx, NULL) != ZNG_ROCM_ENODEV) return 13;
        if (idx != NULL) return 14;
    }
    if (strstr(zng_rocm_last_error(), "zng_rocm_init") == NULL) return 15;
    /* the index calls take a null index */
    if (zng_rocm_inflate_index_points(NULL, NULL, 0) != 0 || zng_rocm_inflate_index_plain_len(NULL) != 0) return 16;
    zng_rocm_inflate_index_destroy(NULL);
    for (size_t i = 0; i < sizeof dst; ++i)
        if (dst[i]) return 17;
    puts("ok nodev");
    return 0;
}
