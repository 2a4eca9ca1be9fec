/* abi_inflate_sizes.c -- a strict C11 consumer of zng_rocm_inflate_sizes_dev and zng_rocm_uncompress_packed_dev
 * (include/zng_rocm.h), run WITHOUT zng_rocm_init (tests/test_abi_inflate_sizes.py): the argument checks come first and answer
 * ZNG_ROCM_EINVAL, a call they accept answers ZNG_ROCM_ENODEV, an empty sizing call answers 0, and nothing is written either
 * way. */
#include <stdio.h>
#include <string.h>

#include "zng_rocm.h"

int main(void) {
    static uint8_t bytes[64], dst[64];
    uint32_t results[4] = {41u, 42u, 43u, 44u};
    uint64_t offsets[2] = {45u, 46u};
    zng_rocm_inflate_dev_job j;
    memset(&j, 0, sizeof j);
    memset(dst, 0x5a, sizeof dst);
    j.in = bytes;
    j.in_len = sizeof bytes;
    if (zng_rocm_inflate_sizes_dev(1, NULL, &j, 1, results, NULL) != ZNG_ROCM_ENODEV) return 1;
    if (zng_rocm_uncompress_packed_dev(1, NULL, &j, 1, dst, sizeof dst, 64, offsets, results, NULL) != ZNG_ROCM_ENODEV) return 2;
    if (zng_rocm_uncompress_packed_dev(2, NULL, NULL, 0, NULL, 0, 0, offsets, results, NULL) != ZNG_ROCM_ENODEV) return 3;
    if (zng_rocm_inflate_sizes_dev(0, NULL, NULL, 0, NULL, NULL) != ZNG_ROCM_OK) return 4;
    /* refusals, before the device is asked for */
    if (zng_rocm_inflate_sizes_dev(3, NULL, &j, 1, results, NULL) != ZNG_ROCM_EINVAL) return 5;
    if (zng_rocm_inflate_sizes_dev(1, NULL, &j, 1, NULL, NULL) != ZNG_ROCM_EINVAL) return 6;
    if (zng_rocm_uncompress_packed_dev(1, NULL, &j, 1, dst, sizeof dst, 3, offsets, results, NULL) != ZNG_ROCM_EINVAL) return 7;
    if (zng_rocm_uncompress_packed_dev(1, NULL, &j, 1, NULL, sizeof dst, 1, offsets, results, NULL) != ZNG_ROCM_EINVAL) return 8;
    if (zng_rocm_uncompress_packed_dev(1, NULL, &j, 1, dst, sizeof dst, 1, NULL, results, NULL) != ZNG_ROCM_EINVAL) return 9;
    j.flags = 1u;
    if (zng_rocm_inflate_sizes_dev(1, NULL, &j, 1, results, NULL) != ZNG_ROCM_EINVAL) return 10;
    j.flags = 0u;
    j.dict_len = 5u;
    if (zng_rocm_inflate_sizes_dev(1, NULL, &j, 1, results, NULL) != ZNG_ROCM_EINVAL) return 11;
    if (zng_rocm_uncompress_packed_dev(0, NULL, &j, 1, dst, sizeof dst, 1, offsets, results, NULL) != ZNG_ROCM_EINVAL) return 12;
    if (results[0] != 41u || results[1] != 42u || results[2] != 43u || results[3] != 44u) return 13;
    if (offsets[0] != 45u || offsets[1] != 46u) return 14;
    for (size_t k = 0; k < sizeof dst; ++k)
        if (dst[k] != 0x5a) return 15;
    puts("ok nodev");
    return 0;
}
