/* abi_dict.c -- a strict C11 consumer of the shared-dictionary entry points of include/zng_rocm.h, run WITHOUT
 * zng_rocm_init (tests/test_abi_dict.py): zng_rocm_dict_create_dev returns ZNG_ROCM_ENODEV and hands out no object, the calls
 * that take one answer the same, zng_rocm_dict_destroy(NULL) is harmless, and the bound is 0 for a format the call refuses. */
#include <stdio.h>
#include <string.h>

#include "zng_rocm.h"

int main(void) {
    static uint8_t bytes[64];
    zng_rocm_dict *d = (zng_rocm_dict *)bytes;            /* must come back NULL */
    uint32_t results[4] = {41u, 42u, 43u, 44u};
    zng_rocm_stream_job cj;
    zng_rocm_inflate_dev_job ij;
    memset(&cj, 0, sizeof cj);
    memset(&ij, 0, sizeof ij);
    if (zng_rocm_dict_create_dev(bytes, sizeof bytes, &d, NULL) != ZNG_ROCM_ENODEV || d != NULL) return 1;
    if (zng_rocm_dict_create_dev(NULL, 0, &d, NULL) != ZNG_ROCM_ENODEV || d != NULL) return 2;
    zng_rocm_dict_destroy(NULL);
    if (zng_rocm_dict_id(NULL) != 0u || zng_rocm_dict_window(NULL) != 0u) return 3;
    if (zng_rocm_compress_streams_dict_bound(1000, 2) != 0 || zng_rocm_compress_streams_dict_bound(1000, -1) != 0 ||
        zng_rocm_compress_streams_dict_bound(1000, 3) != 0) return 4;
    if (zng_rocm_compress_streams_dict_bound(1000, 0) != zng_rocm_compress_streams_bound(1000, 0)) return 5;
    /* the wrapper with the DICTID is four bytes longer than the one without */
    if (zng_rocm_compress_streams_dict_bound(1000, 1) != zng_rocm_compress_streams_bound(1000, 1) + 4) return 6;
    if (zng_rocm_compress_streams_dict_dev(1, NULL, &cj, 1, results, NULL) != ZNG_ROCM_ENODEV) return 7;
    if (zng_rocm_uncompress_streams_dict_dev(1, NULL, &ij, 1, results, NULL) != ZNG_ROCM_ENODEV) return 8;
    if (results[0] != 41u || results[1] != 42u || results[2] != 43u || results[3] != 44u) return 9;
    puts("ok nodev");
    return 0;
}
