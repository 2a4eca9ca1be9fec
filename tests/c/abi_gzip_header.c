/* abi_gzip_header.c -- a strict C11 consumer of the gzip header calls of include/zng_rocm.h, run WITHOUT zng_rocm_init
 * (tests/test_abi_gzip_header.py): the layouts of both structures, the two host calls at work without a device, the three
 * device calls refusing what they refuse before the device is asked for and answering ZNG_ROCM_ENODEV with nothing written. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "zng_rocm.h"

_Static_assert(sizeof(zng_rocm_gzip_header) == 48, "zng_rocm_gzip_header is 48 bytes");
_Static_assert(offsetof(zng_rocm_gzip_header, time) == 0 && offsetof(zng_rocm_gzip_header, os) == 4 &&
               offsetof(zng_rocm_gzip_header, text) == 8 && offsetof(zng_rocm_gzip_header, hcrc) == 12 &&
               offsetof(zng_rocm_gzip_header, extra) == 16 && offsetof(zng_rocm_gzip_header, name) == 24 &&
               offsetof(zng_rocm_gzip_header, comment) == 32 && offsetof(zng_rocm_gzip_header, extra_len) == 40 &&
               offsetof(zng_rocm_gzip_header, reserved) == 44, "zng_rocm_gzip_header layout");
_Static_assert(sizeof(zng_rocm_gzip_header_row) == 96, "zng_rocm_gzip_header_row is 96 bytes");
_Static_assert(offsetof(zng_rocm_gzip_header_row, status) == 0 && offsetof(zng_rocm_gzip_header_row, flg) == 4 &&
               offsetof(zng_rocm_gzip_header_row, msg) == 8 && offsetof(zng_rocm_gzip_header_row, header_len) == 16 &&
               offsetof(zng_rocm_gzip_header_row, time) == 24 && offsetof(zng_rocm_gzip_header_row, xflags) == 28 &&
               offsetof(zng_rocm_gzip_header_row, os) == 32 && offsetof(zng_rocm_gzip_header_row, text) == 36 &&
               offsetof(zng_rocm_gzip_header_row, hcrc) == 40 && offsetof(zng_rocm_gzip_header_row, extra_len) == 44 &&
               offsetof(zng_rocm_gzip_header_row, name_len) == 48 && offsetof(zng_rocm_gzip_header_row, comment_len) == 56 &&
               offsetof(zng_rocm_gzip_header_row, extra_off) == 64 && offsetof(zng_rocm_gzip_header_row, name_off) == 72 &&
               offsetof(zng_rocm_gzip_header_row, comment_off) == 80 && offsetof(zng_rocm_gzip_header_row, text_off) == 88,
               "zng_rocm_gzip_header_row layout");

int main(void) {
    static uint8_t in[64], out[4096], file[64], text[64];
    static const uint8_t sub[6] = {'B', 'C', 2, 0, 0x1b, 0};
    uint8_t head[64];
    uint32_t results[2] = {41u, 42u}, checks[1] = {43u};
    uint64_t offsets[2] = {44u, 45u};
    size_t need = 77, n, k;
    zng_rocm_stream_job j;
    zng_rocm_gzip_header h;
    zng_rocm_gzip_header_row row, rows[1];
    zng_rocm_gzip_member m;
    memset(&j, 0, sizeof j);
    memset(&h, 0, sizeof h);
    memset(&m, 0, sizeof m);
    memset(rows, 0x5a, sizeof rows);
    j.in = in;
    j.in_len = sizeof in;
    j.out = out;
    j.out_cap = sizeof out;
    /* the host calls: 10 + (2 + 6) + 6 + 3 + 2 bytes, FLG 1e, and back */
    h.time = 0x01020304u;
    h.os = 0x1ffu;
    h.hcrc = 1;
    h.extra = sub;
    h.extra_len = sizeof sub;
    h.name = "a.txt";
    h.comment = "hi";
    if (zng_rocm_gzip_header_bytes(NULL) != 10 || zng_rocm_gzip_header_bytes(&h) != 29) return 1;
    if (zng_rocm_gzip_header_write(&h, 9, 0, head, 28) != 0) return 2;
    n = zng_rocm_gzip_header_write(&h, 9, 0, head, sizeof head);
    if (n != 29 || head[0] != 0x1f || head[1] != 0x8b || head[2] != 8 || head[3] != 0x1e || head[4] != 4 || head[7] != 1 ||
        head[8] != 2 || head[9] != 0xff || head[10] != 6 || head[11] != 0 || memcmp(head + 12, sub, 6) ||
        memcmp(head + 18, "a.txt", 6) || memcmp(head + 24, "hi", 3))
        return 3;
    if (zng_rocm_gzip_header_parse(head, n, &row) != 0 || row.status != 0 || row.msg != NULL || row.header_len != 29 ||
        row.flg != 0x1e || row.time != 0x01020304u || row.xflags != 2 || row.os != 0xff || row.text != 0 || row.hcrc != 1 ||
        row.extra_len != 6 || row.extra_off != 12 || row.name_len != 5 || row.name_off != 18 || row.comment_len != 2 ||
        row.comment_off != 24 || row.text_off != 0)
        return 4;
    head[n - 1] ^= 1u;
    if (zng_rocm_gzip_header_parse(head, n, &row) != -3 || !row.msg || strcmp(row.msg, "header crc mismatch") || row.header_len) return 5;
    if (zng_rocm_gzip_header_parse(head, 20, &row) != -5 || row.msg) return 6;
    /* the device calls: refusals first */
    h.reserved = 1;
    if (zng_rocm_gzip_header_bytes(&h) != 0) return 7;
    if (zng_rocm_compress_streams2_header_dev(6, 0, 15, &j, &h, 1, 0, results, NULL) != ZNG_ROCM_EINVAL) return 8;
    if (zng_rocm_compress_members_header_dev(6, 0, 15, &j, &h, 1, out, sizeof out, 0, offsets, checks, NULL) != ZNG_ROCM_EINVAL) return 9;
    h.reserved = 0;
    if (zng_rocm_compress_members_header_dev(6, 0, 8, &j, &h, 1, out, sizeof out, 0, offsets, checks, NULL) != ZNG_ROCM_EINVAL) return 10;
    if (zng_rocm_compress_streams2_header_dev(10, 0, 15, &j, &h, 1, 0, results, NULL) != ZNG_ROCM_EINVAL) return 11;
    j.out_cap = (uint32_t)(zng_rocm_compress_streams2_bound(sizeof in, 2) - 10 + zng_rocm_gzip_header_bytes(&h)) - 1u;
    if (zng_rocm_compress_streams2_header_dev(6, 0, 15, &j, &h, 1, 0, results, NULL) != -5) return 12;
    j.out_cap += 1u;
    if (zng_rocm_compress_streams2_header_dev(6, 0, 15, &j, &h, 1, 0, results, NULL) != ZNG_ROCM_ENODEV) return 13;
    if (zng_rocm_compress_streams2_header_dev(6, 0, 15, &j, NULL, 1, 0, results, NULL) != ZNG_ROCM_ENODEV) return 14;
    if (zng_rocm_compress_members_header_dev(-1, 3, 9, &j, &h, 1, out, sizeof out, 0, offsets, checks, NULL) != ZNG_ROCM_ENODEV) return 15;
    if (zng_rocm_compress_members_header_dev(6, 0, 15, NULL, NULL, 0, NULL, 0, 0, NULL, NULL, NULL) != ZNG_ROCM_OK) return 16;
    m.src_off = 60;
    m.src_len = 5;                                           /* ends behind the file */
    if (zng_rocm_gzip_headers_dev(file, sizeof file, &m, 1, rows, text, sizeof text, &need, NULL) != ZNG_ROCM_EINVAL || need != 0) return 17;
    m.src_len = 4;
    need = 77;
    if (zng_rocm_gzip_headers_dev(file, sizeof file, &m, 1, NULL, text, sizeof text, &need, NULL) != ZNG_ROCM_EINVAL || need != 0) return 18;
    if (zng_rocm_gzip_headers_dev(file, sizeof file, &m, 1, rows, NULL, 1, &need, NULL) != ZNG_ROCM_EINVAL) return 19;
    if (zng_rocm_gzip_headers_dev(file, sizeof file, &m, 1, rows, text, sizeof text, NULL, NULL) != ZNG_ROCM_EINVAL) return 20;
    need = 77;
    if (zng_rocm_gzip_headers_dev(file, sizeof file, NULL, 0, NULL, NULL, 0, &need, NULL) != ZNG_ROCM_OK || need != 0) return 21;
    if (zng_rocm_gzip_headers_dev(file, sizeof file, &m, 1, rows, text, sizeof text, &need, NULL) != ZNG_ROCM_ENODEV) return 22;
    /* nothing was written */
    if (results[0] != 41u || results[1] != 42u || checks[0] != 43u || offsets[0] != 44u || offsets[1] != 45u) return 23;
    for (k = 0; k < sizeof out; ++k)
        if (out[k]) return 24;
    for (k = 0; k < sizeof text; ++k)
        if (text[k]) return 25;
    for (k = 0; k < sizeof rows; ++k)
        if (((const uint8_t *)rows)[k] != 0x5a) return 26;
    puts("ok nodev");
    return 0;
}
