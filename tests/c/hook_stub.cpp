// tests/c/hook_stub.cpp -- TEST INFRASTRUCTURE: the zng_rocm_hook_* calls of include/zng_rocm.h on the CPU, so that the state
// machines of integration/arch/rocm/rocm_deflate.c and rocm_inflate.c (gather, drain, carry, copy) run where no GPU is, and
// under ASan / UBSan (tools/sanitize_coarse_copy.sh).  Nothing in the product links it.
//   deflate   a block leaves as stored blocks (RFC 1951 3.2.4) that honour ZNG_ROCM_BLOCK_NOT_FINAL; the check value continues
//   inflate   the project's own host decoder (zlib-ng_amd/csrc/inflate_host.cpp, compiled into the same program):
//             zng_rocm_inflate_tokens_decode_blocks, then a byte replay of its tokens against the 32 KiB history
//   memory    every hook owns a heap buffer for its history, and the plaintext a decode hands out is a fresh heap block that
//             the NEXT call on that hook frees ("valid until the next call"): two streams that share a hook, a hook released
//             twice, or plaintext read through a stale pointer are what a sanitizer then reports
// HOOK_STUB_FAIL_CLONE=1 in the environment makes zng_rocm_hook_clone fail as a device would (ZNG_ROCM_EHIP).
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "zng_rocm.h"

struct zng_rocm_hook {
    uint8_t *hist;          // 32768 bytes, the history is hist[32768 - hist_len, 32768)
    uint32_t hist_len;
    uint8_t *out;           // plaintext of the last decode
};

namespace {
constexpr uint32_t kHist = 32768u;

uint32_t adler32(uint32_t adler, const uint8_t *buf, size_t len) {
    uint32_t s1 = adler & 0xffff, s2 = (adler >> 16) & 0xffff;
    while (len) {
        size_t n = len < 5552 ? len : 5552;             // the largest run that cannot overflow 32 bits
        len -= n;
        while (n--) {
            s1 += *buf++;
            s2 += s1;
        }
        s1 %= 65521u;
        s2 %= 65521u;
    }
    return s1 | (s2 << 16);
}

uint32_t crc32(uint32_t crc, const uint8_t *buf, size_t len) {
    static uint32_t table[256];
    if (!table[1])
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
            table[i] = c;
        }
    crc = ~crc;
    for (size_t i = 0; i < len; ++i) crc = table[(crc ^ buf[i]) & 0xff] ^ (crc >> 8);
    return ~crc;
}

uint32_t check_of(int check, uint32_t v, const uint8_t *buf, size_t len) {
    return check == 1 ? adler32(v, buf, len) : check == 2 ? crc32(v, buf, len) : v;
}

// history <- the last min(32768, hist_len + n) bytes of [history][p, p + n)
void roll_history(zng_rocm_hook *h, const uint8_t *p, size_t n) {
    if (n >= kHist) {
        memcpy(h->hist, p + (n - kHist), kHist);
        h->hist_len = kHist;
        return;
    }
    const uint32_t keep_old = h->hist_len + n > kHist ? kHist - (uint32_t)n : h->hist_len;
    memmove(h->hist + kHist - n - keep_old, h->hist + kHist - keep_old, keep_old);
    memcpy(h->hist + kHist - n, p, n);
    h->hist_len = keep_old + (uint32_t)n;
}
}  // namespace

extern "C" {

int zng_rocm_device_count(void) { return 1; }
int zng_rocm_init(int) { return ZNG_ROCM_OK; }
int zng_rocm_inflate_large_last_parts(void) { return 0; }

// the functable slots of rocm_slots.c (linked for its rocm_cpu_* helpers): no device, the CPU tier answers
int zng_rocm_adler32_try(uint32_t, const uint8_t *, size_t, uint32_t *) { return ZNG_ROCM_ENODEV; }
int zng_rocm_adler32_fold_copy_try(uint32_t, uint8_t *, const uint8_t *, size_t, uint32_t *) { return ZNG_ROCM_ENODEV; }
int zng_rocm_crc32_try(uint32_t, const uint8_t *, size_t, uint32_t *) { return ZNG_ROCM_ENODEV; }
int zng_rocm_crc32_fold_try(zng_rocm_crc32_fold_t *, const uint8_t *, size_t, uint32_t) { return ZNG_ROCM_ENODEV; }
int zng_rocm_crc32_fold_copy_try(zng_rocm_crc32_fold_t *, uint8_t *, const uint8_t *, size_t) { return ZNG_ROCM_ENODEV; }

int zng_rocm_hook_create(zng_rocm_hook **out, size_t) {
    if (!out) return ZNG_ROCM_EINVAL;
    *out = nullptr;
    zng_rocm_hook *h = (zng_rocm_hook *)calloc(1, sizeof *h);
    if (!h) return ZNG_ROCM_ENOMEM;
    if (!(h->hist = (uint8_t *)malloc(kHist))) {
        free(h);
        return ZNG_ROCM_ENOMEM;
    }
    *out = h;
    return ZNG_ROCM_OK;
}

void zng_rocm_hook_destroy(zng_rocm_hook *h) {
    if (!h) return;
    free(h->hist);
    free(h->out);
    free(h);
}

int zng_rocm_hook_reset(zng_rocm_hook *h) {
    if (!h) return ZNG_ROCM_ENODEV;
    h->hist_len = 0;
    return ZNG_ROCM_OK;
}

int zng_rocm_hook_set_history(zng_rocm_hook *h, const uint8_t *dict, uint32_t len) {
    if (!h) return ZNG_ROCM_ENODEV;
    if (len && !dict) return ZNG_ROCM_EINVAL;
    const uint32_t keep = len < kHist ? len : kHist;
    if (keep) memcpy(h->hist + kHist - keep, dict + (len - keep), keep);
    h->hist_len = keep;
    return ZNG_ROCM_OK;
}

int zng_rocm_hook_get_history(zng_rocm_hook *h, uint8_t *dict, uint32_t *len) {
    if (!h) return ZNG_ROCM_ENODEV;
    if (dict && h->hist_len) memcpy(dict, h->hist + kHist - h->hist_len, h->hist_len);
    if (len) *len = h->hist_len;
    return ZNG_ROCM_OK;
}

int zng_rocm_hook_clone(const zng_rocm_hook *src, zng_rocm_hook **out) {
    if (!out) return ZNG_ROCM_EINVAL;
    *out = nullptr;
    if (!src) return ZNG_ROCM_EINVAL;
    if (getenv("HOOK_STUB_FAIL_CLONE")) return ZNG_ROCM_EHIP;
    zng_rocm_hook *h = nullptr;
    if (int rc = zng_rocm_hook_create(&h, 0)) return rc;
    if (src->hist_len) memcpy(h->hist + kHist - src->hist_len, src->hist + kHist - src->hist_len, src->hist_len);
    h->hist_len = src->hist_len;
    *out = h;
    return ZNG_ROCM_OK;
}

size_t zng_rocm_hook_deflate_bound(size_t in_len) { return in_len + 5 * (in_len / 65535u + 1); }

int zng_rocm_hook_deflate_block_window(zng_rocm_hook *h, int level, int strategy, int window_bits, const uint8_t *in, size_t in_len,
                                       uint32_t flags, int check, uint32_t *check_value, uint8_t *out, size_t out_cap,
                                       size_t *out_len) {
    if (!h) return ZNG_ROCM_ENODEV;
    if (!out || !out_len || (in_len && !in) || (check && !check_value) || check < 0 || check > 2 || level < 0 || level > 9 ||
        strategy < 0 || strategy > 4 || window_bits < 9 || window_bits > 15)
        return ZNG_ROCM_EINVAL;
    if (out_cap < zng_rocm_hook_deflate_bound(in_len)) return -5;
    const int final = !(flags & ZNG_ROCM_BLOCK_NOT_FINAL);
    size_t o = 0, left = in_len;
    const uint8_t *p = in;
    do {
        const size_t ln = left > 65535u ? 65535u : left;
        out[o++] = (uint8_t)((final && ln == left) ? 1 : 0);
        out[o++] = (uint8_t)ln;
        out[o++] = (uint8_t)(ln >> 8);
        out[o++] = (uint8_t)~ln;
        out[o++] = (uint8_t)(~ln >> 8);
        if (ln) memcpy(out + o, p, ln);
        o += ln;
        p += ln;
        left -= ln;
    } while (left);
    if (check) *check_value = check_of(check, *check_value, in, in_len);
    roll_history(h, in, in_len);
    *out_len = o;
    return ZNG_ROCM_OK;
}

int zng_rocm_hook_inflate_blocks(zng_rocm_hook *h, const uint8_t *in, size_t in_len, unsigned start_bit, int check,
                                 uint32_t *check_value, const uint8_t **out, size_t *out_len, uint64_t *end_bit,
                                 const char **msg) {
    if (!h) return ZNG_ROCM_ENODEV;
    if (!out || !out_len || !end_bit || (in_len && !in) || start_bit > 7u || (check && !check_value) || check < 0 || check > 2)
        return ZNG_ROCM_EINVAL;
    *out = nullptr;
    *out_len = 0;
    *end_bit = start_bit;
    if (msg) *msg = nullptr;
    if (in_len == 0) return 0;
    zng_rocm_inflate_tokens tk;
    memset(&tk, 0, sizeof tk);
    uint64_t eb = start_bit;
    const int status = zng_rocm_inflate_tokens_decode_blocks(in, in_len, start_bit, h->hist_len, &tk, &eb);
    if ((status != 1 && status != 0 && status != -3) || (status == -3 && !tk.msg)) {
        zng_rocm_inflate_tokens_free(&tk);
        return status == -4 ? ZNG_ROCM_ENOMEM : ZNG_ROCM_EINVAL;
    }
    const char *text = tk.msg;
    const size_t n = (size_t)tk.out_len, hl = h->hist_len;
    if (n) {
        // [history][plaintext] in one block, so that a distance may reach back into the history
        uint8_t *buf = (uint8_t *)malloc(hl + n);
        if (!buf) {
            zng_rocm_inflate_tokens_free(&tk);
            return ZNG_ROCM_ENOMEM;
        }
        if (hl) memcpy(buf, h->hist + kHist - hl, hl);
        size_t at = hl, lit = 0;
        for (size_t t = 0; t < tk.ntokens; ++t) {
            const uint32_t tok = tk.tokens[t];
            if (!(tok >> 31)) {
                if (tok > tk.nliterals - lit || tok > hl + n - at) abort();     // the decoder's own accounting is off
                memcpy(buf + at, tk.literals + lit, tok);
                lit += tok;
                at += tok;
            } else {
                const size_t len = ((tok >> 16) & 0xff) + 3, dist = (tok & 0xffff) + 1;
                if (dist > at || len > hl + n - at) abort();
                for (size_t k = 0; k < len; ++k, ++at) buf[at] = buf[at - dist];
            }
        }
        if (at != hl + n) abort();
        free(h->out);                                        // what the last call handed out ends here
        h->out = (uint8_t *)malloc(n);
        if (!h->out) {
            free(buf);
            zng_rocm_inflate_tokens_free(&tk);
            return ZNG_ROCM_ENOMEM;
        }
        memcpy(h->out, buf + hl, n);
        free(buf);
        if (check) *check_value = check_of(check, *check_value, h->out, n);
        roll_history(h, h->out, n);
        *out = h->out;
        *out_len = n;
    }
    zng_rocm_inflate_tokens_free(&tk);
    *end_bit = eb;
    if (status == -3 && msg) *msg = text;
    return status;
}

}  // extern "C"
