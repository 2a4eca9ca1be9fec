// hook.hip -- the device side of the COARSE boundary: what an arch/rocm DEFLATE_HOOK / INFLATE_TYPEDO_HOOK backend holds
// in its arch_deflate_state / arch_inflate_state (deflate.h:319-321, inflate.h:160-162) and calls per deflate() /
// inflate() (deflate.c:1039-1083, inflate.c:728).  The model is IBM Z DFLTCC (arch/s390/dfltcc_deflate.c,
// dfltcc_inflate.c): the history lives with the accelerator (here: 32 KiB in front of the staging buffer in HBM), the
// host code keeps zng_stream's next_in / next_out bookkeeping and falls back to software when the accelerator says no.
// Host pointers in, host pointers out: staging is this file's business (bounded: one block).
#include "context.h"
#include "deflate_dev.h"
#include "inflate_dev.h"

#include <string.h>

struct zng_rocm_hook {
    uint64_t     generation;          // of the context it was created under
    hipStream_t  st;
    uint8_t     *d_in;                // [32768 history][block]
    size_t       in_cap;              // bytes of block room
    uint32_t     hist_len;            // history is d_in[32768 - hist_len, 32768)
    uint8_t     *d_out;               // compressed block / plaintext
    size_t       out_cap;
    uint8_t     *h_out;               // pinned mirror of d_out (what the inflate side hands back)
    size_t       h_cap;
    uint32_t    *d_check;             // 2 words
    uint32_t    *h_check;             // pinned
};

namespace {
constexpr uint32_t kHist = 32768u;

int grow_device(uint8_t **p, size_t *cap, size_t want, size_t front) {
    if (*cap >= want && *p) return ZNG_ROCM_OK;
    uint8_t *n = nullptr;
    const size_t c = want + (want >> 2) + 4096;
    if (hipMalloc(&n, front + c + 64) != hipSuccess) {
        zr::set_error("device allocation of %zu bytes failed", front + c);
        return ZNG_ROCM_ENOMEM;
    }
    if (*p && front) (void)hipMemcpy(n, *p, front, hipMemcpyDeviceToDevice);      // the history survives a growth
    if (*p) (void)hipFree(*p);
    *p = n;
    *cap = c;
    return ZNG_ROCM_OK;
}

int grow_pinned(uint8_t **p, size_t *cap, size_t want) {
    if (*cap >= want && *p) return ZNG_ROCM_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    const size_t c = want + (want >> 2) + 4096;
    if (hipHostMalloc((void **)p, c, hipHostMallocDefault) != hipSuccess) {
        zr::set_error("pinned allocation of %zu bytes failed", c);
        *cap = 0;
        return ZNG_ROCM_ENOMEM;
    }
    *cap = c;
    return ZNG_ROCM_OK;
}

// history <- the last min(32768, hist + n) bytes of [history][n bytes at d_in + 32768]; through d_out (the two may overlap)
int roll_history(zng_rocm_hook *h, size_t n) {
    const size_t have = (size_t)h->hist_len + n;
    const uint32_t keep = (uint32_t)(have < kHist ? have : kHist);
    if (n == 0) return ZNG_ROCM_OK;
    if (int rc = grow_device(&h->d_out, &h->out_cap, kHist, 0)) return rc;
    const uint8_t *src = h->d_in + kHist + n - keep;
    if (hipMemcpyAsync(h->d_out, src, keep, hipMemcpyDeviceToDevice, h->st) != hipSuccess ||
        hipMemcpyAsync(h->d_in + kHist - keep, h->d_out, keep, hipMemcpyDeviceToDevice, h->st) != hipSuccess) {
        zr::set_error("history copy failed");
        return ZNG_ROCM_EHIP;
    }
    h->hist_len = keep;
    return ZNG_ROCM_OK;
}

bool stale(const zng_rocm_hook *h) { return !zr::ctx() || !h || h->generation != zr::ctx()->generation; }

constexpr size_t kHookLargeMember = 4u << 20;         // compressed bytes from which a member is decoded on the device

// the n bytes of plaintext at d_in + kHist: their check continues *check_value, they go back to the host (h_out) and become
// the history
int deliver_plaintext(zng_rocm_hook *h, size_t n, int check, uint32_t *check_value, const uint8_t **out, size_t *out_len) {
    if (grow_pinned(&h->h_out, &h->h_cap, n) != ZNG_ROCM_OK) return ZNG_ROCM_ENOMEM;
    if (check && n) {
        const int rc = check == 1 ? zng_rocm_adler32_dev(*check_value, h->d_in + kHist, n, h->d_check, h->st)
                                  : zng_rocm_crc32_dev(*check_value, h->d_in + kHist, n, h->d_check, h->st);
        if (rc != ZNG_ROCM_OK) return rc;
        ZR_HIP(hipMemcpyAsync(h->h_check, h->d_check, 4, hipMemcpyDeviceToHost, h->st));
    }
    if (n) ZR_HIP(hipMemcpyAsync(h->h_out, h->d_in + kHist, n, hipMemcpyDeviceToHost, h->st));
    if (int r2 = roll_history(h, n)) return r2;
    ZR_HIP(hipStreamSynchronize(h->st));
    if (check && n) *check_value = h->h_check[0];
    *out = h->h_out;
    *out_len = n;
    return ZNG_ROCM_OK;
}

// blocks mode on the device: 1 = done (*status = 1 or 0 as zng_rocm_inflate_tokens_decode_blocks, outputs set), 0 = leave
// it to the host decoder, negative = error
int hook_blocks_on_device(zng_rocm_hook *h, const uint8_t *in, size_t in_len, unsigned start_bit, int check,
                          uint32_t *check_value, const uint8_t **out, size_t *out_len, uint64_t *end_bit, int *status) {
    if (grow_device(&h->d_out, &h->out_cap, in_len, 0) != ZNG_ROCM_OK) return 0;          // the compressed bytes
    if (hipMemcpyAsync(h->d_out, in, in_len, hipMemcpyHostToDevice, h->st) != hipSuccess) return 0;
    size_t room = h->in_cap > 4 * in_len ? h->in_cap : 4 * in_len;                    // a guess; the call says what it needs
    uint64_t n = 0, eb = start_bit;
    int fin = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (grow_device(&h->d_in, &h->in_cap, room, kHist) != ZNG_ROCM_OK) return 0;
        const int rc = zr::inflate_large_blocks_device_only(h->d_out, in_len, start_bit, h->hist_len ? h->d_in + kHist - h->hist_len : nullptr,
                                                           h->hist_len, h->d_in + kHist, h->in_cap, &n, &eb, &fin, h->st);
        if (rc == 1) break;
        if (rc == -5 && attempt == 0 && n > h->in_cap) {
            room = (size_t)n;
            continue;
        }
        return 0;
    }
    if (int rc = deliver_plaintext(h, (size_t)n, check, check_value, out, out_len)) return rc;
    *end_bit = eb;
    *status = fin;
    return 1;
}

// 1 = stream end (outputs set), 0 = leave it to the host decoder, negative = error
int hook_inflate_on_device(zng_rocm_hook *h, const uint8_t *in, size_t in_len, int check, uint32_t *check_value,
                           const uint8_t **out, size_t *out_len, size_t *in_used) {
    if (grow_device(&h->d_out, &h->out_cap, in_len, 0) != ZNG_ROCM_OK) return 0;          // the compressed bytes
    if (hipMemcpyAsync(h->d_out, in, in_len, hipMemcpyHostToDevice, h->st) != hipSuccess) return 0;
    size_t room = h->in_cap > 4 * in_len ? h->in_cap : 4 * in_len;                    // a guess; the call says what it needs
    uint64_t n = 0;
    size_t used = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (grow_device(&h->d_in, &h->in_cap, room, kHist) != ZNG_ROCM_OK) return 0;
        const int rc = zr::inflate_large_device_only(h->d_out, in_len, h->hist_len ? h->d_in + kHist - h->hist_len : nullptr,
                                                     h->hist_len, h->d_in + kHist, h->in_cap, &n, &used, h->st);
        if (rc == 1) break;
        if (rc == -5 && attempt == 0 && n > h->in_cap) {
            room = (size_t)n;
            continue;
        }
        return 0;
    }
    if (int rc = deliver_plaintext(h, (size_t)n, check, check_value, out, out_len)) return rc;
    *in_used = used;
    return 1;
}
}  // namespace

using namespace zr;

extern "C" {

int zng_rocm_hook_create(zng_rocm_hook **out, size_t block_bytes) {
    if (!out) return ZNG_ROCM_EINVAL;
    *out = nullptr;
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    DeviceGuard dev;
    zng_rocm_hook *h = new (std::nothrow) zng_rocm_hook();
    if (!h) return ZNG_ROCM_ENOMEM;
    memset(h, 0, sizeof *h);
    h->generation = ctx()->generation;
    if (hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void **)&h->d_check, 16) != hipSuccess ||
        hipHostMalloc((void **)&h->h_check, 16, hipHostMallocDefault) != hipSuccess ||
        grow_device(&h->d_in, &h->in_cap, block_bytes ? block_bytes : (1u << 20), kHist) != ZNG_ROCM_OK) {
        set_error("hook context: stream / buffer creation failed");
        zng_rocm_hook_destroy(h);
        return ZNG_ROCM_EHIP;
    }
    *out = h;
    return ZNG_ROCM_OK;
}

void zng_rocm_hook_destroy(zng_rocm_hook *h) {
    if (!h) return;
    if (!stale(h)) {                           // after a shutdown the device objects are gone with their context
        DeviceGuard dev;
        if (h->st) {
            (void)hipStreamSynchronize(h->st);
            (void)zng_rocm_stream_release(h->st);
            (void)hipStreamDestroy(h->st);
        }
        if (h->d_in) (void)hipFree(h->d_in);
        if (h->d_out) (void)hipFree(h->d_out);
        if (h->d_check) (void)hipFree(h->d_check);
        if (h->h_out) (void)hipHostFree(h->h_out);
        if (h->h_check) (void)hipHostFree(h->h_check);
    }
    delete h;
}

// deflateCopy / inflateCopy (deflate.c:1131-1181, inflate.c:1379-1413) for a stream whose history the device holds: a new
// hook with the source's history and nothing else of it.  The history is read on the SOURCE's stream, so the copy stands
// behind whatever that stream still has in flight, and the call waits for it: afterwards the two share nothing.
int zng_rocm_hook_clone(const zng_rocm_hook *src, zng_rocm_hook **out) {
    if (!out) return ZNG_ROCM_EINVAL;
    *out = nullptr;
    if (!src) return ZNG_ROCM_EINVAL;
    if (stale(src)) {
        set_error("zng_rocm_hook_clone: no context, or a hook from before zng_rocm_shutdown()");
        return ZNG_ROCM_ENODEV;
    }
    zng_rocm_hook *h = nullptr;
    if (int rc = zng_rocm_hook_create(&h, 0)) return rc;           // the default block room, not what src has grown to
    if (src->hist_len) {
        DeviceGuard dev;
        const size_t at = kHist - src->hist_len;
        if (hipMemcpyAsync(h->d_in + at, src->d_in + at, src->hist_len, hipMemcpyDeviceToDevice, src->st) != hipSuccess ||
            hipStreamSynchronize(src->st) != hipSuccess) {
            set_error("zng_rocm_hook_clone: history copy failed");
            zng_rocm_hook_destroy(h);
            return ZNG_ROCM_EHIP;
        }
    }
    h->hist_len = src->hist_len;
    *out = h;
    return ZNG_ROCM_OK;
}

int zng_rocm_hook_reset(zng_rocm_hook *h) {
    if (stale(h)) return ZNG_ROCM_ENODEV;
    h->hist_len = 0;
    return ZNG_ROCM_OK;
}

int zng_rocm_hook_set_history(zng_rocm_hook *h, const uint8_t *dict, uint32_t len) {
    if (stale(h)) return ZNG_ROCM_ENODEV;
    if (len && !dict) return ZNG_ROCM_EINVAL;
    DeviceGuard dev;
    const uint32_t keep = len < kHist ? len : kHist;               // the last 32 KiB count (deflate.c:479-484)
    if (keep) {
        ZR_HIP(hipMemcpyAsync(h->d_in + kHist - keep, dict + (len - keep), keep, hipMemcpyHostToDevice, h->st));
        ZR_HIP(hipStreamSynchronize(h->st));
    }
    h->hist_len = keep;
    return ZNG_ROCM_OK;
}

int zng_rocm_hook_get_history(zng_rocm_hook *h, uint8_t *dict, uint32_t *len) {
    if (stale(h)) return ZNG_ROCM_ENODEV;
    DeviceGuard dev;
    if (dict && h->hist_len) {
        ZR_HIP(hipMemcpyAsync(dict, h->d_in + kHist - h->hist_len, h->hist_len, hipMemcpyDeviceToHost, h->st));
        ZR_HIP(hipStreamSynchronize(h->st));
    }
    if (len) *len = h->hist_len;
    return ZNG_ROCM_OK;
}

size_t zng_rocm_hook_deflate_bound(size_t in_len) { return zng_rocm_deflate_bound(in_len); }

int zng_rocm_hook_deflate_block(zng_rocm_hook *h, int level, const uint8_t *in, size_t in_len, uint32_t flags, int check,
                                uint32_t *check_value, uint8_t *out, size_t out_cap, size_t *out_len) {
    return zng_rocm_hook_deflate_block_strategy(h, level, 0, in, in_len, flags, check, check_value, out, out_cap, out_len);
}

int zng_rocm_hook_deflate_block_strategy(zng_rocm_hook *h, int level, int strategy, const uint8_t *in, size_t in_len,
                                         uint32_t flags, int check, uint32_t *check_value, uint8_t *out, size_t out_cap,
                                         size_t *out_len) {
    return zng_rocm_hook_deflate_block_window(h, level, strategy, 15, in, in_len, flags, check, check_value, out, out_cap, out_len);
}

// the same block at the stream's w_bits (9..15, zng_rocm_deflate_window_block_dev): the history the hook keeps is 32 KiB
// whatever the window, the matcher reaches no further back than (1 << window_bits) - 262
int zng_rocm_hook_deflate_block_window(zng_rocm_hook *h, int level, int strategy, int window_bits, const uint8_t *in, size_t in_len,
                                       uint32_t flags, int check, uint32_t *check_value, uint8_t *out, size_t out_cap,
                                       size_t *out_len) {
    if (stale(h)) return ZNG_ROCM_ENODEV;
    if (!out || !out_len || (in_len && !in) || (check && !check_value) || check < 0 || check > 2 || strategy < 0 ||
        strategy > 4 || window_bits < 9 || window_bits > 15)
        return ZNG_ROCM_EINVAL;
    DeviceGuard dev;
    if (int rc = grow_device(&h->d_in, &h->in_cap, in_len, kHist)) return rc;
    const size_t bound = zng_rocm_deflate_bound(in_len);
    if (int rc = grow_device(&h->d_out, &h->out_cap, bound, 0)) return rc;
    if (in_len) ZR_HIP(hipMemcpyAsync(h->d_in + kHist, in, in_len, hipMemcpyHostToDevice, h->st));
    if (check && in_len) {
        const int rc = check == 1 ? zng_rocm_adler32_dev(*check_value, h->d_in + kHist, in_len, h->d_check, h->st)
                                  : zng_rocm_crc32_dev(*check_value, h->d_in + kHist, in_len, h->d_check, h->st);
        if (rc != ZNG_ROCM_OK) return rc;
        ZR_HIP(hipMemcpyAsync(h->h_check, h->d_check, 4, hipMemcpyDeviceToHost, h->st));
    }
    size_t clen = 0;
    if (int rc = zng_rocm_deflate_window_block_dev(level, strategy, window_bits, h->d_in + kHist, in_len, h->hist_len, flags, h->d_out,
                                                   h->out_cap, &clen, h->st))
        return rc;
    if (clen > out_cap) {
        set_error("compressed block (%zu bytes) exceeds out_cap", clen);
        return -5;
    }
    ZR_HIP(hipMemcpyAsync(out, h->d_out, clen, hipMemcpyDeviceToHost, h->st));
    if (int rc = roll_history(h, in_len)) return rc;
    ZR_HIP(hipStreamSynchronize(h->st));
    if (check && in_len) *check_value = h->h_check[0];
    *out_len = clen;
    return ZNG_ROCM_OK;
}

int zng_rocm_hook_inflate(zng_rocm_hook *h, const uint8_t *in, size_t in_len, int check, uint32_t *check_value,
                          const uint8_t **out, size_t *out_len, size_t *in_used, const char **msg) {
    if (stale(h)) return ZNG_ROCM_ENODEV;
    if (!out || !out_len || !in_used || (in_len && !in) || (check && !check_value) || check < 0 || check > 2) return ZNG_ROCM_EINVAL;
    DeviceGuard dev;
    *out = nullptr;
    *out_len = 0;
    *in_used = 0;
    if (msg) *msg = nullptr;
    // A large member goes to the device whole (inflate_large.hip: block starts found there, one wavefront per part): the
    // host decoder below manages ~0.8 GB/s of output on its one thread.  Anything but a clean end of stream -- truncated
    // input, a data error, output larger than the estimate twice over -- is left to that decoder, whose status, message
    // and byte counts are the reference's.
    if (in_len >= kHookLargeMember) {
        const int rc = hook_inflate_on_device(h, in, in_len, check, check_value, out, out_len, in_used);
        if (rc != 0) return rc;
    }
    zng_rocm_inflate_tokens tk;
    const int status = zng_rocm_inflate_tokens_decode_window(in, in_len, h->hist_len, &tk);
    if (status != 1) {                                   // not a complete stream: nothing is consumed, nothing produced
        if (msg) *msg = tk.msg;
        zng_rocm_inflate_tokens_free(&tk);
        return status == -4 ? ZNG_ROCM_ENOMEM : status;
    }
    const size_t n = (size_t)tk.out_len;
    int rc = grow_device(&h->d_in, &h->in_cap, n, kHist);               // the plaintext lands behind the history
    if (rc == ZNG_ROCM_OK) rc = grow_pinned(&h->h_out, &h->h_cap, n);
    if (rc == ZNG_ROCM_OK)
        rc = inflate_tokens_to_device(&tk, h->hist_len ? h->d_in + kHist - h->hist_len : nullptr, h->hist_len, h->d_in + kHist, h->st);
    *in_used = tk.in_used;
    zng_rocm_inflate_tokens_free(&tk);
    if (rc != ZNG_ROCM_OK) return rc;
    if ((rc = deliver_plaintext(h, n, check, check_value, out, out_len)) != ZNG_ROCM_OK) return rc;
    return 1;                                            // Z_STREAM_END
}

int zng_rocm_hook_inflate_blocks(zng_rocm_hook *h, const uint8_t *in, size_t in_len, unsigned start_bit, int check,
                                 uint32_t *check_value, const uint8_t **out, size_t *out_len, uint64_t *end_bit,
                                 const char **msg) {
    if (stale(h)) return ZNG_ROCM_ENODEV;
    if (!out || !out_len || !end_bit || (in_len && !in) || start_bit > 7u || (check && !check_value) || check < 0 || check > 2)
        return ZNG_ROCM_EINVAL;
    DeviceGuard dev;
    *out = nullptr;
    *out_len = 0;
    *end_bit = start_bit;
    if (msg) *msg = nullptr;
    if (in_len == 0) return 0;                           // no bits: no block complete, nothing consumed, no launch
    // as zng_rocm_hook_inflate: a large piece goes to the device in parts, whatever is irregular there (a data error, a
    // stream without findable block starts) to the host decoder, whose statuses and messages are the reference's
    if (in_len >= kHookLargeMember) {
        int status = 0;
        const int rc = hook_blocks_on_device(h, in, in_len, start_bit, check, check_value, out, out_len, end_bit, &status);
        if (rc < 0) return rc;
        if (rc == 1) return status;
    }
    // (start_bit <= 7 < 8 * in_len here, and the other arguments are checked above: the decoder's ZNG_ROCM_EINVAL, which has
    // the value of Z_DATA_ERROR, cannot come back; it would carry no message and be told apart by that)
    zng_rocm_inflate_tokens tk;
    memset(&tk, 0, sizeof tk);
    uint64_t eb = start_bit;
    const int status = zng_rocm_inflate_tokens_decode_blocks(in, in_len, start_bit, h->hist_len, &tk, &eb);
    if ((status != 1 && status != 0 && status != -3) || (status == -3 && !tk.msg)) {
        zng_rocm_inflate_tokens_free(&tk);
        return status == -4 ? ZNG_ROCM_ENOMEM : ZNG_ROCM_EINVAL;
    }
    const char *text = tk.msg;                           // (a static string)
    const size_t n = (size_t)tk.out_len;
    int rc = ZNG_ROCM_OK;
    if (n) {                                             // no block complete: no launch, the history stays
        rc = grow_device(&h->d_in, &h->in_cap, n, kHist);
        if (rc == ZNG_ROCM_OK)
            rc = inflate_tokens_to_device(&tk, h->hist_len ? h->d_in + kHist - h->hist_len : nullptr, h->hist_len, h->d_in + kHist, h->st);
    }
    zng_rocm_inflate_tokens_free(&tk);
    if (rc != ZNG_ROCM_OK) return rc;
    if (n && (rc = deliver_plaintext(h, n, check, check_value, out, out_len)) != ZNG_ROCM_OK) return rc;
    *end_bit = eb;
    if (status == -3 && msg) *msg = text;
    return status;
}

}  // extern "C"
