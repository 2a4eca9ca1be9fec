// dict.hip -- the shared preset dictionary of the many-stream calls, prepared once on the device: what
// deflateSetDictionary / inflateSetDictionary (deflate.c:456-512, inflate.c:1234-1260) do per stream -- and the reference
// amortises with one primed state that is deflateCopy'd per message -- done once for a whole batch of small messages:
//   the DICTID     Adler-32 of every byte given (deflate.c:470-471), with the streaming checksum kernel
//   the window     the last min(dict_len, 32768) bytes (the tail rule, deflate.c:477-486), copied into memory the object owns
//                  and zero padded so that the matcher's 16-byte probes stay inside
//   the head table of the level-1 class, primed: for every bucket the LAST entered position + 1 (dict_plan.h).  One atomic
//                  max per position: the result is that of entering the positions in order, whatever the scheduling.
//   the row tables of the rows engine (levels 1..9 of zng_rocm_compress_streams2_dict_dev), primed: what lz_rows_kernel's
//                  priming leaves behind the whole batches inside the window (rows_dict_table_kernel, deflate_dyn.hip).
// The object is immutable afterwards: zng_rocm_compress_streams_dict_dev / zng_rocm_uncompress_streams_dict_dev
// (framing_dev.hip) and zng_rocm_compress_streams2_dict_dev / zng_rocm_compress_members_dict_dev (compress_streams.hip) only read it, from any thread and any HIP stream of its device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dict_dev.h"

namespace zr {

__global__ __launch_bounds__(256)
void dict_head_kernel(const uint8_t *__restrict__ window, uint32_t W, uint32_t *__restrict__ head) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < dict_positions(W)) atomicMax(&head[dict_hash(dict_first4(window + p))], p + 1u);
}

int dict_usable(const zng_rocm_dict *d) {
    Context *c = ctx();
    if (!c) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    if (d && d->generation != c->generation) {
        set_error("the dictionary object was made before a zng_rocm_shutdown()");
        return ZNG_ROCM_ENODEV;
    }
    return ZNG_ROCM_OK;
}

// one allocation: head table | the DICTID on its way to the host (16 bytes) | row tables | window | padding
constexpr size_t kDictIdAt = kDictHeadSlots * sizeof(uint32_t), kDictRowsAt = kDictIdAt + 16, kDictWindowAt = kDictRowsAt + kDictRowsBytes;
static_assert(kDictRowsAt % 16 == 0 && kDictWindowAt % 16 == 0, "the matchers load tables and window in 16-byte pieces");

static int dict_fill(zng_rocm_dict *d, const uint8_t *d_dict, size_t dict_len, hipStream_t st) {
    const uint32_t W = d->window;
    uint8_t *base = reinterpret_cast<uint8_t *>(d->d_head);
    ZR_HIP(hipMemsetAsync(base, 0, kDictWindowAt + W + kDictPad, st));
    ZR_HIP(hipMemcpyAsync(d->d_window, d_dict + dict_window_start(dict_len), W, hipMemcpyDeviceToDevice, st));
    if (dict_positions(W)) {
        hipLaunchKernelGGL(dict_head_kernel, dim3((dict_positions(W) + 255u) / 256u), dim3(256), 0, st,
                           (const uint8_t *)d->d_window, W, d->d_head);
        ZR_HIP(hipGetLastError());
    }
    // (no primed position: the tables are the zeroes already there)
    if (dict_rows_primed(W))
        if (int rc = launch_rows_dict_table(d->d_window, W, d->d_rows, st)) return rc;
    uint32_t *d_id = reinterpret_cast<uint32_t *>(base + kDictIdAt);
    if (int rc = launch_checksum(true, false, 1u, 0u, d_dict, nullptr, dict_len, d_id, nullptr, st)) return rc;
    ZR_HIP(hipMemcpyAsync(&d->id, d_id, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ZR_HIP(hipStreamSynchronize(st));
    return ZNG_ROCM_OK;
}

}  // namespace zr

using namespace zr;

extern "C" {

int zng_rocm_dict_create_dev(const uint8_t *d_dict, size_t dict_len, zng_rocm_dict **out, void *stream) {
    if (out) *out = nullptr;
    if (int rc = dict_usable(nullptr)) return rc;
    if (!out || !d_dict || !dict_len) {
        set_error("a dictionary needs device memory, at least one byte and a place for the object");
        return ZNG_ROCM_EINVAL;
    }
    Context *c = ctx();
    DeviceGuard dev;
    zng_rocm_dict *d = new zng_rocm_dict();
    d->generation = c->generation;
    d->device = c->device;
    d->id = 0;
    d->window = dict_window(dict_len);
    void *base = nullptr;
    if (hipMalloc(&base, kDictWindowAt + d->window + kDictPad) != hipSuccess) {
        set_error("dictionary object: %s", hipGetErrorString(hipGetLastError()));
        delete d;
        return ZNG_ROCM_ENOMEM;
    }
    d->d_head = reinterpret_cast<uint32_t *>(base);
    d->d_window = reinterpret_cast<uint8_t *>(base) + kDictWindowAt;
    d->d_rows = reinterpret_cast<uint8_t *>(base) + kDictRowsAt;
    if (int rc = dict_fill(d, d_dict, dict_len, (hipStream_t)stream)) {
        (void)hipFree(base);
        delete d;
        return rc;
    }
    *out = d;
    return ZNG_ROCM_OK;
}

void zng_rocm_dict_destroy(zng_rocm_dict *d) {
    if (!d) return;
    // the memory belongs to the object, not to the context: it is freed the same way before and after a zng_rocm_shutdown()
    (void)hipFree(d->d_head);
    delete d;
}

uint32_t zng_rocm_dict_id(const zng_rocm_dict *d) { return d ? d->id : 0u; }

uint32_t zng_rocm_dict_window(const zng_rocm_dict *d) { return d ? d->window : 0u; }

}  // extern "C"
