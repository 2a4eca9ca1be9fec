// checksum_args.h -- the message descriptors of the streaming checksum kernels (checksum_kernel.h), shared with the
// translation units that fill them on the DEVICE (framing_dev.hip: the checksums of many inflated streams whose
// lengths only the device knows).
#pragma once
#include "context.h"

namespace zr {

// What the CRC prologue needs to BUILD its tables in registers instead of fetching them: entry e of a table that is
// linear over GF(2) is the XOR of the entries of e's set bits, so eight words per table suffice.  They travel as
// kernel arguments (scalar loads from the kernarg segment): the prologue touches no table in HBM at all -- measured,
// the fetch of the 9 KiB of tables cost 2.1-2.6 us per launch (L2 is flushed by the pass between two launches).
struct CrcBits {
    uint32_t stride[4][8];    // stride_tab[k][1 << i]
    uint32_t x32[4][8];       // x32_tab[k][1 << i]
};

struct StreamArgs {
    const uint8_t *a0;        // 16-byte aligned
    uint8_t       *dst0;      // COPY: destination of byte a0[0] (same 16-byte phase as a0), else unused
    long long      n;         // message bytes
    long long      body;      // tail_base - a0 (multiple of 16, >= 0)
    long long      nunits;    // ceil(body / kUnitBytes)
    int            head;      // buf - a0, 0..15
    int            tail;      // bytes of the message living in the granule at tail_base
    unsigned long long *phase_stamps;   // tools/micro only (PROFILE instantiations): 8 stamps per workgroup
    CrcBits        bits;
};

struct FinalArgs {
    const uint8_t *tail_base;   // granule holding the trailing bytes
    uint8_t       *tail_dst;    // COPY: where those bytes go (else nullptr)
    long long      n;
    long long      nunits;
    int            tail_lo;     // valid bytes of that granule: [tail_lo, tail_hi)
    int            tail_hi;
    int            groups;
    uint32_t       adler_seed;
    uint32_t       crc_seed;
    uint32_t       crc_len_pow;     // x^(8n), evaluated on the host (a handful of table multiplies)
    // seeds chained on the device (the bounded host-pointer staging of slots.hip): when non-null they replace the
    // two scalar seeds above with the words an earlier launch on the same stream wrote
    const uint32_t *adler_seed_ptr;
    const uint32_t *crc_seed_ptr;
    int            do_adler, do_crc;
};

// many-message pass over descriptors that already sit in device memory (checksum.hip): rows messages, one workgroup
// each, `d_part` rows Partial of scratch, two result words per message at d_out2
int launch_checksum_batch_device(bool do_adler, bool do_crc, const StreamArgs *d_messages, const FinalArgs *d_finals,
                                 Partial *d_part, size_t rows, uint32_t *d_out2, hipStream_t stream);

#if defined(__HIPCC__)
// The descriptors of one message of the many-message pass (one workgroup per message, seeds 1 / 0), built ON THE DEVICE as
// checksum.hip's host code builds them: for messages whose address or length only the device knows, or that are cut there.
__device__ __forceinline__ void fill_check_descriptor(const uint8_t *buf, uint64_t len, const DeviceTables *__restrict__ tabs, int do_adler,
                                             int do_crc, StreamArgs *sa, FinalArgs *fa) {
    const uintptr_t p = (uintptr_t)buf;
    const uintptr_t a0 = p & ~(uintptr_t)15, tail_base = (p + len) & ~(uintptr_t)15;
    StreamArgs s;
    s.a0 = (const uint8_t *)a0;
    s.dst0 = nullptr;
    s.n = (long long)len;
    s.body = (long long)(tail_base - a0);
    s.nunits = (s.body + kUnitBytes - 1) / kUnitBytes;
    s.head = (int)(p - a0);
    s.tail = (int)((p + len) - tail_base);
    s.phase_stamps = nullptr;
    for (int k = 0; k < 4; ++k)
        for (int b = 0; b < 8; ++b) {
            s.bits.stride[k][b] = tabs->stride_tab[k][1u << b];
            s.bits.x32[k][b] = tabs->x32_tab[k][1u << b];
        }
    *sa = s;
    FinalArgs f;
    f.tail_base = (const uint8_t *)tail_base;
    f.tail_dst = nullptr;
    f.n = s.n;
    f.nunits = s.nunits;
    f.tail_lo = s.body == 0 ? s.head : 0;
    f.tail_hi = s.tail;
    if (len == 0) f.tail_lo = f.tail_hi = 0;
    f.groups = 1;
    f.adler_seed = 1;
    f.crc_seed = 0;
    f.crc_len_pow = do_crc ? xpow_bytes(tabs->pow_tab, len) : 0u;
    f.adler_seed_ptr = nullptr;
    f.crc_seed_ptr = nullptr;
    f.do_adler = do_adler;
    f.do_crc = do_crc;
    *fa = f;
}
#endif

}  // namespace zr
