/* arch/rocm/rocm_deflate.h -- the hook block deflate.c includes instead of its defaults when ROCM_DEFLATE is defined
 * (deflate.c:72-106; precedent arch/s390/dfltcc_deflate.h:17-56).  Two additions the reference does not have yet:
 * DEFLATE_END_HOOK, invoked from deflateEnd() before free_deflate() -- DFLTCC owns no resources, a GPU backend does;
 * DEFLATE_COPY_HOOK, invoked from deflateCopy() behind the memcpy of the state block, as soon as the copy has an allocation
 * record of its own (deflate.c:1152) and in front of every later failure path (:1158) -- that memcpy is all DFLTCC's plain-data
 * block needs, ours holds owning pointers.  On a value other than Z_OK deflateCopy calls deflateEnd(dest) and returns it
 * (INTEGRATION.md section 6).
 * Function names carry `archrocm_`, not `rocm_`: under the native API PREFIX() prepends `zng_`, and `zng_rocm_*` is the name space of
 * libzng_rocm's own entry points (a `zng_rocm_deflate_bound` here would shadow the library's).
 */
#ifndef ROCM_DEFLATE_H_
#define ROCM_DEFLATE_H_
#include "rocm_common.h"

/* zlib's strategy codes (zlib-ng.h.in) under names of the adapter's own: tests/c/zlibng_coarse_min.h, the strict-C11
 * stand-in for the reference's headers, defines only the first two */
#define ROCM_Z_DEFAULT_STRATEGY 0
#define ROCM_Z_FILTERED 1
#define ROCM_Z_HUFFMAN_ONLY 2
#define ROCM_Z_RLE 3
#define ROCM_Z_FIXED 4
#ifndef ZNG_ROCM_STANDALONE_CHECK
_Static_assert(ROCM_Z_DEFAULT_STRATEGY == Z_DEFAULT_STRATEGY && ROCM_Z_FILTERED == Z_FILTERED &&
               ROCM_Z_HUFFMAN_ONLY == Z_HUFFMAN_ONLY && ROCM_Z_RLE == Z_RLE && ROCM_Z_FIXED == Z_FIXED,
               "arch/rocm strategy codes differ from zlib-ng.h");
#endif

void Z_INTERNAL PREFIX(archrocm_reset_deflate_state)(PREFIX3(streamp) strm);
void Z_INTERNAL PREFIX(archrocm_deflate_end)(PREFIX3(streamp) strm);
int  Z_INTERNAL PREFIX(archrocm_deflate_copy)(PREFIX3(streamp) dest, PREFIX3(streamp) source);
int  Z_INTERNAL PREFIX(archrocm_can_deflate)(PREFIX3(streamp) strm);
int  Z_INTERNAL PREFIX(archrocm_deflate)(PREFIX3(streamp) strm, int flush, block_state *result);
int  Z_INTERNAL PREFIX(archrocm_deflate_params)(PREFIX3(streamp) strm, int level, int strategy, int *flush);
int  Z_INTERNAL PREFIX(archrocm_deflate_done)(PREFIX3(streamp) strm, int flush);
int  Z_INTERNAL PREFIX(archrocm_deflate_set_dictionary)(PREFIX3(streamp) strm, const unsigned char *dictionary, unsigned dict_length);
int  Z_INTERNAL PREFIX(archrocm_deflate_get_dictionary)(PREFIX3(streamp) strm, unsigned char *dictionary, unsigned *dict_length);
size_t Z_INTERNAL PREFIX(archrocm_deflate_bound)(size_t source_len);

#define DEFLATE_SET_DICTIONARY_HOOK(strm, dict, dict_len) \
    do { \
        if (PREFIX(archrocm_can_deflate)((strm))) \
            return PREFIX(archrocm_deflate_set_dictionary)((strm), (dict), (dict_len)); \
    } while (0)
#define DEFLATE_GET_DICTIONARY_HOOK(strm, dict, dict_len) \
    do { \
        if (PREFIX(archrocm_can_deflate)((strm))) \
            return PREFIX(archrocm_deflate_get_dictionary)((strm), (dict), (dict_len)); \
    } while (0)
#define DEFLATE_RESET_KEEP_HOOK PREFIX(archrocm_reset_deflate_state)
#define DEFLATE_END_HOOK PREFIX(archrocm_deflate_end)
#define DEFLATE_COPY_HOOK PREFIX(archrocm_deflate_copy)
#define DEFLATE_PARAMS_HOOK(strm, level, strategy, hook_flush) \
    do { \
        int err = PREFIX(archrocm_deflate_params)((strm), (level), (strategy), (hook_flush)); \
        if (err == Z_STREAM_ERROR) \
            return err; \
    } while (0)
#define DEFLATE_DONE PREFIX(archrocm_deflate_done)
#define DEFLATE_BOUND_ADJUST_COMPLEN(strm, complen, source_len) \
    do { \
        if (deflateStateCheck((strm)) || PREFIX(archrocm_can_deflate)((strm))) \
            (complen) = PREFIX(archrocm_deflate_bound)(source_len); \
    } while (0)
#define DEFLATE_NEED_CONSERVATIVE_BOUND(strm) (PREFIX(archrocm_can_deflate)((strm)))
#define DEFLATE_HOOK PREFIX(archrocm_deflate)
#define DEFLATE_NEED_CHECKSUM(strm) (!PREFIX(archrocm_can_deflate)((strm)))
/* the device's output is a function of the input and of where the caller flushes, nothing else */
#define DEFLATE_CAN_SET_REPRODUCIBLE(strm, reproducible) 1
#define DEFLATE_ADJUST_WINDOW_SIZE(n) (n)
#endif
