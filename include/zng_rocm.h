/* zng_rocm.h -- C ABI of the MI355X (gfx950) backend for zlib-ng's functable hot path.
 *
 * This is the drop-in boundary: a plain C shared library (libzng_rocm.so, built
 * by hipcc from zlib-ng_amd/csrc) whose entry points are what zlib-ng's own
 * dispatch boundary -- `struct functable_s`, functable.h:26-42 -- would bind for
 * an `arch/rocm` backend.  Pointers and sizes only; no C++/torch types.
 * INTEGRATION.md shows the reference-side stub (functable.c / arch/rocm) that
 * calls these.
 *
 * Two families of entry points:
 *
 *  1. `zng_rocm_<slot>`: the functable slot itself, same argument meaning as the
 *     reference slot, HOST pointers.  Data is staged to the device through a
 *     bounded (16 MiB) staging chunk, the HIP kernel runs, the answer comes back.
 *     They never compute on the CPU: if the device is unusable they abort() with
 *     a message (a functable slot has no error channel).  Each has a twin
 *     `zng_rocm_<slot>_try` that returns a ZNG_ROCM_E* code instead of aborting,
 *     which is what the reference-side adapter binds so that it can fall back to
 *     zlib-ng's own CPU tier ("any HIP failure must degrade to the
 *     CPU implementation").
 *
 *  2. `zng_rocm_<slot>_dev`: the same operation on data ALREADY RESIDENT IN HBM
 *     (device pointers), asynchronous on a caller-supplied HIP stream
 *     (`void *stream` is a hipStream_t; NULL = the default stream).  Results are
 *     written to device memory.  This is the measured hot path (bench.py) and
 *     what a stream-level offload (DEFLATE_HOOK / INFLATE_TYPEDO_HOOK,
 *     deflate.c:72-106, inflate_p.h:11-41) calls with its device-resident window.
 *
 * All functions return 0 on success or a negative ZNG_ROCM_E* code unless they
 * mirror a reference signature that returns a value.
 */
#ifndef ZNG_ROCM_H
#define ZNG_ROCM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZNG_ROCM_OK          0
#define ZNG_ROCM_ENODEV     (-1)   /* no usable gfx950 device / HIP runtime error at init */
#define ZNG_ROCM_EHIP       (-2)   /* a HIP call failed; see zng_rocm_last_error() */
#define ZNG_ROCM_EINVAL     (-3)   /* bad argument */
#define ZNG_ROCM_ENOMEM     (-4)

/* ---- lifecycle --------------------------------------------------------- */
/* Replaces: the feature probe an arch backend adds to cpu_features
 * (cpu_features.h:23-37, x86_features.c:69-117).  Idempotent, thread-safe.
 * Builds the constant tables in HBM for `device` (-1 = current device). */
int         zng_rocm_init(int device);
int         zng_rocm_available(void);          /* 1 after a successful init */
int         zng_rocm_device_count(void);       /* 0 when there is no GPU; never aborts */
const char *zng_rocm_last_error(void);
/* {CUs, LDS bytes per CU, wavefront size, XCDs} of the initialised device */
int         zng_rocm_device_info(int32_t out[4]);
int         zng_rocm_shutdown(void);
/* Per-stream state (partials, scratch of the stream-level entry points, staging) is created lazily for every HIP
 * stream a *_dev call is given and kept until zng_rocm_shutdown().  A caller that destroys one of its streams
 * releases that state first with this call (it synchronises the stream).  The host-pointer slots use one stream
 * per host thread and release it themselves when the thread ends. */
int         zng_rocm_stream_release(void *stream);
/* device bytes the per-stream state of `stream` holds now (its scratch and staging buffers; 0 when it has none) */
size_t      zng_rocm_workspace_bytes(void *stream);
/* The checksum kernels run one workgroup per CU for the whole pass.  A caller that overlaps them with work on
 * other HIP streams of the same device (an RCCL collective, the combine of the previous step) asks for `n` CUs
 * to be left out of that grid, so the other stream's kernels do not have to displace a workgroup the whole pass
 * waits for.  0 (the default) = use every CU.  Process-wide; takes effect at the next launch. */
int         zng_rocm_reserve_cus(int n);

/* ---- functable slots, host pointers (functable.h:26-42) ---------------- */
/* slot `adler32`: arch/generic/adler32_c.c:11-54 */
uint32_t zng_rocm_adler32(uint32_t adler, const uint8_t *buf, size_t len);
/* slot `adler32_fold_copy`: arch/generic/adler32_fold_c.c:11-15 */
uint32_t zng_rocm_adler32_fold_copy(uint32_t adler, uint8_t *dst, const uint8_t *src, size_t len);
/* slot `crc32`: arch/generic/crc32_braid_c.c:62-216 */
uint32_t zng_rocm_crc32(uint32_t crc, const uint8_t *buf, size_t len);

/* slots `crc32_fold_reset/_fold/_fold_copy/_fold_final`:
 * arch/generic/crc32_fold_c.c:10-31 over struct crc32_fold_s (crc32.h:8-14). */
typedef struct zng_rocm_crc32_fold_s {
    uint8_t  fold[64];
    uint32_t value;
} zng_rocm_crc32_fold_t;
uint32_t zng_rocm_crc32_fold_reset(zng_rocm_crc32_fold_t *crc);
void     zng_rocm_crc32_fold(zng_rocm_crc32_fold_t *crc, const uint8_t *src, size_t len, uint32_t init_crc);
void     zng_rocm_crc32_fold_copy(zng_rocm_crc32_fold_t *crc, uint8_t *dst, const uint8_t *src, size_t len);
uint32_t zng_rocm_crc32_fold_final(zng_rocm_crc32_fold_t *crc);

/* The same slots with an error channel (no reference counterpart: a functable slot returns a value only).
 * 0 and the value through *out / the updated fold state, or a negative ZNG_ROCM_E* code with nothing written and
 * the fold state unchanged; never abort().  NULL buffers behave as in the slot (adler32 -> 1, crc32 -> 0). */
int zng_rocm_adler32_try(uint32_t adler, const uint8_t *buf, size_t len, uint32_t *out);
int zng_rocm_adler32_fold_copy_try(uint32_t adler, uint8_t *dst, const uint8_t *src, size_t len, uint32_t *out);
int zng_rocm_crc32_try(uint32_t crc, const uint8_t *buf, size_t len, uint32_t *out);
int zng_rocm_crc32_fold_try(zng_rocm_crc32_fold_t *crc, const uint8_t *src, size_t len, uint32_t init_crc);
int zng_rocm_crc32_fold_copy_try(zng_rocm_crc32_fold_t *crc, uint8_t *dst, const uint8_t *src, size_t len);

/* ---- checksums on device-resident data --------------------------------- */
/* d_out: device pointer to one uint32_t.  Same value as the slot on the same
 * bytes and seed (bit-exact), including len == 0. */
int zng_rocm_adler32_dev(uint32_t adler, const void *d_buf, size_t len, uint32_t *d_out, void *stream);
int zng_rocm_crc32_dev(uint32_t crc, const void *d_buf, size_t len, uint32_t *d_out, void *stream);
/* One pass over the bytes, both checksums: d_out[0] = adler32, d_out[1] = crc32.
 * (What inflate's inf_chksum / deflate's read_buf need for a gzip+zlib pair,
 * inflate.c:25-49, deflate.c:1190-1212; BASELINE.json configs[1].) */
int zng_rocm_adler32_crc32_dev(uint32_t adler, uint32_t crc, const void *d_buf, size_t len,
                               uint32_t *d_out2, void *stream);
/* fold_copy on device: checksum `len` bytes of d_src while copying them to
 * d_dst (2N bytes of traffic).  which: 1 = adler32, 2 = crc32, 3 = both
 * (d_out2[0] adler, d_out2[1] crc; unused entries untouched). */
int zng_rocm_fold_copy_dev(int which, uint32_t adler, uint32_t crc, void *d_dst, const void *d_src,
                           size_t len, uint32_t *d_out2, void *stream);

/* combine operators, computed ON DEVICE from device-resident operands
 * (adler32.c:32-54 adler32_combine_, crc32_braid_comb.c:16-18 crc32_combine_):
 * folds `count` consecutive blocks {check[i], len[i]} left to right into one
 * checksum.  d_checks/d_lens are device arrays; d_out one uint32_t. */
int zng_rocm_adler32_combine_dev(const uint32_t *d_checks, const uint64_t *d_lens, size_t count,
                                 uint32_t *d_out, void *stream);
int zng_rocm_crc32_combine_dev(const uint32_t *d_checks, const uint64_t *d_lens, size_t count,
                               uint32_t *d_out, void *stream);

/* The same fold over packed rows {adler32, crc32, len} -- the payload the multi-GPU aggregate all-gathers
 * (one 16-byte row per rank or shard): d_out2[0] = adler32, d_out2[1] = crc32 of the
 * concatenation, rows in order.  Asynchronous on `stream`, no allocation: made to be chained behind a collective. */
typedef struct zng_rocm_check_row {
    uint32_t adler, crc;
    uint64_t len;
} zng_rocm_check_row;
int zng_rocm_combine_rows_dev(const zng_rocm_check_row *d_rows, size_t count, uint32_t *d_out2, void *stream);

/* host-side scalar forms with the reference's exact semantics
 * (zng_adler32_combine adler32.c:66-68; zng_crc32_combine/_gen/_op
 * crc32_braid_comb.c:44-54) -- used by the multi-GPU aggregate. */
uint32_t zng_rocm_adler32_combine(uint32_t adler1, uint32_t adler2, int64_t len2);
uint32_t zng_rocm_crc32_combine(uint32_t crc1, uint32_t crc2, int64_t len2);
uint32_t zng_rocm_crc32_combine_gen(int64_t len2);
uint32_t zng_rocm_crc32_combine_op(uint32_t crc1, uint32_t crc2, uint32_t op);

/* ---- deflate-side primitives on device-resident stream state -------------
 * The window/prev/head slabs of `deflate_state` (deflate.h:164-244, layout
 * deflate.c:202-264) live in HBM; one `zng_rocm_deflate_view` per stream is the
 * subset of fields the functable kernels read.  A
 * stream-level offload (DEFLATE_HOOK) marshals these from its deflate_state.
 * Every call below works on an ARRAY of views in device memory: one wavefront
 * per stream, all streams of the batch in one launch.  Field meaning is the
 * reference's. */
typedef struct zng_rocm_deflate_view {
    uint8_t  *window;            /* device; 2*w_size bytes + >= 258+8 readable padding (deflate.c:1341-1372) */
    uint16_t *prev;              /* device; w_size Pos entries */
    uint16_t *head;              /* device; 65536 Pos entries (HASH_SIZE, deflate.h:81-85) */
    uint32_t  w_size, w_mask;
    uint32_t  lookahead, strstart, match_start, prev_length;
    uint32_t  max_chain_length, good_match;
    int32_t   nice_match, level;
} zng_rocm_deflate_view;

/* slot `slide_hash` (arch/generic/slide_hash_c.c:15-52) for nstreams states: every head[] and
 * prev[] entry m becomes m >= w_size ? m - w_size : 0. */
int zng_rocm_slide_hash_dev(const zng_rocm_deflate_view *d_views, size_t nstreams, void *stream);
/* slot `compare256` (arch/generic/compare256_c.c:12-47): d_len[i] = first differing byte of
 * d_base + d_off0[i] and d_base + d_off1[i], capped at 256 (both must have 256 readable bytes). */
int zng_rocm_compare256_dev(const uint8_t *d_base, const uint64_t *d_off0, const uint64_t *d_off1, size_t npairs,
                            uint32_t *d_len, void *stream);
/* `update_hash` (insert_string.c:11-13, insert_string_tpl.h:48-51) over an array of 4-byte values */
int zng_rocm_update_hash_dev(const uint32_t *d_val, size_t n, uint32_t *d_hash, void *stream);
/* `quick_insert_string` (insert_string_tpl.h:58-75): stream i inserts position d_str[i]; d_head_out[i]
 * receives the previous chain head. */
int zng_rocm_quick_insert_string_dev(const zng_rocm_deflate_view *d_views, size_t nstreams, const uint32_t *d_str,
                                     uint16_t *d_head_out, void *stream);
/* `insert_string` (insert_string_tpl.h:85-104): stream i inserts d_count[i] consecutive positions from d_str[i],
 * in order. */
int zng_rocm_insert_string_dev(const zng_rocm_deflate_view *d_views, size_t nstreams, const uint32_t *d_str,
                               const uint32_t *d_count, void *stream);
/* The rolling-hash instantiation of the same three (insert_string_roll.c:10-24: HASH_SLIDE 5, one byte read
 * at str + 2, mask 32767), which lm_init binds for level 9 (max_chain_length > 1024, deflate.c:1223-1234).
 * The running key s->ins_h (deflate.h:196) is per stream: d_ins_h[i] is read and updated.
 * update_hash_roll: d_hash[i] = ((d_h[i] << 5) ^ (uint8_t)d_val[i]) & 32767. */
int zng_rocm_update_hash_roll_dev(const uint32_t *d_h, const uint32_t *d_val, size_t n, uint32_t *d_hash, void *stream);
int zng_rocm_quick_insert_string_roll_dev(const zng_rocm_deflate_view *d_views, size_t nstreams, const uint32_t *d_str,
                                          uint32_t *d_ins_h, uint16_t *d_head_out, void *stream);
int zng_rocm_insert_string_roll_dev(const zng_rocm_deflate_view *d_views, size_t nstreams, const uint32_t *d_str,
                                    const uint32_t *d_count, uint32_t *d_ins_h, void *stream);
/* slot `longest_match` (match_tpl.h:26-280, non-SLOW): for stream i walks the chain from d_cur_match[i];
 * d_len_out[i] = returned length, d_match_start_out[i] = s->match_start afterwards (unchanged if no
 * longer match was found). */
int zng_rocm_longest_match_dev(const zng_rocm_deflate_view *d_views, size_t nstreams, const uint16_t *d_cur_match,
                               uint32_t *d_len_out, uint32_t *d_match_start_out, void *stream);

/* slot `longest_match_slow` (match_tpl.h:26-280 with LONGEST_MATCH_SLOW; levels 7-9).  s->update_hash is the
 * multiplicative hash of insert_string.c:11-13 for levels 7-8 and the rolling one for level 9, chosen as
 * lm_init does by max_chain_length > 1024.  Same interface as zng_rocm_longest_match_dev. */
int zng_rocm_longest_match_slow_dev(const zng_rocm_deflate_view *d_views, size_t nstreams,
                                    const uint16_t *d_cur_match, uint32_t *d_len_out, uint32_t *d_match_start_out,
                                    void *stream);

/* Many messages in one pass -- the many-stream form of adler32 / crc32 (every block or stream of a pigz-style job has
 * its own check value, combined afterwards with zng_rocm_*_combine_dev): one workgroup per message up to 16 MiB, more
 * above, one set of launches for all of them.  which: 1 = Adler-32, 2 = CRC-32, 3 = both; per job the device buffer, its
 * length (< 16 GiB) and the seeds (adler32.c:11 / crc32.c semantics: 1 and 0 start a new check).  d_out2 receives two
 * words per job {adler, crc}; the word not asked for is left untouched.  Asynchronous on `stream`; jobs is a host array. */
typedef struct zng_rocm_check_job {
    const void *buf;      /* device */
    uint64_t    len;
    uint32_t    adler;    /* seed */
    uint32_t    crc;      /* seed */
} zng_rocm_check_job;
int zng_rocm_checksums_dev(int which, const zng_rocm_check_job *jobs, size_t njobs, uint32_t *d_out2, void *stream);
/* The same for a FEW LARGE messages (the outputs of a round of zng_rocm_uncompress_large_streams_dev: a dozen of 2 .. 32 MiB,
 * or one of gigabytes), where zng_rocm_checksums_dev -- the same number of workgroups for every message, one per 16 MiB and at
 * most 16 -- would leave most of the chip idle: every message is cut into 512 KiB sub-messages, ALL sub-messages go through one
 * many-message pass (one workgroup each), and one workgroup per message folds its sub-checks in order behind the message's
 * seeds (adler32_combine_ / crc32_combine_, adler32.c:32-54, crc32_braid_comb.c:16-18).  Arguments, results and limits as
 * zng_rocm_checksums_dev; one more small launch.  Asynchronous on `stream`. */
int zng_rocm_checksums_cut_dev(int which, const zng_rocm_check_job *jobs, size_t njobs, uint32_t *d_out2, void *stream);

/* ---- inflate-side copy primitive ------------------------------------------
 * slot `chunkmemset_safe` (chunkset_tpl.h:229-261) as a batch of INDEPENDENT copies inside one device
 * buffer: copy i writes out = d_base + d_out_off[i], reads from = d_base + d_from_off[i], with the
 * reference's contract on [out, out + min(len,left)): forward byte-serial copy (a distance shorter than
 * the length replicates the pattern; `from` ahead of `out` behaves like memmove).  Nothing outside that
 * range is written.  Copies of one batch must not depend on each other. */
int zng_rocm_chunkmemset_safe_dev(uint8_t *d_base, const uint64_t *d_out_off, const uint64_t *d_from_off,
                                  const uint32_t *d_len, const uint32_t *d_left, size_t ncopies, void *stream);
/* slot `chunksize` (chunkset_tpl.h:9-11): store granule of the device copy kernels (bytes). */
uint32_t zng_rocm_chunksize(void);

/* ---- whole-stream deflate on device, many independent streams (level-1 class) -------------
 * The caller this replaces is deflate_quick (deflate_quick.c:47-130) behind DEFLATE_HOOK
 * (deflate.c:1039): per job ONE static-Huffman block of raw RFC 1951, built from the same primitives
 * (insert_string hash, single chain-head probe, compare256, static trees) run wavefront-wide with the
 * head table in LDS and the bit assembly in LDS (one kernel; nothing but input and output touches HBM).
 * Output is valid deflate that any inflater restores to the input; it is not bit-identical to the
 * reference's stream.
 *   in:  device; any alignment; `dict_len` (<= 32768) bytes of history sit directly in front of it
 *        (in - dict_len .. in): they prime the hash as deflateSetDictionary does (deflate.c:456-531) and
 *        matches may reach back into them, but they are neither emitted nor part of the checksum
 *   out: device, 4-byte aligned, out_cap >= zng_rocm_deflate_quick_bound(in_len).  out_cap is 32 bits wide, so ONE stream is at
 *        most 3 817 748 681 bytes (3.55 GiB), the largest in_len whose bound is at most 0xffffffff; a longer one is
 *        ZNG_ROCM_EINVAL.  Up to there a stream's output bits (up to 8 * 2^32) and its check row are exact
 *        (csrc/deflate_quick_plan.h)
 *   flags: 0 = the block is the stream's last (BFINAL = 1: what one deflate(Z_FINISH) call emits);
 *        ZNG_ROCM_BLOCK_NOT_FINAL = BFINAL 0; with ZNG_ROCM_BLOCK_SYNC_FLUSH an empty stored block follows
 *        (00 00 ff ff after the padding bits: the Z_SYNC_FLUSH marker, deflate.c:1064-1076), so the job's
 *        output is a whole number of bytes and jobs CONCATENATE into one valid stream -- the pigz scheme:
 *        blocks of one input compressed independently, each primed with the 32 KiB before it.
 * `jobs` is a HOST array (copied internally).  d_results (device) receives per job
 * {compressed length, adler32(1, in, in_len)} -- the {clen, check} row of the multi-stream table. */
#define ZNG_ROCM_BLOCK_NOT_FINAL  1u
#define ZNG_ROCM_BLOCK_SYNC_FLUSH 2u
typedef struct zng_rocm_stream_job {
    const uint8_t *in;
    uint8_t       *out;
    uint32_t       in_len;
    uint32_t       out_cap;
    uint32_t       dict_len;
    uint32_t       flags;
} zng_rocm_stream_job;
size_t zng_rocm_deflate_quick_bound(size_t source_len);
int    zng_rocm_deflate_quick_dev(const zng_rocm_stream_job *jobs, size_t njobs, uint32_t *d_results, void *stream);

/* ---- whole-stream deflate on device, ONE large stream (chain-walking levels) -----------------
 * The caller this replaces is deflate_medium (deflate_medium.c:145-277) + zng_tr_flush_block's
 * dynamic-tree block (trees.c:625-741) behind DEFLATE_HOOK.  The plaintext is device resident and
 * complete, so it is compressed as parallel 128-512 KiB segments (hash primed with the preceding 32 KiB,
 * so matches cross segment borders) into one continuous raw RFC 1951 stream: per segment one block whose
 * type is chosen as zng_tr_flush_block does (stored / static / dynamic, trees.c:660-719), followed by an
 * empty stored block where byte alignment needs it (as Z_SYNC_FLUSH), and a final empty static block.
 * `level` 2..9 selects max_chain_length and good_match as deflate.c:142-168 does (chain capped at 256); level 1 is
 * deflate_quick's matcher (one probe of the chain head, deflate_quick.c:89-97) on the same segment scheme; level 0
 * is deflate_stored (deflate_stored.c:27-186): stored blocks of MAX_STORED = 65535 bytes, the last one final -- the
 * split that function makes when input and output are both complete (:46-95).  d_out needs
 * zng_rocm_deflate_bound(in_len) bytes.
 * Synchronises `stream` (the segment lengths are prefix-summed on the host).  Returns 0, a ZNG_ROCM_E* code, or
 * -5 (Z_BUF_ERROR).
 * zng_rocm_deflate_block_dev is the same for one BLOCK of a longer stream: `dict_len` (<= 32768) bytes of history
 * in front of d_in prime the first segment, and `flags` (ZNG_ROCM_BLOCK_*, above) say whether the stream ends
 * here; a non-final block always ends byte aligned behind an empty stored block.
 * d_in and d_out: no alignment is asked of either, here and in the async, streams, strategy and window forms below (the
 * blocks are built in 4-byte aligned scratch of the library's own and packed into d_out by bytes; level 0 writes its headers
 * and payload with stores that take any address).  Of d_in, only [d_in - dict_len, d_in + in_len) is read; no byte outside
 * [d_out, d_out + out_cap) is written. */
size_t zng_rocm_deflate_bound(size_t source_len);
int    zng_rocm_deflate_dev(int level, const uint8_t *d_in, size_t in_len, uint8_t *d_out, size_t out_cap,
                            size_t *out_len, void *stream);
/* as zng_rocm_deflate_block_dev for levels 1..9, without any synchronisation: every step (matcher, block emitter, the scan that
 * places the segments, the packing) is enqueued on `stream`; d_result (device, 2 x uint64) = {compressed size, 1 if it
 * did not fit out_cap} once the stream has got there */
int    zng_rocm_deflate_async_dev(int level, const uint8_t *d_in, size_t in_len, uint32_t dict_len, uint32_t flags,
                                  uint8_t *d_out, size_t out_cap, uint64_t *d_result, void *stream);
int    zng_rocm_deflate_block_dev(int level, const uint8_t *d_in, size_t in_len, uint32_t dict_len, uint32_t flags,
                                  uint8_t *d_out, size_t out_cap, size_t *out_len, void *stream);
/* Many independent streams (or independent blocks of one input) at one of the chain levels 1..9 -- the reference's
 * many-stream model (test/pigz/CMakeLists.txt:123-200) at pigz's default level: the segments of ALL streams go through
 * one set of launches per ~1 GiB of plaintext.  Per job as zng_rocm_deflate_block_dev (dict_len bytes of history in
 * front of `in`, ZNG_ROCM_BLOCK_* flags, out_cap >= zng_rocm_deflate_bound(in_len)); synchronous; out_lens[i] (host) =
 * compressed size of stream i.  The level-1 CLASS (static Huffman, one kernel) is zng_rocm_deflate_quick_dev. */
int    zng_rocm_deflate_streams_dev(int level, const zng_rocm_stream_job *jobs, size_t njobs, size_t *out_lens,
                                    void *stream);
/* The same two with zlib's `strategy` (deflateInit2; zlib-ng.h.in codes): 0 Z_DEFAULT_STRATEGY and 1 Z_FILTERED give
 * exactly the bytes of the calls above; anything outside 0..4 returns ZNG_ROCM_EINVAL with nothing launched or written.
 * As deflate.c:1039-1043 chooses:
 *   level 0            stored blocks, whatever the strategy;
 *   2 Z_HUFFMAN_ONLY   every byte a literal (deflate_huff.c:16-45); the level makes no difference;
 *   3 Z_RLE            the greedy parse of deflate_rle.c:30-86 run on every device segment: p is a match iff
 *                      in[p-1] == in[p] == in[p+1] == in[p+2] and p + 3 <= the segment's end, of distance 1 and of the
 *                      length of the run of in[p-1] from p on (at most 258, not past the segment's end); in[p-1] may lie
 *                      in the previous segment or in the dict_len history; the level makes no difference;
 *   4 Z_FIXED          the level's matcher; each block stored if that is not larger than static, otherwise static
 *                      (trees.c:660-672 with opt_lenb = static_lenb): never a dynamic block.
 * The blocks are valid raw RFC 1951, not bit-identical to the reference's (their boundaries differ);
 * zng_rocm_deflate_bound(in_len) holds for every strategy. */
int    zng_rocm_deflate_strategy_block_dev(int level, int strategy, const uint8_t *d_in, size_t in_len, uint32_t dict_len,
                                           uint32_t flags, uint8_t *d_out, size_t out_cap, size_t *out_len, void *stream);
int    zng_rocm_deflate_strategy_streams_dev(int level, int strategy, const zng_rocm_stream_job *jobs, size_t njobs,
                                             size_t *out_lens, void *stream);
/* The same two with deflateInit2's `windowBits`: the stream is one that a reader with a window of 1 << window_bits bytes can
 * decode.  For such a reader a distance above its window is a hard error ("invalid distance too far back"), not a loss of ratio.
 *   range     window_bits is 9..15 (deflate.c:317-318); anything else returns ZNG_ROCM_EINVAL with nothing launched or written.
 *             8 exists for the zlib wrapper alone (deflate.c:319) and these raw calls have no format: they refuse it.
 *   cap       no match reaches further back than MAX_DIST(s) = (1 << window_bits) - 262 (deflate.h:410-415): 250, 762, 1786, 3834,
 *             7930, 16122 for 9..14.  The level's matcher runs in its window form (lz_rows_win_kernel: the cap and the priming
 *             length are arguments; a segment enters the 1 << window_bits bytes in front of itself, nothing further back can be
 *             referenced).  Z_RLE, Z_HUFFMAN_ONLY and level 0 write distance 1 or none and give the bytes they give at 15;
 *             Z_FIXED uses the window form of the matcher.
 *   15        exactly the bytes of the calls above, through the kernel they have always run (deflate.c:345: w_size 32768).
 *   history   dict_len up to 32768 is still accepted; history further back than the cap is never referenced (deflate.c:479-484
 *             keeps the last w_size bytes of a dictionary; what lies in front of them cannot be reached either way).
 *   bound     zng_rocm_deflate_bound(in_len) holds at every window: the emitter stores a block whenever that is not larger
 *             (trees.c:660-672), so fewer matches never cost more than the stored form the bound covers. */
int    zng_rocm_deflate_window_block_dev(int level, int strategy, int window_bits, const uint8_t *d_in, size_t in_len,
                                         uint32_t dict_len, uint32_t flags, uint8_t *d_out, size_t out_cap, size_t *out_len,
                                         void *stream);
int    zng_rocm_deflate_window_streams_dev(int level, int strategy, int window_bits, const zng_rocm_stream_job *jobs, size_t njobs,
                                           size_t *out_lens, void *stream);

/* ---- inflate: host bitstream decode -> token stream -> device copy resolution -------------
 * The split of slot `inflate_fast` (inffast_tpl.h:53-318): the sequential Huffman decode loop
 * (:151-226) runs on the host and emits TOKENS instead of stores; the literal stores and match
 * copies (:155-171, :228-279 CHUNKCOPY / CHUNKMEMSET / chunkcopy_safe) are resolved on the
 * device, all segments in parallel.
 *   token (uint32): bit31 = 0 -> run of `tok` literals, taken in order from `literals`
 *                   bit31 = 1 -> match: length = ((tok >> 16) & 0xff) + 3, distance = (tok & 0xffff) + 1
 *   segs: (nsegs + 1) triples {first token, first output byte, first literal}; every segment but
 *         the last holds >= 32 KiB (and < 32 KiB + 258) of output, so a match never reaches
 *         further back than the previous segment.
 * status / msg follow zlib: 1 = Z_STREAM_END, -3 = Z_DATA_ERROR with the reference's strm->msg text
 * (inflate.c:735-917, inffast_tpl.h:189-226), -5 = input ended early, -4 = out of memory.  On an
 * error the tokens describe everything decoded before the bad symbol. */
typedef struct zng_rocm_inflate_tokens {
    uint32_t   *tokens;    size_t ntokens;
    uint8_t    *literals;  size_t nliterals;
    uint64_t   *segs;      size_t nsegs;
    uint64_t    out_len;
    size_t      in_used;
    int         status;
    const char *msg;
} zng_rocm_inflate_tokens;

int  zng_rocm_inflate_tokens_decode(const uint8_t *src, size_t src_len, zng_rocm_inflate_tokens *out);
/* the same for a stream that continues history: `window_len` (<= 32768) bytes precede its first byte -- a preset
 * dictionary (inflateSetDictionary on a raw stream, inflate.c:1214-1261) or the last bytes an earlier call produced
 * (inflate's sliding window, inflate.c:325-378) -- so a distance may reach that far beyond the start of the output
 * before it is "invalid distance too far back" (inffast_tpl.h:198-226 with whave = window_len) */
int  zng_rocm_inflate_tokens_decode_window(const uint8_t *src, size_t src_len, uint32_t window_len,
                                           zng_rocm_inflate_tokens *out);
/* Every COMPLETE block of a raw stream from bit `start_bit` of src on (a block header starts there), continuing
 * `window_len` bytes of history.  1 = the BFINAL block was decoded, *end_bit = first bit behind it; 0 = the input ends
 * inside a block: the tokens describe every block that ended inside src, *end_bit = the bit where the first incomplete
 * block starts (== start_bit when none completed); -3 = Z_DATA_ERROR with the reference's text in out->msg, the tokens
 * describe the complete blocks before the failing one, *end_bit = its start; -4 = out of memory.  `out` is zeroed and
 * *end_bit = start_bit on every return, ZNG_ROCM_EINVAL (a refused argument, e.g. start_bit beyond 8 * src_len) included;
 * out->msg is set on a data error only.  The streaming form of
 * inflate's TYPEDO (inflate.c:728): what a Z_SYNC_FLUSH promises the decompressor, it gets. */
int  zng_rocm_inflate_tokens_decode_blocks(const uint8_t *src, size_t src_len, uint64_t start_bit, uint32_t window_len,
                                           zng_rocm_inflate_tokens *out, uint64_t *end_bit);
void zng_rocm_inflate_tokens_free(zng_rocm_inflate_tokens *t);
/* Device stage on device-resident token arrays.  d_symbols: workspace of out_len uint16_t;
 * d_out: out_len bytes.  Up to four launches: per-segment resolution into 16-bit symbols (a symbol
 * >= 256 names a byte of the previous segment's last 32 KiB), the context chain over those 32 KiB
 * tails in two levels, and the final translate.  `segs` must keep the >= 32 KiB-per-segment rule
 * above (zng_rocm_inflate_tokens_decode does). */
int  zng_rocm_inflate_resolve_dev(const uint32_t *d_tokens, size_t ntokens, const uint8_t *d_literals,
                                  size_t nliterals, const uint64_t *d_segs, size_t nsegs, uint16_t *d_symbols,
                                  uint8_t *d_out, uint64_t out_len, void *stream);
/* ... and on `nthreads` host threads (<= 0: one per hardware thread, capped by the control group's CPU quota): the compressed bytes are cut into parts, each
 * thread finds a block boundary in its part (a valid dynamic block header or a sync-flush marker) and decodes from
 * there; the parts are then chained from bit 0 and joined.  Same token stream semantics, status and messages as the
 * one-thread decoder (irregular streams are simply handed to it); streams without findable boundaries (all blocks
 * fixed-Huffman or stored) decode on one thread. */
int  zng_rocm_inflate_tokens_decode_threads(const uint8_t *src, size_t src_len, uint32_t window_len, int nthreads,
                                            zng_rocm_inflate_tokens *out);
/* how many parts the calling thread's last multi-threaded decode was joined from (0 = the one-thread decoder did it) */
int  zng_rocm_inflate_threads_last_parts(void);
/* resolve with a prior window: `d_window` holds the window_len bytes that precede the stream (device);
 * d_symbols must then have room for 32768 + out_len uint16_t (the window's symbols are laid in front) */
int  zng_rocm_inflate_resolve_window_dev(const uint32_t *d_tokens, size_t ntokens, const uint8_t *d_literals,
                                         size_t nliterals, const uint64_t *d_segs, size_t nsegs, uint16_t *d_symbols,
                                         uint8_t *d_out, uint64_t out_len, const uint8_t *d_window,
                                         uint32_t window_len, void *stream);
/* One-shot raw inflate (windowBits < 0): host stream in, plaintext left in device memory at d_dst.
 * Returns the zlib status of the decode (1 = Z_STREAM_END) or a negative ZNG_ROCM_E* / Z_* code;
 * *out_len = bytes produced.  -5 also when dst_cap is too small.  A stream of 4 MiB and more is copied to the device and
 * decoded there (as zng_rocm_inflate_large_dev; zng_rocm_inflate_large_last_parts() tells); anything irregular, and every
 * smaller stream, is decoded on the calling thread (zng_rocm_inflate_tokens_decode) and resolved on the device. */
int  zng_rocm_inflate_raw(const uint8_t *src, size_t src_len, uint8_t *d_dst, size_t dst_cap, uint64_t *out_len,
                          void *stream);

/* as zng_rocm_inflate_raw, also reporting how many input bytes the deflate stream occupied */
int  zng_rocm_inflate_raw_ex(const uint8_t *src, size_t src_len, uint8_t *d_dst, size_t dst_cap, uint64_t *out_len,
                             size_t *in_used, void *stream);

/* ... and of a stream that continues `window_len` bytes of device-resident history (dictionary / sliding window) */
int  zng_rocm_inflate_raw_window(const uint8_t *src, size_t src_len, const uint8_t *d_window, uint32_t window_len,
                                 uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, size_t *in_used, void *stream);

/* ONE large raw stream that is ALREADY in device memory, inflated on the device: block starts are found on the device
 * (dynamic headers the decoder would accept, sync-flush markers, byte-aligned stored blocks), the stream is cut there into parts, one
 * wavefront decodes each part into 16-bit symbols (inffast_tpl.h:151-298 with the history still unknown), the parts are
 * chained from bit 0 and the context chain of zng_rocm_inflate_resolve_dev turns the symbols into bytes.  The host only
 * sorts a few thousand candidates and walks the chain.  Streams that offer nothing to cut at (fixed-Huffman blocks
 * only) and every irregular stream go to the sequential decoder, so status and message are always the
 * reference's.  Returns as zng_rocm_inflate_raw_window; synchronous. */
int  zng_rocm_inflate_large_dev(const uint8_t *d_src, size_t src_len, const uint8_t *d_window, uint32_t window_len,
                                uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, size_t *in_used, void *stream);
/* parts on the chain of the calling thread's last zng_rocm_inflate_large_dev or zng_rocm_inflate_raw* call (0: the
 * sequential decoder did it) */
int  zng_rocm_inflate_large_last_parts(void);

/* zng_rocm_inflate_large_ex_dev flags */
#define ZNG_ROCM_INFLATE_SUBBLOCK 1u   /* parts may also begin INSIDE a block */
/* zng_rocm_inflate_large_dev with flags.  flags == 0 is exactly zng_rocm_inflate_large_dev (same path, bytes, status, part
 * count).  ZNG_ROCM_INFLATE_SUBBLOCK also cuts the stream inside blocks, which is what a stream of fixed-Huffman blocks
 * (level-1 class writers, Z_FIXED, zng_rocm_deflate_quick_dev) needs to be decoded in parts at all, and what evens out a
 * foreign stream whose blocks expand very unequally.  Guesses are placed in the stretches between the block starts found;
 * a dry parse of 128 symbols from each (with the fixed codes, or the tables of the dynamic header the stretch begins with)
 * gives a bit B on the symbol grid of that block.  A part hands off at B only when it is decoding a block of the same
 * identity (fixed codes; or the dynamic block with that header), stands at a symbol boundary and its bit position is
 * exactly B: the part from B then decodes what the stream has there (inffast_tpl.h:151-298 from B on; the headers around
 * it inflate.c:735-917).  A part that began inside a fixed-code block does not know that block's BFINAL; the part in front
 * of it does, and when it is set the stream ends at the first end of block behind B (so *in_used is the reference's
 * also with bytes behind the stream).  Everything irregular goes to the sequential decoder as in zng_rocm_inflate_large_dev.
 * Unknown flag bits return ZNG_ROCM_EINVAL with nothing launched or written to d_dst; that value equals Z_DATA_ERROR, and
 * such a refusal is told apart by *out_len = *in_used = 0 and zng_rocm_last_error() naming the flag bits (a data error
 * of the stream says the reference's message instead).  Synchronous. */
int  zng_rocm_inflate_large_ex_dev(const uint8_t *d_src, size_t src_len, const uint8_t *d_window, uint32_t window_len,
                                   uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, size_t *in_used, uint32_t flags,
                                   void *stream);
/* of the parts on the calling thread's last chain, how many began inside a block (0: none did, or the sequential decoder
 * did the work); thread-local like zng_rocm_inflate_large_last_parts */
int  zng_rocm_inflate_large_last_subparts(void);
/* how many sub-starts (bit positions inside blocks, after the dry parse) the calling thread's last
 * ZNG_ROCM_INFLATE_SUBBLOCK call placed, whether or not the sequential decoder did the work in the end; with
 * zng_rocm_inflate_large_last_subparts() it gives the share that a genuine decode landed on */
int  zng_rocm_inflate_large_last_substarts(void);
/* zng_rocm_inflate_large_ex_dev piece by piece: the same arguments, flags (0 or ZNG_ROCM_INFLATE_SUBBLOCK) and results,
 * for a stream of any length (src_len and the output may pass 4 GiB), with device scratch that does not grow with it.
 * The stream is decoded in device passes over pieces of at most `piece_bytes` compressed bytes (0 = 64 MiB; otherwise
 * 4 MiB .. 1 GiB).  A pass that does not reach the stream's end delivers the parts in front of the first one that ran out of
 * the piece's input, and the next piece begins exactly where that part began (a block start, or with
 * ZNG_ROCM_INFLATE_SUBBLOCK a start inside a block that the part in front landed on).  Each pass has the 32 KiB in front
 * of its output as history (the caller's window spliced with d_dst while fewer bytes were produced).  A piece the device
 * cannot do -- no start behind its own is landed on, a data error, a truncated end -- goes to the sequential decoder
 * from the last block start delivered: complete blocks, behind which the device goes on; a data error or the end of the
 * input is decoded there once more in the stream form.  So for every stream zng_rocm_inflate_large_ex_dev accepts with a
 * dst_cap that holds the output, the return value, *out_len, *in_used, the bytes at d_dst[0, *out_len) and the
 * zng_rocm_last_error() text of a data error are the same.
 * dst_cap too small: -5, nothing written at or beyond d_dst + dst_cap; *out_len is the output decoded until then, more than
 * dst_cap but possibly less than the whole stream's (which zng_rocm_inflate_large_ex_dev reports), *in_used where it ended.
 * Scratch: the device bytes the call adds to the workspace of `stream` (zng_rocm_workspace_bytes) are at most
 * 256 x piece_bytes + 640 MiB, whatever src_len is; a pass over scratch caps is run again on half the piece, down to 4 MiB.
 * Unknown flag bits or a piece_bytes outside 4 MiB .. 1 GiB return ZNG_ROCM_EINVAL with nothing launched or written and
 * *out_len = *in_used = 0.  The part counters (last_parts / _subparts / _substarts) are sums over the pieces.
 * Synchronous. */
int  zng_rocm_inflate_large_pieces_dev(const uint8_t *d_src, size_t src_len, const uint8_t *d_window, uint32_t window_len,
                                       uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, size_t *in_used, size_t piece_bytes,
                                       uint32_t flags, void *stream);
/* device passes of the calling thread's last zng_rocm_inflate_large_pieces_dev call */
int  zng_rocm_inflate_large_last_pieces(void);
/* compressed bytes of the calling thread's last zng_rocm_inflate_large_pieces_dev call that the sequential decoder took */
uint64_t zng_rocm_inflate_large_last_host_bytes(void);

/* MANY large raw streams that are already in device memory, in one set of launches: what zng_rocm_inflate_large_ex_dev
 * does for one stream -- finder, parts, chain, compaction, resolve -- runs once per ROUND over the parts of all the round's
 * streams, so that the long parts of one stream run under the short parts of the others and the host round trips between
 * the kernels are paid per round, not per stream (a shard set of a few to a few hundred streams of 1 .. 64 MiB each).
 * Per job, on return: `status` as the return value of zng_rocm_inflate_large_ex_dev for this job alone (1 = Z_STREAM_END,
 * -3 with the reference's text in `msg`, -5 input ended early or dst_cap too small -- then nothing is written at or behind
 * d_dst + dst_cap --, negative ZNG_ROCM_E*), `out_len` / `in_used` as there, and on status 1 the same bytes at
 * d_dst[0, out_len).  `parts` = parts of this job on its chain (0: the sequential decoder did it), `subparts` = of them,
 * parts that began inside a block.  A job the device path cannot do (below 128 KiB or from 2 GiB on, fewer than four starts,
 * anything irregular on its chain) leaves its round and is decoded as zng_rocm_inflate_large_ex_dev decodes it (host copy,
 * sequential decoder) behind the round's device work; the round's other jobs do not notice.
 * Rounds: jobs are taken in order until their compressed bytes would pass `round_bytes` (0 = 256 MiB; otherwise 4 MiB up
 * to, not including, 2 GiB) or their parts 65535; a job larger than round_bytes is a round of its own.  Rounds run one
 * after the other; device scratch (zng_rocm_workspace_bytes of `stream`) is sized by the largest round: 128 bytes of part
 * slots per compressed byte plus slack, 2 bytes of symbols per output byte plus 64 KiB per stream.  Per round the call
 * synchronises a fixed number of times, whatever the number of streams in it.
 * flags: 0 or ZNG_ROCM_INFLATE_SUBBLOCK, as for zng_rocm_inflate_large_ex_dev (the guess step is derived from the round's
 * bits).  Unknown flag bits, a window_len above 32768, a null buffer with a non-zero length or a round_bytes outside the
 * range return ZNG_ROCM_EINVAL with nothing launched and nothing written to any job's output fields or d_dst.
 * Synchronous.  Returns 0 or the first device error; a stream's own trouble is its job's status alone. */
typedef struct zng_rocm_inflate_large_job {
    const uint8_t *d_src;     size_t   src_len;      /* device: raw deflate stream */
    const uint8_t *d_window;  uint32_t window_len;   /* device: <= 32768 bytes of history, or NULL / 0 */
    uint8_t       *d_dst;     size_t   dst_cap;      /* device: plaintext */
    /* out */
    int            status;
    uint64_t       out_len;
    size_t         in_used;
    const char    *msg;       /* reference's strm->msg text on a data error, else NULL (static storage) */
    uint32_t       parts;
    uint32_t       subparts;
} zng_rocm_inflate_large_job;
int  zng_rocm_inflate_large_streams_dev(zng_rocm_inflate_large_job *jobs, size_t njobs, size_t round_bytes, uint32_t flags,
                                        void *stream);
/* rounds of the calling thread's last zng_rocm_inflate_large_streams_dev call (thread-local, like the other last_* counters) */
int  zng_rocm_inflate_large_last_rounds(void);
/* part-kernel launches of that call, reruns of overflowed parts included: at most two per round */
int  zng_rocm_inflate_large_last_part_launches(void);

/* Many independent raw streams at once: `nthreads` host threads (<= 0: as many as the host gives us) take the jobs in
 * order, each decoding on the host and resolving on the device on its own HIP stream, so that the sequential decode
 * -- where an inflate spends its time -- runs on all the cores the caller allows while the device work of one stream
 * overlaps the decode of the next (the pigz shape: test/pigz/CMakeLists.txt).  Per job: `src` host, `d_dst` device
 * (dst_cap bytes), an optional device-resident window / dictionary in front (as zng_rocm_inflate_raw_window); on
 * return `status` is the job's zlib status (1 = Z_STREAM_END, -3 with the reference's text in `msg`, -5 input ended
 * early or destination too small, negative ZNG_ROCM_E*), `out_len` / `in_used` as in the one-shot call.  Synchronous:
 * every plaintext is in place when the call returns.  The return value is 0 or the first device error. */
typedef struct zng_rocm_inflate_job {
    const uint8_t *src;       size_t   src_len;
    uint8_t       *d_dst;     size_t   dst_cap;
    const uint8_t *d_window;  uint32_t window_len;
    int            status;
    uint64_t       out_len;
    size_t         in_used;
    const char    *msg;
} zng_rocm_inflate_job;
int  zng_rocm_inflate_many(zng_rocm_inflate_job *jobs, size_t njobs, int nthreads);

/* Many independent raw deflate streams that are ALREADY in device memory, decoded entirely on the device: one wavefront
 * per stream runs slot `inflate_fast` (inffast_tpl.h:53-318) and the block decoding around it (inflate.c:735-917,
 * inftrees.c:32-297) -- Huffman decode and copies -- with the last 4 KiB of output in an LDS ring (inflate's sliding
 * window, inflate.c:325-378).  The inverse of zng_rocm_deflate_quick_dev for the reference's many-stream model
 * (test/pigz/CMakeLists.txt:123-200): nothing crosses PCIe.  `dict_len` bytes of history (a dictionary,
 * inflateSetDictionary on a raw stream inflate.c:1214-1261, or the previous window) must sit directly in front of `out`.
 * Asynchronous on `stream`; jobs is a host array (copied before the call returns).  The compressed words are fetched as
 * aligned dwords: up to 3 bytes on either side of [in, in + in_len) inside the same 4-byte words are read (never used).
 * d_results: 4 uint32 per job: {bytes produced, input bytes consumed, status as int32 (1 = Z_STREAM_END, -3 = Z_DATA_ERROR,
 * -5 = Z_BUF_ERROR: input ended early or out_cap too small), message id for zng_rocm_inflate_message}. */
typedef struct zng_rocm_inflate_dev_job {
    const void *in;        /* device: raw deflate stream */
    void       *out;       /* device: plaintext */
    uint64_t    in_len;    /* < 2 GiB */
    uint64_t    out_cap;   /* < 2 GiB */
    uint32_t    dict_len;  /* <= 32768 */
    uint32_t    flags;     /* 0 */
} zng_rocm_inflate_dev_job;
int  zng_rocm_inflate_streams_dev(const zng_rocm_inflate_dev_job *jobs, size_t njobs, uint32_t *d_results, void *stream);
/* the reference's strm->msg text for a message id of d_results ("" for 0 / unknown ids) */
const char *zng_rocm_inflate_message(uint32_t id);

/* zlib (format 1) / gzip (format 2) / raw (format 0) framing for MANY device-resident streams -- compress2 / uncompress2
 * (compress.c:31-69, uncompr.c:25-76) in the shape of the many-stream model, every step on the device, asynchronous on
 * `stream`:
 *   compress: the level-1 class per stream + (gzip) the CRC-32 of every plaintext in one pass + one kernel that writes
 *   every header and trailer.  Both wrappers are 12 bytes long so that the block starts 4-byte aligned: gzip declares an
 *   empty FEXTRA field, zlib puts two empty stored blocks behind its 2-byte header.  Per job: out 4-byte aligned,
 *   out_cap >= zng_rocm_compress_streams_bound(in_len, format), no dictionary / flags for a wrapped stream.
 *   d_results: 2 words per job {total bytes written, check value (Adler-32; gzip: CRC-32)}.
 *   uncompress: every header parsed on the device (inflate.c:509-555, :556-700 incl. FHCRC), zng_rocm_inflate_streams_dev's
 *   kernel, the check values of all outputs in one many-message pass whose descriptors are filled on the device, every
 *   trailer compared (inflate.c:1105-1147).  d_results: 4 words per job as zng_rocm_inflate_streams_dev, bytes consumed
 *   counting header and trailer; message ids include "incorrect header check", "unknown compression method", "invalid
 *   window size", "header crc mismatch", "need dictionary", "incorrect data check", "incorrect length check".  This call
 *   holds no dictionary, so a zlib member with FDICT is "need dictionary" (-3; uncompr.c:70-75);
 *   zng_rocm_uncompress_streams_dict_dev below is the call that reads such members.
 * Levels 0..9, every strategy and canonical wrappers for a batch: zng_rocm_compress_streams2_dev / _members_dev below. */
size_t zng_rocm_compress_streams_bound(size_t source_len, int format);
int  zng_rocm_compress_streams_dev(int format, const zng_rocm_stream_job *jobs, size_t njobs, uint32_t *d_results, void *stream);
int  zng_rocm_uncompress_streams_dev(int format, const zng_rocm_inflate_dev_job *jobs, size_t njobs, uint32_t *d_results,
                                     void *stream);

/* Many wrapped streams at EVERY level and strategy -- compress2 (compress.c:31-69) / deflateInit2 + deflate(Z_FINISH) over a whole
 * batch, in place or as one file.  Asynchronous on `stream`: no host synchronisation and no device-to-host copy inside the
 * calls; the result words are valid once the stream has got there.  (With more than one round the host waits, between rounds,
 * for the upload of the round before's segment table -- an event, not the stream.)
 *   format       0 raw, 1 zlib, 2 gzip
 *   level        -1 (= 6, deflate.c:296) or 0..9
 *   strategy     0..4 as zng_rocm_deflate_strategy_streams_dev
 *   jobs         HOST array (copied internally); in / in_len / dict_len / flags as zng_rocm_deflate_block_dev; a wrapped format
 *                takes neither dict_len nor flags; no alignment is asked of in or out
 *   round_bytes  plaintext per round (one set of launches); 0 = 4 GiB; a job is never split, so a round has at least one job
 * The members are canonical (no padding, unlike the 12-byte wrappers of zng_rocm_compress_streams_dev):
 *   zlib   CMF FLG with FLEVEL as deflate.c:868-885 sets it (0 for strategy >= Z_HUFFMAN_ONLY or level < 2) | data | Adler-32,
 *          most significant byte first (deflate.c:1098-1101)
 *   gzip   the 10 bytes of deflate.c:902-913 -- no name, no extra field, mtime 0, XFL by the same rule (:911-912), OS 3 | data |
 *          CRC-32, ISIZE, little endian (deflate.c:1091-1096)
 *   data   levels 1..9: exactly the bytes zng_rocm_deflate_strategy_streams_dev writes for the same job list, level and
 *          strategy (the segment size is chosen once from the call's whole plaintext); level 0: exactly the bytes
 *          zng_rocm_deflate_strategy_block_dev writes per job at level 0 (deflate_stored.c:46-95: stored blocks of 65535 bytes)
 * Check values: Adler-32 for formats 0 and 1, CRC-32 for format 2, of every plaintext in one many-message pass per round.
 * Refused with ZNG_ROCM_EINVAL before anything is launched or written: format / level / strategy out of range, a null pointer,
 * dict_len > 32768, flags other than ZNG_ROCM_BLOCK_*, dict_len or flags in a wrapped format, a job whose
 * zng_rocm_compress_bound(in_len, format) does not fit 32 bits.  njobs == 0 returns 0.
 *
 * zng_rocm_compress_streams2_dev: member i goes to jobs[i].out, out_cap >= zng_rocm_compress_streams2_bound(in_len, format)
 *   (= zng_rocm_compress_bound; a smaller one returns -5 with nothing launched).  d_results (device): 2 words per job {bytes
 *   written, check value}, as zng_rocm_compress_streams_dev.
 * zng_rocm_compress_members_dev: the members stand back to back in d_dst -- for gzip the multi-member file of RFC 1952 2.2 (what
 *   `cat a.gz b.gz` makes and zng_rocm_gunzip_members_dev reads); out / out_cap of the jobs are not looked at.  d_offsets
 *   (device, njobs + 1): d_offsets[i] = first byte of member i, d_offsets[njobs] = the file's length.  A length above dst_cap
 *   means the file did not fit: then no byte at or behind d_dst + dst_cap is written and the bytes in front of it are those of
 *   the file that fits.  d_checks (device, njobs, may be NULL): the check values.
 * zng_rocm_compress_streams2_last_rounds: rounds of the calling thread's last call of either. */
size_t zng_rocm_compress_streams2_bound(size_t source_len, int format);
int    zng_rocm_compress_streams2_dev(int format, int level, int strategy, const zng_rocm_stream_job *jobs, size_t njobs,
                                      size_t round_bytes, uint32_t *d_results, void *stream);
int    zng_rocm_compress_members_dev(int format, int level, int strategy, const zng_rocm_stream_job *jobs, size_t njobs,
                                     uint8_t *d_dst, size_t dst_cap, size_t round_bytes, uint64_t *d_offsets, uint32_t *d_checks,
                                     void *stream);
int    zng_rocm_compress_streams2_last_rounds(void);
/* The two calls above with deflateInit2's `windowBits`, as zng_rocm_deflate_window_streams_dev:
 *   window_bits  9..15; 8 is accepted for format 1 alone and taken as 9 (deflate.c:319, :322-323: "until 256-byte window bug
 *                fixed"), so it gives the whole member 9 gives; formats 0 and 2 refuse it.  Anything else: ZNG_ROCM_EINVAL with
 *                nothing launched or written.
 *   zlib         CMF = 8 + ((window_bits - 8) << 4), FLEVEL by the rule above, FCHECK over the new CMF (deflate.c:870-885): 0x18..
 *                for 9, 0x28.. for 10, ... 0x78.. for 15.  A reader opened with a smaller window answers "invalid window size"
 *                (inflate.c:541-546).
 *   gzip         has no window field (deflate.c:902-913): only the distances change.
 *   data         levels 1..9: exactly the bytes zng_rocm_deflate_window_streams_dev writes for the same job list; level 0 as ever.
 *   15           exactly the bytes of the calls above.
 * Bounds, results, offsets, rounds and every other refusal are those of the calls above; zng_rocm_compress_streams2_bound holds
 * at every window because the emitter stores a block whenever that is not larger (trees.c:660-672). */
int    zng_rocm_compress_streams2_window_dev(int format, int level, int strategy, int window_bits, const zng_rocm_stream_job *jobs,
                                             size_t njobs, size_t round_bytes, uint32_t *d_results, void *stream);
int    zng_rocm_compress_members_window_dev(int format, int level, int strategy, int window_bits, const zng_rocm_stream_job *jobs,
                                            size_t njobs, uint8_t *d_dst, size_t dst_cap, size_t round_bytes, uint64_t *d_offsets,
                                            uint32_t *d_checks, void *stream);

/* ---- one preset dictionary shared by many small device-resident streams -----------------------------------------------
 * deflateSetDictionary / inflateSetDictionary (deflate.c:456-512, inflate.c:1234-1260) for the many-stream calls above.  The
 * reference amortises a dictionary with one primed state that is deflateCopy'd per message; here the dictionary is prepared
 * ONCE on the device as an object, and a whole batch of messages -- records, pages, RPC payloads -- is compressed or restored
 * against it in one set of launches, with no copy of the dictionary in front of any buffer.
 *
 * zng_rocm_dict_create_dev: d_dict is device memory, dict_len >= 1 (NULL or 0: ZNG_ROCM_EINVAL, *out = NULL).  The call
 *   - computes the DICTID, the Adler-32 of ALL dict_len bytes (deflate.c:470-471), with the streaming checksum kernel;
 *   - copies the last W = min(dict_len, 32768) bytes into memory the object owns (the tail rule, deflate.c:477-486; d_dict
 *     may be freed afterwards), zero padded so that the matcher's probes stay inside -- the padding never lengthens a match;
 *   - builds the primed head table of the level-1 class: for every bucket the last position p with p + 4 <= W whose four
 *     bytes hash there, + 1 (the last 3 positions are left out, deflate.c:494-501) -- one atomic max per position, so the
 *     table is what entering the positions in order leaves, whatever the scheduling;
 *   - builds the primed row tables of the rows engine (levels 1..9 of zng_rocm_compress_streams2_dict_dev below): what its
 *     priming leaves behind the positions [0, T), T the largest multiple of 1024 with T + 3 <= W -- one workgroup, the
 *     matcher's own ordered insert;
 *   - synchronises `stream` once, to bring the DICTID to the host.
 * The object is immutable afterwards and may be used from any thread and any HIP stream of the device it was made on.  After
 * zng_rocm_shutdown() every call with it returns ZNG_ROCM_ENODEV (also under a later zng_rocm_init()); zng_rocm_dict_destroy
 * frees it then as before (NULL is harmless).  zng_rocm_dict_id: the DICTID; zng_rocm_dict_window: W.
 *
 * zng_rocm_compress_streams_dict_dev is zng_rocm_compress_streams_dev with the shared history: format 0 = raw, 1 = zlib; 2
 * (gzip has no dictionary, deflate.c:467) or a NULL dict is ZNG_ROCM_EINVAL with nothing launched.  Per job as there -- out
 * 4-byte aligned, out_cap >= zng_rocm_compress_streams_dict_bound(in_len, format) (0 for a format the call refuses), two
 * result words {total bytes written, Adler-32 of the plaintext} -- with the job's own dict_len 0 and block flags for format
 * 0 only.  The payload comes from the dictionary form of the level-1 kernel: the head table is loaded from the object
 * instead of being zeroed and primed, a candidate in the dictionary is probed and extended from the object's window, and a
 * match whose source begins in the dictionary ends at the dictionary's last byte at the latest.  The zlib wrapper is 16 bytes
 * so that the block starts 4-byte aligned: CMF / FLG with FDICT as deflate.c:868-888 writes them for the fastest level (78
 * 3f), the DICTID most significant byte first (deflate.c:889-892), two empty stored blocks; the trailer is the Adler-32 of
 * the plaintext alone (deflate.c:1098-1101).
 *
 * zng_rocm_uncompress_streams_dict_dev is zng_rocm_uncompress_streams_dev with the shared history (format 2 or a NULL dict:
 * ZNG_ROCM_EINVAL; a job's dict_len and flags are 0).  Format 0: every job decodes with the W bytes as history
 * (inflateSetDictionary on a raw stream).  Format 1, per member: FDICT set and the DICTID the object's -- decoded with the
 * history, in_used counts the 6 header bytes; FDICT set and another DICTID -- status -3, out_len 0, in_used 6, message id 0
 * (inflate.c:1247-1249 sets no text: the one -3 row without a message); FDICT clear -- decoded with NO history, as the large
 * calls do, so a distance beyond the output is "invalid distance too far back"; a header that ends inside the DICTID is
 * reported as a short header is (-5, nothing consumed).  Everything else -- result rows, statuses, trailer checks -- as
 * zng_rocm_uncompress_streams_dev. */
typedef struct zng_rocm_dict zng_rocm_dict;
int      zng_rocm_dict_create_dev(const uint8_t *d_dict, size_t dict_len, zng_rocm_dict **out, void *stream);
void     zng_rocm_dict_destroy(zng_rocm_dict *d);
uint32_t zng_rocm_dict_id(const zng_rocm_dict *d);      /* Adler-32 of ALL dict_len bytes: the DICTID */
uint32_t zng_rocm_dict_window(const zng_rocm_dict *d);  /* bytes that serve as history: min(dict_len, 32768) */
size_t   zng_rocm_compress_streams_dict_bound(size_t source_len, int format);
int      zng_rocm_compress_streams_dict_dev(int format, const zng_rocm_dict *dict, const zng_rocm_stream_job *jobs,
                                            size_t njobs, uint32_t *d_results, void *stream);
int      zng_rocm_uncompress_streams_dict_dev(int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs,
                                              size_t njobs, uint32_t *d_results, void *stream);

/* The shared preset dictionary at EVERY level: zng_rocm_compress_streams2_dev / zng_rocm_compress_members_dev with the object's
 * window as every stream's history.  They behave as those two calls in every respect -- rounds, asynchrony, result words, the
 * offsets table, the does-not-fit rule, zng_rocm_compress_streams2_last_rounds -- except:
 *   format    0 raw (deflateSetDictionary on a raw stream) or 1 zlib; 2 (gzip has no dictionary, deflate.c:467) or a NULL dict
 *             is ZNG_ROCM_EINVAL with nothing launched
 *   zlib      the header is the canonical 6 bytes: CMF FLG with FLEVEL as above, FDICT set and FCHECK making the pair a multiple
 *             of 31 (deflate.c:868-888), then the DICTID, most significant byte first (:889-892) -- no padding, unlike the
 *             16-byte wrapper of zng_rocm_compress_streams_dict_dev; the trailer is the Adler-32 of the plaintext alone.
 *             zng_rocm_uncompress_streams_dict_dev and inflateSetDictionary read these members.
 *   bound     zng_rocm_compress_streams2_dict_bound = zng_rocm_compress_streams2_bound, + 4 for format 1; 0 for a refused format
 *   level     -1, 1..9 with strategy 0, 1 or 4 (Z_FIXED): the dictionary form of the rows matcher (Z_FIXED with the static-only
 *             emitter behind it).  zng_rocm_dict_create_dev has built, once, the row tables the matcher's priming leaves behind
 *             the whole 1 KiB batches inside the window; a stream's first segment loads them (about 88 KiB) and the window into
 *             LDS instead of entering up to 32 batches of history, and every stream's bytes are EXACTLY those the plain call
 *             writes for the same plaintext with the W window bytes copied in front of it and dict_len = W -- matches that
 *             begin in the window and run on into the plaintext included.  Level 0 writes stored blocks behind the FDICT header
 *             and reads no dictionary byte.
 *   strategy  2 (Z_HUFFMAN_ONLY) and 3 (Z_RLE) are ZNG_ROCM_EINVAL here: their front end is another kernel, and at most one
 *             byte of history is not worth a dictionary form
 *   jobs      a job's own dict_len must be 0; flags (ZNG_ROCM_BLOCK_*) in format 0 only
 * A dictionary made before a zng_rocm_shutdown() gives ZNG_ROCM_ENODEV, as in the dictionary calls above; argument refusals
 * come first. */
size_t zng_rocm_compress_streams2_dict_bound(size_t source_len, int format);
int    zng_rocm_compress_streams2_dict_dev(int format, int level, int strategy, const zng_rocm_dict *dict,
                                           const zng_rocm_stream_job *jobs, size_t njobs, size_t round_bytes,
                                           uint32_t *d_results, void *stream);
int    zng_rocm_compress_members_dict_dev(int format, int level, int strategy, const zng_rocm_dict *dict,
                                          const zng_rocm_stream_job *jobs, size_t njobs, uint8_t *d_dst, size_t dst_cap,
                                          size_t round_bytes, uint64_t *d_offsets, uint32_t *d_checks, void *stream);

/* Many small device-resident streams whose plaintext lengths nobody handed over: the read side of
 * zng_rocm_compress_members_dev.  Raw deflate and zlib members do not record their length; these two calls find it on the
 * device.  Both are asynchronous on `stream`, with no host synchronisation and no device-to-host copy inside; results are
 * valid once the stream has got there.
 *   format    0 raw, 1 zlib, 2 gzip; another value is ZNG_ROCM_EINVAL
 *   dict      NULL, or a zng_rocm_dict for format 0 and 1 (format 2 with one: ZNG_ROCM_EINVAL, as in the *_dict calls)
 *   jobs      HOST array, copied internally.  in / in_len: the whole member with its wrapper, as
 *             zng_rocm_uncompress_streams_dev takes them, in_len below 2 GiB; out and out_cap are not looked at; flags 0
 *   refusals  ZNG_ROCM_EINVAL before anything is launched or written: the format, a null buffer with a length, in_len of 2 GiB
 *             and more, flags, a dict_len above 32768 or beside `dict` or a wrapped format, a null d_results with njobs > 0.  A
 *             dictionary made before a zng_rocm_shutdown(): ZNG_ROCM_ENODEV, after the argument checks
 *
 * zng_rocm_inflate_sizes_dev: d_results (device, 4 words per job) = {plaintext bytes, input bytes consumed, status, message
 *   id}: the row zng_rocm_inflate_streams_dev (format 0) or zng_rocm_uncompress_streams_dev / _dict_dev (1, 2) would write for
 *   the job with out_cap = 0x7fffffff and its history in place -- every header refusal, "need dictionary", the DICTID mismatch
 *   (-3, message 0), every data error with its message and its count of bytes consumed, truncation (-5) -- except that the
 *   trailer's check value and ISIZE are not compared: there is no plaintext to check.  Status 1 for a wrapped member: header
 *   accepted, payload decoded to its final block, the 4 / 8 trailer bytes present and counted (input that ends inside the
 *   trailer: -5).  No output and no history byte is touched; of the history only the LENGTH matters: jobs[i].dict_len (format 0
 *   without `dict`: the bytes the caller will place in front of `out`) or the object's window as the header's verdict gives
 *   it.  A plaintext that does not fit 0x7fffffff bytes: {0x7fffffff, ., -5, "output buffer too small"}.  One field is NOT the
 *   decode's: the plaintext count of a stream that runs out of input (-5, "input ended ...") is the bytes of the symbols whose
 *   bits were all input -- what inflate() delivers for that input -- where the decode's partial count also holds what the
 *   zero bits behind the input decoded to.  njobs == 0 returns 0.
 *
 * zng_rocm_uncompress_packed_dev: sizes, places, decode and verification in one enqueue sequence.  A job whose sizing row has
 *   status 1 gets its size in bytes of d_dst, every other job none; job i starts at d_offsets[i] = the end of the bytes in front
 *   of it, rounded up to `align` (0 or 1: back to back; else a power of two up to 4096, anything else ZNG_ROCM_EINVAL);
 *   d_offsets (device, njobs + 1, required) [njobs] = the end of the last job's bytes: the room the batch needs.  Padding is never
 *   written.  A job that ends at or before dst_cap is decoded by the existing engine and verified (check value and ISIZE
 *   compared: "incorrect data check" / "incorrect length check" appear here, out_len the decoded count); a job that does not fit
 *   gets {0, 0, -5, "output buffer too small"} and nothing is stored at or behind d_dst + dst_cap -- d_offsets still describes
 *   the whole layout, so a caller allocates d_offsets[njobs] bytes and calls again; a job whose sizing row was not status 1 gets
 *   {0, the sizing row's in_used, its status, its message}.  Complete streams only: for the bytes in front of a fault decode
 *   that stream alone.  Refused on top: jobs[i].dict_len != 0, a null d_dst with dst_cap > 0, a null d_offsets or d_results. */
int    zng_rocm_inflate_sizes_dev(int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                                  uint32_t *d_results, void *stream);
int    zng_rocm_uncompress_packed_dev(int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, size_t njobs,
                                      uint8_t *d_dst, size_t dst_cap, uint32_t align, uint64_t *d_offsets, uint32_t *d_results,
                                      void *stream);

/* zlib (format 1) / gzip (format 2) members around the LARGE device inflaters: zng_rocm_inflate_large_streams_dev (the
 * batch) and zng_rocm_inflate_large_pieces_dev (one member of any length) for wrapped streams that already sit in device
 * memory.  format 0 is the raw call itself, field for field and byte for byte; any other format value is ZNG_ROCM_EINVAL
 * with nothing launched or written.
 * Per job `d_src / src_len` is the whole member, wrapper included.  `d_window / window_len` is the PRESET DICTIONARY of a
 * zlib member (inflateSetDictionary, inflate.c:1214-1261) and must be NULL / 0 for gzip (else ZNG_ROCM_EINVAL for the call,
 * before anything is launched).  round_bytes / piece_bytes, flags (0 or ZNG_ROCM_INFLATE_SUBBLOCK), the refusals, the
 * thread-local zng_rocm_inflate_large_last_* counters and the scratch bounds are those of the raw calls, which run on the
 * payload.
 * What happens: every header is parsed on the device, one wavefront per member (inflate.c:509-555 zlib, :556-700 gzip with
 * FEXTRA / FNAME / FCOMMENT / FHCRC of any length, :702-715 DICTID; for zlib the Adler-32 of every dictionary given, one pass);
 * one small readback; the raw engine on the payloads; the check values of all outputs in one many-message pass over 512 KiB
 * sub-messages folded per member on the device (the single call: the full-grid checksum kernel over its one output); one
 * small kernel compares the trailers (inflate.c:1105-1147).  Only the FIRST member of a multi-member gzip file is decoded;
 * in_used is where the next one starts (every member: zng_rocm_gunzip_members_dev).  The header kernel and the checksum pass fetch aligned 16-byte lines: up to 15 bytes
 * on either side of a member, a dictionary or an output, inside the same 16-byte line, are read (never used).
 * Per job (batch) or per call (single; the text of a data error then in zng_rocm_last_error()):
 *   member complete, check value and length agree   status 1, out_len, in_used = header + payload + trailer (4 / 8 bytes)
 *   wrapper refused     -3, out_len 0, msg "incorrect header check" (also a gzip magic other than 1f 8b), "unknown
 *                       compression method", "invalid window size" (inflate.c:527-546), "unknown header flags set"
 *                       (:565-567), "header crc mismatch" (:686-692)
 *   input ends inside the header                     -5, out_len 0, in_used = src_len
 *   zlib FDICT set, no dictionary given              2 (Z_NEED_DICT, inflate.c:713-715), out_len 0, in_used 6
 *   zlib FDICT set, Adler-32 of the dictionary differs from DICTID    -3, out_len 0, msg NULL (inflate.c:1247-1249)
 *   zlib FDICT clear                                 the payload is decoded with NO history, dictionary or not
 *   the payload's own trouble (data error, truncated, dst_cap too small)   as the raw call; in_used counts the header
 *   payload complete, input ends inside the trailer  -5, out_len (the plaintext is in place), in_used = src_len
 *   check value differs                              -3, out_len, msg "incorrect data check" (inflate.c:1132)
 *   gzip ISIZE != out_len mod 2^32                   -3, out_len, msg "incorrect length check" (inflate.c:1146)
 * Synchronous. */
int  zng_rocm_uncompress_large_streams_dev(int format, zng_rocm_inflate_large_job *jobs, size_t njobs, size_t round_bytes,
                                           uint32_t flags, void *stream);
int  zng_rocm_uncompress_large_dev(int format, const uint8_t *d_src, size_t src_len, const uint8_t *d_dict, uint32_t dict_len,
                                   uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, size_t *in_used, size_t piece_bytes,
                                   uint32_t flags, void *stream);
/* The plaintext SIZE of large device-resident streams, without decoding them: what a caller needs before it can hand any of
 * the large inflaters a destination -- raw deflate and zlib do not record the length, gzip records it mod 2^32 only.
 * One finder pass, ONE launch of a counting part kernel (one wavefront per part; it stores nothing but eight result words per
 * part) and the chain walk of the decode: no part slots, no rerun of parts above a ratio of 64, no symbol array, no resolve,
 * and no byte of the stream comes to the host.  Device scratch is the finder's tables (about src_len / 7) and under 100 bytes
 * per part, against the decode's 128 bytes per compressed byte.  A stream the finder does not cut (below 128 KiB, fewer
 * than four starts, more parts than a launch takes) is ONE part of the same launch, its whole length walked by one
 * wavefront; a stream with anything irregular on its chain is sized once more on the device, whole, by one wavefront of a
 * second kernel that gives the decoder's verdict, message and consumed bytes.
 *   format    0 raw: d_dict / dict_len (window_len) is the LENGTH (<= 32768) of the history the caller will put in front; its
 *             bytes are not looked at and the pointer may be NULL.  1 zlib, 2 gzip: the whole member with its wrapper; the
 *             header is parsed and FDICT / DICTID judged as zng_rocm_uncompress_large_dev does (the dictionary's bytes are
 *             needed for the DICTID; gzip with a dictionary: ZNG_ROCM_EINVAL); the 4 / 8 trailer bytes must be present and
 *             are counted, but the check value and ISIZE are NOT compared -- there is no plaintext to check, so a member with
 *             a damaged trailer still answers 1 (as in zng_rocm_inflate_sizes_dev)
 *   results   what zng_rocm_inflate_sizes_dev's row says of the same stream and history length, with a 64-bit count that
 *             does not saturate: 1 with the plaintext length and the bytes used; every header refusal, 2 (Z_NEED_DICT), the
 *             DICTID mismatch (-3, no text), every data error with its text and consumed bytes, truncation (-5; out_len then
 *             the bytes of the symbols whose bits were all input) -- header verdicts as zng_rocm_uncompress_large_dev lists
 *             them.  The single call: *out_len, *in_used, the return value, a data error's text in zng_rocm_last_error().
 *             The batch: per job status / out_len / in_used / msg / parts, subparts 0; d_dst / dst_cap are not looked at and
 *             nothing is written there.  The plaintext may be of any size.
 *   counters  zng_rocm_inflate_large_last_parts() (the single call) and `parts` (the batch): the parts on the chain -- the
 *             decode's count for the same stream; 1: the stream was not cut; 0: the second kernel sized it whole, as for
 *             every stream that is not a valid one.  zng_rocm_inflate_large_last_rounds() / _last_part_launches(): as for
 *             zng_rocm_inflate_large_streams_dev, with exactly one launch of the counting part kernel per round
 *   refusals  ZNG_ROCM_EINVAL before anything is launched or written: a format outside 0 .. 2; any flag bit (there is no
 *             ZNG_ROCM_INFLATE_SUBBLOCK form; zng_rocm_last_error() names the bits); dict_len / window_len above 32768; a
 *             null d_src with a length; a null out_len or in_used; round_bytes outside zng_rocm_inflate_large_streams_dev's
 *             range; src_len of 2 GiB and more (bit positions must fit the part tables; sizing in pieces is a later step).
 *             An accepted call before zng_rocm_init: ZNG_ROCM_ENODEV, nothing written.
 * Both synchronous.  The batch returns 0 or the first device error; a stream's own trouble is its job's status alone. */
int  zng_rocm_uncompress_large_size_dev(int format, const uint8_t *d_src, size_t src_len, const uint8_t *d_dict, uint32_t dict_len,
                                        uint64_t *out_len, size_t *in_used, uint32_t flags, void *stream);
int  zng_rocm_uncompress_large_sizes_dev(int format, zng_rocm_inflate_large_job *jobs, size_t njobs, size_t round_bytes,
                                         uint32_t flags, void *stream);
/* The wrapper alone, on HOST bytes: the same rules as the header kernel of the two calls above (one function for both),
 * no device needed -- works before zng_rocm_init and without a GPU.  Returns 0 (header complete and accepted; info filled),
 * 2 (accepted zlib header with FDICT: info->dictid is the Adler-32 the dictionary must have, header_len 6), -3 with the
 * reference's text in *msg (static storage; msg may be NULL), -5 (src_len ends inside the header), ZNG_ROCM_EINVAL with
 * *msg = NULL for a format outside 0 .. 2 or a null argument.  format 0: header_len 0. */
typedef struct zng_rocm_wrapper_info {
    uint64_t header_len;   /* bytes in front of the raw deflate payload */
    uint32_t dictid;       /* zlib with FDICT: the Adler-32 the dictionary must have, else 0 */
    uint32_t fdict;        /* 1 when the zlib header announces a preset dictionary */
} zng_rocm_wrapper_info;
int  zng_rocm_wrapper_parse(int format, const uint8_t *src, size_t src_len, zng_rocm_wrapper_info *info, const char **msg);

/* EVERY member of a gzip file that sits in device memory, BGZF (bgzip, BAM, tabix) included: what gzread does with a file
 * of several members -- gz_look (gzread.c.in:81-154) starts a new member whenever 1f 8b follows a finished one and ignores
 * anything else as trailing garbage, gz_decomp (:161-207) inflates each -- for a file that is all in memory, in place of the
 * caller's loop over zng_rocm_uncompress_large_dev(2, ...) along in_used.  The plaintexts land in d_dst one behind the other
 * in file order.
 * What happens: one pass over the file marks every position that holds 1f 8b 08 F with F & 0xe0 == 0 (a candidate: the
 * bytes every accepted header begins with, inflate.c:556-567); the header kernel of the wrapped large calls judges every
 * candidate; a BGZF 'BC' subfield (SI1 66, SI2 67, SLEN 2: BSIZE = member bytes - 1) says where its member ends, any other
 * member is guessed to reach the next candidate, and the eight bytes in front of the guessed end are its guessed CRC-32 and
 * ISIZE.  Discovery synchronises twice: the candidates' number comes down (4 bytes: it sizes the tables), then the candidate
 * table, once, 40 bytes per candidate; every plan that holds members of the one-wavefront engine reads their results back
 * (16 bytes each), and the large batch synchronises as zng_rocm_uncompress_large_streams_dev does.  What a file made to hurt
 * can cost is bounded: the header kernel is shown at most 4 KiB of a candidate (a header that does not end inside them --
 * legal: FEXTRA alone can be 64 KiB -- counts as cut, and its member is decoded alone by the single call, with the same
 * results), and a file with more than 2^24 candidates gets no table: it goes through single calls, member by member, and
 * zng_rocm_gunzip_last_candidates() says -1.  From candidate 0 the host follows the guesses: members below 128 KiB go to
 * zng_rocm_uncompress_streams_dev in one launch (one wavefront each), the others to zng_rocm_uncompress_large_streams_dev,
 * every one with exactly its guessed ISIZE as capacity.  A member counts when it decoded with status 1 (so check value and
 * length agree), consumed exactly its guessed bytes and produced exactly its guessed length, and every member in front of it
 * counts.  The first one that does not (a candidate inside its data that was no member, an ISIZE that wrapped at 4 GiB) is
 * decoded alone by zng_rocm_uncompress_large_dev(2, ...) where it really belongs, and the plan is made again from where it
 * really ended: a re-plan; after 8 of them the rest of the file goes through single calls.  A candidate that was no member
 * never contributes a byte to d_dst[0, *out_len) or a row to `members` (bytes of d_dst behind *out_len, inside dst_cap, may
 * have been written).
 * Results (gz_look / gz_decomp):
 *   the first member   judged exactly as zng_rocm_uncompress_large_dev(2, ...) judges it: status, text in
 *                      zng_rocm_last_error(), *out_len, *in_used; src_len == 0 included
 *   behind a complete member   fewer than 2 bytes, or two bytes other than 1f 8b: trailing garbage (gz_look asks avail_in > 1,
 *                      gzread.c.in:127), the call returns 1 with *in_used = the end of the last member
 *                      1f 8b: a member that has to decode; a header refusal, data error or check mismatch returns -3 with the
 *                      reference's text, a truncated member -5
 *   on failure         *out_len = the plaintext of the complete members in front + what the failing member's own call
 *                      reports, *in_used = its offset + its in_used, *nmembers = the complete members in front
 *   dst_cap            nothing is written at or behind d_dst + dst_cap; a file that does not fit returns -5
 * Empty members (ISIZE 0, the BGZF end-of-file block) are members; members of 4 GiB and more work (the pieces engine).
 * `members` (NULL when members_cap is 0) receives one row per complete member, the first members_cap of them; *nmembers is
 * always the true count.  flags: 0 or ZNG_ROCM_INFLATE_SUBBLOCK, passed to the large engine.  Unknown flag bits, a null buffer
 * with a non-zero length or a null result pointer return ZNG_ROCM_EINVAL with nothing launched or written and *out_len =
 * *in_used = *nmembers = 0.  The scan and the header kernel fetch aligned 16-byte lines: up to 15 bytes on either side of the
 * file inside the same line are read (never used).  Synchronous. */
typedef struct zng_rocm_gzip_member {
    uint64_t src_off, src_len;   /* the member in d_src, header and trailer included */
    uint64_t dst_off, out_len;   /* its plaintext in d_dst */
    uint32_t crc;                /* CRC-32 of that plaintext (the trailer's, verified) */
    uint32_t bgzf;               /* 1: the header carried a BGZF 'BC' subfield */
} zng_rocm_gzip_member;
int  zng_rocm_gunzip_members_dev(const uint8_t *d_src, size_t src_len, uint8_t *d_dst, size_t dst_cap, uint64_t *out_len,
                                 size_t *in_used, zng_rocm_gzip_member *members, size_t members_cap, size_t *nmembers,
                                 uint32_t flags, void *stream);
/* of the calling thread's last zng_rocm_gunzip_members_dev call (thread-local, like the other last_* counters): candidates
 * the scan found, re-plans, members the one-wavefront engine decoded, members the large engines decoded (the batch, and the
 * single call for a member decoded alone) */
int  zng_rocm_gunzip_last_candidates(void);
int  zng_rocm_gunzip_last_replans(void);
int  zng_rocm_gunzip_last_small(void);
int  zng_rocm_gunzip_last_large(void);

/* The write side of the call above: device-resident plaintext -> a BGZF file in device memory (SAM specification 4.1; what
 * bgzip, BAM and tabix read), nothing crossing PCIe.  d_src[0, src_len) is cut every block_bytes bytes (0 = 65280; 1 .. 65280,
 * anything above is ZNG_ROCM_EINVAL); piece i becomes member i, the members stand one behind the other from d_dst[0] at byte
 * granularity; neither buffer has an alignment requirement.
 *   a member    1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 <BSIZE lo> <BSIZE hi> (htslib's header at every level; BSIZE =
 *               the member's bytes - 1) | raw deflate of the piece, no history, one final stream | CRC-32 of the piece |
 *               its length, both least significant byte first
 *   the end     unless ZNG_ROCM_BGZF_NO_EOF is set, the 28 constant bytes of the end-of-file block (an empty member); src_len
 *               == 0 gives exactly those 28 bytes, with NO_EOF nothing at all
 *   level       as zng_rocm_compress2_dev: -1 = 6; 1..9 the engine of zng_rocm_deflate_streams_dev, every piece an independent
 *               stream; 0 = every member one stored block (no engine is launched); with ZNG_ROCM_BGZF_QUICK (level must be 1)
 *               the payloads come from the engine of zng_rocm_deflate_quick_dev
 *   64 KiB      a piece of n bytes whose engine output has clen bytes with clen > n + 5 or clen > 65510 gets one final stored
 *               block (01 LEN NLEN and the n bytes) as its payload instead -- decided on the device from the engine's own
 *               length; zng_rocm_bgzf_last_stored() counts these members (at level 0: every member).  So a member is at most
 *               n + 31 bytes and at most 65536, and zng_rocm_bgzf_bound(src_len, block_bytes) = src_len + 31 per member + 28
 *               bounds the file (0 for a block_bytes the call refuses)
 *   dst_cap     need not reach the bound: every member's place is known on the device before a byte of it is written, nothing
 *               is stored at or behind d_dst + dst_cap, and a file that does not fit returns -5 (Z_BUF_ERROR) with *out_len =
 *               the bytes it needs (and *nmembers, `members` as on success); d_dst[0, dst_cap) then holds the file's beginning
 *   members     (NULL when members_cap is 0) the first members_cap rows, in the meaning zng_rocm_gunzip_members_dev gives the
 *               struct -- src_off / src_len the member inside the BGZF file, dst_off / out_len its plaintext range, crc, bgzf 1;
 *               the end-of-file block is a row with out_len 0 -- exactly the rows that call reports for the file: the content
 *               of a .gzi index and of virtual offsets.  *nmembers is always the true count
 *   rounds      scratch is bounded: the pieces go through the device in rounds of at most round_bytes of plaintext (0 = 1 GiB
 *               + 65280; rounded down to whole pieces, at least one), the running file offset carried on the device from
 *               round to round; zng_rocm_bgzf_last_rounds() says how many there were
 * Per round: the CRC-32 of every piece in one many-message pass (the kernels of zng_rocm_checksums_dev), the engine, one
 * workgroup that turns the engine's lengths into member sizes and scans them, one kernel that writes every header and trailer
 * and moves every payload to its byte (levels 1..9: straight from the engine's block slots; stored members: from the
 * plaintext).  Synchronous, one host
 * synchronisation for the whole call; the members table comes down only when members_cap > 0.  The checksum pass fetches
 * aligned 16-byte lines: up to 15 bytes on either side of the plaintext inside the same line are read (never used).
 * Returns 0, -5, or ZNG_ROCM_EINVAL -- unknown flag bits, a level outside -1..9, QUICK with a level other than 1, block_bytes
 * above 65280, a null buffer with a non-zero length or capacity, a null out_len or nmembers -- with nothing launched or
 * written and *out_len = *nmembers = 0.  The two counters are thread-local, like the other last_* counters. */
#define ZNG_ROCM_BGZF_BLOCK   65280u      /* htslib's BGZF_BLOCK_SIZE: the most plaintext one member takes */
#define ZNG_ROCM_BGZF_NO_EOF  1u          /* do not append the 28-byte end-of-file block (the caller appends more) */
#define ZNG_ROCM_BGZF_QUICK   2u          /* the level-1 CLASS (zng_rocm_deflate_quick_dev: static Huffman, one kernel); level must be 1 */
size_t zng_rocm_bgzf_bound(size_t src_len, uint32_t block_bytes);
int    zng_rocm_bgzf_compress_dev(int level, const uint8_t *d_src, size_t src_len, uint32_t block_bytes,
                                  uint8_t *d_dst, size_t dst_cap, uint64_t *out_len,
                                  zng_rocm_gzip_member *members, size_t members_cap, size_t *nmembers,
                                  size_t round_bytes, uint32_t flags, void *stream);
int    zng_rocm_bgzf_last_rounds(void);
int    zng_rocm_bgzf_last_stored(void);

/* ---- BGZF random access: what the members of at most 64 KiB are for (SAM specification 4.1; bgzip, BAM, tabix) ------------
 * zng_rocm_bgzf_index_dev: the members table of a device-resident BGZF file WITHOUT decoding it -- the cost of a scan, not of
 * an inflate.  For a well-formed file the rows are exactly the rows zng_rocm_gunzip_members_dev reports for it: src_off,
 * src_len (BSIZE + 1), dst_off (the running sum of ISIZE), out_len (ISIZE), crc (the trailer's word), bgzf 1; the end-of-file
 * block is a row with out_len 0; *plain_len is their sum, *in_used the end of the last member; members_cap / *nmembers as in
 * that call.  The rows are what the file CLAIMS (BSIZE of the 'BC' subfield, the eight bytes in front of the claimed end): no
 * inflate kernel is launched, and zng_rocm_bgzf_read_dev below verifies what it uses.
 * What happens: the candidate scan, scatter and header kernel of zng_rocm_gunzip_members_dev (same bounds: a candidate's
 * header is shown at most 4 KiB); one lane per candidate writes a row for every accepted header with a 'BC' subfield; the
 * table comes down once (32 bytes per candidate; two synchronisations in all); the host follows the chain from offset 0 by
 * binary search, so candidates inside a member's bytes are never looked at.
 * Results (what follows a member is judged as gz_look judges it, gzread.c.in:81-154):
 *   0    the chain reached the end of the file, or trailing garbage behind a complete member -- fewer than 2 bytes, or two
 *        bytes other than 1f 8b (gz_look asks avail_in > 1, gzread.c.in:127) -- with *in_used in front of the garbage;
 *        src_len == 0: no members
 *   -3   behind a complete member, or at offset 0, 1f 8b (at offset 0: anything) where no accepted BGZF header begins -- a
 *        plain gzip member, a refused header, one longer than 4 KiB, a BSIZE that leaves no room for header, two bytes of
 *        deflate and trailer, an ISIZE above 65536; zng_rocm_last_error() names the offset; *nmembers, *plain_len, *in_used
 *        and `members` describe the members in front
 *   -5   a member whose BSIZE end lies behind src_len, or a header the file's end cuts (1f 8b with fewer than two bytes
 *        behind it, and a file shorter than 18 bytes, included); the same outputs
 *   ZNG_ROCM_EINVAL   a null buffer with a non-zero length or a null result pointer: nothing launched or written, the outputs
 *        zeroed; more than 2^24 candidates (known behind the scan): the outputs zeroed -- zng_rocm_gunzip_members_dev reads
 *        such a file
 * The scan and the header kernel fetch aligned 16-byte lines: up to 15 bytes on either side of the file inside the same line
 * are read (never used).  Synchronous.
 *
 * zng_rocm_bgzf_read_dev: MANY plaintext ranges [uoff, uoff + len) of the file in one set of launches, decoding only the
 * members the ranges touch.  `members` is a HOST array: the rows of zng_rocm_bgzf_index_dev, zng_rocm_gunzip_members_dev or
 * zng_rocm_bgzf_compress_dev for this file.  Before anything is launched the rows are checked -- src_off ascending and
 * members not overlapping, every member inside src_len, dst_off contiguous from 0, bgzf == 1, 28 <= src_len <= 65536, out_len
 * <= 65536 -- and every range for a null d_dst with a non-zero len; scratch_bytes is 0 (= 256 MiB) or 128 KiB .. 4 GiB.  Any
 * violation is ZNG_ROCM_EINVAL with nothing launched and no range field or destination byte written.
 * plain_len is the end of the last row, and a range is clipped to it: uoff >= plain_len gives status 1 with out_len 0, else
 * out_len = min(len, plain_len - uoff) on success.  Members with out_len 0 are never decoded.
 * What happens: for every range a binary search finds its first member.  A member that lies wholly inside the range is
 * decoded straight to d_dst + (row.dst_off - uoff) with exactly row.out_len as capacity; a member the range only cuts (an
 * edge: a range has at most two) is decoded into a 64 KiB slot of scratch, once per round however many ranges cut it, and
 * each of those ranges gets a slice of it.  All members of a round go through ONE launch of the one-wavefront engine as gzip
 * members (zng_rocm_uncompress_streams_dev, format 2), so header, payload, CRC-32 and ISIZE are verified on the device
 * (inflate.c:556-700, :1105-1147); behind it on the same stream, with no host round trip, one kernel copies the slices, one
 * workgroup each -- only from a member that ended with status 1, consumed exactly row.src_len and produced exactly
 * row.out_len -- with 16-byte vector stores and byte steps at head and tail, for every pair of alignments.  One readback of
 * the result rows and one synchronisation per round.  Ranges are taken in order until the edge slots of a round would pass
 * scratch_bytes (or the round holds 2^22 members: its tables are bounded like its slots); a range is never split across rounds.
 * Per range:
 *   status 1    every member it touched verified; out_len = the clipped length, msg NULL
 *   status -3   a member failed with a data or check error: msg is the engine's text for the first such member of the range
 *               ("incorrect data check", "incorrect length check", "invalid distance too far back", ...), or "index row does
 *               not match the file" when that member decoded cleanly but consumed or produced other than its row says
 *   status -5   no member failed that way, but one was truncated or did not fit its row's out_len; msg NULL
 *   on failure  out_len = the bytes of the range in front of the first failing member's part; those bytes, and the parts of
 *               members behind it that verified, are in place; an edge member that failed has written nothing to d_dst
 * Nothing outside [d_dst, d_dst + len) of any range is ever written, and one range's failure does not change another's
 * result.  Returns 0, or the first device error.  Synchronous.  The three counters are thread-local, like the other last_*
 * ones: members put through the engine, of those the members decoded straight into a destination, rounds.
 *
 * Virtual offsets, htslib's convention (host only; both work without a device): voff = src_off << 16 | (uoff - dst_off) of
 * the member that holds uoff -- an offset at a member's end is offset 0 of the next non-empty member, and plain_len maps to
 * the start of the last row (the end-of-file block of a complete file).  The inverse is uoff = dst_off + (voff & 0xffff) of
 * the member at voff >> 16.  ZNG_ROCM_EINVAL: uoff > plain_len, src_off >= 2^48, voff >> 16 is no member's src_off, voff &
 * 0xffff is above that member's out_len, an offset sixteen bits cannot say, an empty table, a null pointer. */
typedef struct zng_rocm_bgzf_range {
    uint64_t    uoff;      /* first plaintext byte */
    uint64_t    len;       /* bytes wanted */
    uint8_t    *d_dst;     /* device, any alignment, len bytes */
    /* out */
    int         status;    /* 1, -3, -5 */
    uint64_t    out_len;
    const char *msg;       /* static text on -3, else NULL */
} zng_rocm_bgzf_range;
int    zng_rocm_bgzf_index_dev(const uint8_t *d_src, size_t src_len, zng_rocm_gzip_member *members, size_t members_cap,
                               size_t *nmembers, uint64_t *plain_len, size_t *in_used, void *stream);
int    zng_rocm_bgzf_read_dev(const uint8_t *d_src, size_t src_len, const zng_rocm_gzip_member *members, size_t nmembers,
                              zng_rocm_bgzf_range *ranges, size_t nranges, size_t scratch_bytes, void *stream);
int    zng_rocm_bgzf_read_last_decoded(void);
int    zng_rocm_bgzf_read_last_direct(void);
int    zng_rocm_bgzf_read_last_rounds(void);
int    zng_rocm_bgzf_voffset(const zng_rocm_gzip_member *members, size_t nmembers, uint64_t uoff, uint64_t *voff);
int    zng_rocm_bgzf_uoffset(const zng_rocm_gzip_member *members, size_t nmembers, uint64_t voff, uint64_t *uoff);

/* ---- gzip header FIELDS of device-resident members: set on write, get on read -------------------------------------------
 * deflateSetHeader and inflateGetHeader (zlib-ng.h.in:127-141 the zng_gz_header, :796-816, :1020-1055): what deflate.c:922-1023
 * writes in front of a member -- FTEXT, MTIME, OS, the FEXTRA subfields, FNAME, FCOMMENT, the FHCRC -- and inflate.c:556-700 reads
 * back, for the members zng_rocm_compress_members_dev writes and zng_rocm_gunzip_members_dev / zng_rocm_bgzf_index_dev find.
 *
 * zng_rocm_gzip_header: one member's fields; everything it points to is HOST memory and is copied before a call returns.
 *   FLG = text ? 1 : 0 + hcrc ? 2 : 0 + (extra != NULL) ? 4 : 0 + (name != NULL) ? 8 : 0 + (comment != NULL) ? 16 : 0 (deflate.c:927-932)
 *   then MTIME little endian, XFL by level and strategy as the canonical header (deflate.c:939-940), os & 0xff, XLEN and the extra
 *   bytes, name and its 0, comment and its 0, and with hcrc the low 16 bits of the CRC-32 of everything in front (deflate.c:1005-1016).
 * Refused: extra_len above 65535 (the reference writes extra_len & 0xffff as XLEN and still copies extra_len bytes, deflate.c:
 * 947-949: a header no reader follows); extra == NULL with extra_len != 0; a name or a comment of more than 65535 bytes without
 * its terminator (the library's own limit, zlib has none: a header is at most 196621 bytes); reserved != 0.
 * zng_rocm_gzip_header_bytes: the header's length without rendering it; NULL: the canonical 10 bytes; 0 for a refused header.
 * zng_rocm_gzip_header_write: the header into buf[0, cap) on the HOST, no device needed (works before zng_rocm_init and without a
 *   GPU).  level -1 or 0..9 and strategy 0..4 give XFL; NULL: the canonical header.  Returns the bytes written, 0 for a refused
 *   header, level or strategy or when cap is too small (nothing written).
 *
 * zng_rocm_compress_streams2_header_dev / zng_rocm_compress_members_header_dev: zng_rocm_compress_streams2_window_dev(2, ...) /
 * zng_rocm_compress_members_window_dev(2, ...) with `heads`, a HOST array of njobs headers (copied internally, as jobs): member i
 * is the rendered heads[i], then exactly the deflate data those calls write for the same job list, level, strategy and window,
 * then CRC-32 and ISIZE.  gzip only.  heads == NULL: exactly those calls, bytes, results and refusals.  Per-job buffers need
 * out_cap >= zng_rocm_compress_streams2_bound(in_len, 2) - 10 + zng_rocm_gzip_header_bytes(&heads[i]) (less: -5, nothing launched;
 * a bound that does not fit 32 bits: ZNG_ROCM_EINVAL).  A refused header is ZNG_ROCM_EINVAL for the call with nothing launched or
 * written.  Result words, d_offsets, d_checks, rounds and the dst_cap rule -- no byte at or behind d_dst + dst_cap is written, a
 * cut inside a header included -- are those of the calls above, and the calls stay asynchronous: the host renders every header
 * into one pinned blob that goes up with the job table. */
typedef struct zng_rocm_gzip_header {   /* zng_gz_header for one member; everything it points to is HOST memory */
    uint32_t time, os, text, hcrc;      /* os written as os & 0xff; text / hcrc: non-zero = set */
    const uint8_t *extra;               /* NULL: no FEXTRA; non-NULL with extra_len 0: an empty field (XLEN 0) */
    const char    *name;                /* zero-terminated; NULL: no FNAME */
    const char    *comment;             /* zero-terminated; NULL: no FCOMMENT */
    uint32_t extra_len, reserved;       /* <= 65535; 0 */
} zng_rocm_gzip_header;
size_t zng_rocm_gzip_header_bytes(const zng_rocm_gzip_header *h);
size_t zng_rocm_gzip_header_write(const zng_rocm_gzip_header *h, int level, int strategy, uint8_t *buf, size_t cap);
int    zng_rocm_compress_streams2_header_dev(int level, int strategy, int window_bits, const zng_rocm_stream_job *jobs,
                                             const zng_rocm_gzip_header *heads, size_t njobs, size_t round_bytes,
                                             uint32_t *d_results, void *stream);
int    zng_rocm_compress_members_header_dev(int level, int strategy, int window_bits, const zng_rocm_stream_job *jobs,
                                            const zng_rocm_gzip_header *heads, size_t njobs, uint8_t *d_dst, size_t dst_cap,
                                            size_t round_bytes, uint64_t *d_offsets, uint32_t *d_checks, void *stream);
/* The read side (inflateGetHeader, inflate.c:556-700).  status, msg and header_len of a row are what
 * zng_rocm_wrapper_parse(2, member, ...) says about the same bytes -- one text of rules (a bad FHCRC: -3, "header crc mismatch");
 * the other fields are filled for status 0 and are 0 otherwise.
 * zng_rocm_gzip_header_parse: one member in HOST memory, no device needed.  Returns the row's status, or ZNG_ROCM_EINVAL for a
 *   null row or a null src with a length (the row, if any, then holds status ZNG_ROCM_EINVAL and zeros); text_off is 0.
 * zng_rocm_gzip_headers_dev: the headers of `nmembers` members of the device-resident file d_src[0, src_len).
 *   members     HOST array; only src_off and src_len are read: the table zng_rocm_gunzip_members_dev or zng_rocm_bgzf_index_dev
 *               hands back, or one built from the d_offsets of the writers above
 *   rows        HOST array of nmembers
 *   text        HOST buffer of text_cap bytes (NULL with text_cap 0): for the members with status 0, in member order, the extra
 *               bytes, the name and a 0, the comment and a 0 -- the fields the member has; rows[i].text_off is where member i's
 *               begin (a running sum, also for members that put nothing there).  *text_need, always set, is the total; with
 *               text_cap < *text_need the rows are delivered, `text` is untouched and the call returns -5.
 *   A header is followed as far as its member reaches: the 4 KiB the header kernel of zng_rocm_gunzip_members_dev is shown are no
 *   limit here.  One wavefront per member walks the rules, the FHCRC goes through the many-message checksum pass, one workgroup
 *   scans the lengths, one workgroup per member gathers its fields.  Synchronous, with at most two device-to-host copies (the
 *   rows, the text).  A member that does not lie inside src_len, more than 2^31 - 1 members, or a null pointer with a non-zero
 *   count is ZNG_ROCM_EINVAL with nothing launched or written (but *text_need = 0); nmembers == 0 returns 0; before
 *   zng_rocm_init an accepted call returns ZNG_ROCM_ENODEV.  The header kernel and the checksum pass fetch aligned 16-byte
 *   lines: up to 15 bytes on either side of a member inside the same line are read (never used). */
typedef struct zng_rocm_gzip_header_row {
    int32_t     status;                       /* 0 / -3 / -5: zng_rocm_wrapper_parse(2, member)'s return for the same bytes */
    uint32_t    flg;                          /* the FLG byte (status 0) */
    const char *msg;                          /* that call's text (static storage), NULL unless -3 */
    uint64_t    header_len;
    uint32_t    time, xflags, os, text, hcrc, extra_len;
    uint64_t    name_len, comment_len;        /* without the terminator */
    uint64_t    extra_off, name_off, comment_off;   /* in d_src, counted from the FILE's first byte; 0 when the field is absent */
    uint64_t    text_off;                     /* where this member's fields begin in `text` */
} zng_rocm_gzip_header_row;
int    zng_rocm_gzip_header_parse(const uint8_t *src, size_t src_len, zng_rocm_gzip_header_row *row);
int    zng_rocm_gzip_headers_dev(const uint8_t *d_src, size_t src_len, const zng_rocm_gzip_member *members, size_t nmembers,
                                 zng_rocm_gzip_header_row *rows, uint8_t *text, size_t text_cap, size_t *text_need, void *stream);

/* ---- random access into ONE plain stream: raw deflate, zlib or gzip (what zran.c and indexed_gzip do on a CPU) -------------
 * A BGZF file offers random access by construction; every other stream -- a plain .gz, a zlib stream, raw deflate, what
 * zng_rocm_compress2_dev or zng_rocm_deflate_dev write -- needs an INDEX: access points {in_bit, out_off, window_len}, each a
 * block start (bit in_bit of the file), the plaintext offset of its first byte, and the window_len = min(32768, out_off)
 * bytes in front of it, which the index keeps in device memory.  The SPAN of point k is the plaintext [out_off_k,
 * out_off_(k+1)), the last span ends at plain_len; decoding can resume at any point with nothing but its window.
 *
 * zng_rocm_inflate_index_build_dev: zng_rocm_uncompress_large_dev(format, d_src, src_len, NULL, 0, d_dst, dst_cap, out_len,
 * in_used, piece_bytes, flags, stream) plus an index (no preset dictionary).  The return value, *out_len, *in_used, the
 * bytes at d_dst, the zng_rocm_last_error() text and the zng_rocm_inflate_large_last_* counters are that call's for the same
 * arguments.  An index exists only on return value 1; on any other return (a zlib member with FDICT returns 2) *out = NULL.
 * A multi-member gzip file is indexed up to the end of its first member (*in_used).  span_bytes: the least plaintext between
 * two points, 0 (= 1 MiB) or 64 KiB .. 1 GiB; anything else, or out == NULL, is ZNG_ROCM_EINVAL with nothing launched and no
 * device byte written.
 * What happens: while the stream is decoded, the pieces loop notes the block starts it meets -- every part of a device pass
 * that begins at a block start, every block start between two pieces, the block ends the sequential decoder delivers -- with
 * their plaintext offsets.  Point 0 is always {8 * header_len, 0, 0}; walking the starts in stream order, one becomes a point
 * when its out_off is at least span_bytes past the last point and in front of plain_len.  A stream only the sequential decoder
 * handles (below 128 KiB compressed, for one) has point 0 alone: correct, and a read of it decodes from the start.  One
 * kernel, one workgroup per point, then copies all windows out of d_dst into memory the index owns.  Synchronous.
 * The index is immutable; zng_rocm_inflate_index_points copies up to `cap` points to `pts` (may be NULL) and returns their
 * number; zng_rocm_inflate_index_destroy frees it (before zng_rocm_shutdown()).
 *
 * zng_rocm_inflate_index_read_dev: MANY plaintext ranges [uoff, uoff + len) in one set of launches, decoding only the spans
 * the ranges touch.  d_src / src_len: the file the index was built from.  Checked before anything is launched: idx and the
 * buffers are not null, every point of the index begins inside src_len (a file that ends in front of the last point is not
 * the indexed one; a file that is merely cut behind it is read as far as it goes), no range has a null d_dst with a non-zero
 * len, scratch_bytes is 0 (= 256 MiB) or 1 MiB .. 4 GiB.  Any violation is ZNG_ROCM_EINVAL with no range field or
 * destination byte written.  A range is clipped to plain_len: uoff >= plain_len gives status 1 with out_len 0.
 * What happens: a span that lies wholly inside a range is ONE job of the one-wavefront engine in its span form, decoded
 * straight to d_dst + (out_off_k - uoff) with the span's length as capacity: it starts at bit in_bit & 7 of byte in_bit >> 3
 * with in_len = min(src_len - (in_bit >> 3), 2^31 - 1), its history is the point's own window (a distance that reaches in
 * front of it is "invalid distance too far back": a damaged file never reads outside a window), and it ends where its output
 * reaches the capacity, at a block end or inside a block.  A span a range only cuts (an edge: a range has at most two) is
 * decoded once per round into a scratch slot, however many ranges of the round cut it, and only as far as the furthest of
 * them needs; behind the engine on the same stream one kernel copies each range's slice, one workgroup each -- only from a
 * job that ended with status 1 and produced exactly its capacity -- with 16-byte vector stores and byte steps at head and
 * tail, for every pair of alignments.  One launch of each kernel, one readback and one synchronisation per round.  Ranges
 * are taken in order until the edge slots of a round would pass scratch_bytes; a range is never split, so a range whose own
 * edge slots are larger is a round of its own.  A span of 2 GiB and more of plaintext is not this engine's: a range that
 * touches one gets status -5 with msg "span too long for the one-wavefront engine".
 * Per range (fields as zng_rocm_bgzf_range): status 1, out_len = the clipped length; status -3 with the engine's text for
 * the FIRST failing span of the range ("invalid block type", "invalid distance too far back", ..., or "index does not match
 * the stream" when the stream ended in front of the span's end); status -5 when that span was starved of input.  On failure
 * out_len = the bytes of the range in front of the first failing span's part; an edge span that failed has written nothing
 * to d_dst.  Nothing outside [d_dst, d_dst + len) of any range is ever written, and one range's failure does not change
 * another's result.
 * NO CHECK VALUE: a partial read has none to compare.  A read verifies the deflate structure of what it decodes and the
 * length it produces, nothing else -- the build verified Adler-32 / CRC-32 and ISIZE of the whole member once.
 * Returns 0, or the first device error.  Synchronous.  The three counters are thread-local: spans put through the engine, of
 * those the spans decoded straight into a destination, rounds.
 *
 * zng_rocm_inflate_index_export / _import_dev: the index as one little-endian blob in HOST memory (one device-to-host copy of
 * the windows, one copy back):
 *   0   u32 magic "ZRIX"   4  u32 version (1)   8  u32 format   12  u32 0
 *   16  u64 header_len     24 u64 src_end (*in_used of the build: the indexed member's end)   32  u64 plain_len
 *   40  u64 span_bytes     48 u64 npoints
 *   56  npoints rows of 24 bytes: u64 in_bit, u64 out_off, u32 window_len, u32 0
 *   then the windows, point 0's first, each at its real length
 * export: *need is always set; cap < *need returns -5 with nothing written.  import checks, before any allocation: magic and
 * version, format, span_bytes, point 0 = {8 * header_len, 0, 0}, in_bit ascending, out_off ascending and below plain_len,
 * window_len == min(32768, out_off), the reserved words, every point at or in front of src_end, and that the size is exactly
 * header + rows + windows.  Anything else is ZNG_ROCM_EINVAL with *out = NULL. */
typedef struct zng_rocm_inflate_index zng_rocm_inflate_index;        /* opaque; immutable once built */
typedef struct zng_rocm_access_point {
    uint64_t in_bit;         /* bit of the file where a deflate block begins */
    uint64_t out_off;        /* plaintext offset of its first byte */
    uint32_t window_len;     /* min(32768, out_off): bytes of history the index keeps for it */
    uint32_t reserved;       /* 0 */
} zng_rocm_access_point;
typedef struct zng_rocm_inflate_range {           /* same fields and meaning as zng_rocm_bgzf_range */
    uint64_t    uoff;
    uint64_t    len;
    uint8_t    *d_dst;
    /* out */
    int         status;
    uint64_t    out_len;
    const char *msg;
} zng_rocm_inflate_range;
int      zng_rocm_inflate_index_build_dev(int format, const uint8_t *d_src, size_t src_len, uint8_t *d_dst, size_t dst_cap,
                                          uint64_t *out_len, size_t *in_used, uint64_t span_bytes, size_t piece_bytes,
                                          uint32_t flags, zng_rocm_inflate_index **out, void *stream);
int      zng_rocm_inflate_index_read_dev(const zng_rocm_inflate_index *idx, const uint8_t *d_src, size_t src_len,
                                         zng_rocm_inflate_range *ranges, size_t nranges, size_t scratch_bytes, void *stream);
size_t   zng_rocm_inflate_index_points(const zng_rocm_inflate_index *idx, zng_rocm_access_point *pts, size_t cap);
uint64_t zng_rocm_inflate_index_plain_len(const zng_rocm_inflate_index *idx);
int      zng_rocm_inflate_index_export(const zng_rocm_inflate_index *idx, uint8_t *buf, size_t cap, size_t *need, void *stream);
int      zng_rocm_inflate_index_import_dev(const uint8_t *buf, size_t len, zng_rocm_inflate_index **out, void *stream);
void     zng_rocm_inflate_index_destroy(zng_rocm_inflate_index *idx);
int      zng_rocm_inflate_index_read_last_decoded(void);   /* thread-local: spans put through the engine */
int      zng_rocm_inflate_index_read_last_direct(void);    /* of those, spans decoded straight into a destination */
int      zng_rocm_inflate_index_read_last_rounds(void);

/* ONE raw stream with its host decode spread over `nthreads` threads (zng_rocm_inflate_tokens_decode_threads) and one
 * device pass; same results and status as zng_rocm_inflate_raw_window, which it falls back to for streams that
 * offer no block boundary to cut at or turn out irregular.  Synchronous. */
int  zng_rocm_inflate_raw_threads(const uint8_t *src, size_t src_len, const uint8_t *d_window, uint32_t window_len,
                                  uint8_t *d_dst, size_t dst_cap, uint64_t *out_len, size_t *in_used, int nthreads);

/* ---- compress2 / uncompress2 class front ends (compress.c:31-98, uncompr.c:25-76) ---------------------
 * `format`: 0 = raw deflate, 1 = zlib (RFC 1950), 2 = gzip (RFC 1952).  The trailer checksum (Adler-32 /
 * CRC-32 + ISIZE) is computed by the device checksum kernel over the device-resident plaintext.
 * compress2_dev:   d_src (device) -> d_dst (device, *dst_len >= zng_rocm_compress_bound()); level as compress2:
 *                  -1 = 6, 0 = stored blocks, 1..9 as zng_rocm_deflate_dev, anything else Z_STREAM_ERROR (-2,
 *                  deflate.c:318-320); the zlib FLEVEL / gzip XFL hints are those of the requested level
 *                  (deflate.c:868-885, :913).  Returns Z_OK (0) / Z_BUF_ERROR (-5) / error.
 *                  Many streams in one asynchronous call: zng_rocm_compress_streams2_dev / zng_rocm_compress_members_dev.
 * uncompress2_dev: src (HOST, the sequential bitstream stays on the host) -> d_dst (device).  On return *dst_len
 *                  = plaintext bytes, *src_len = input bytes consumed.  Z_OK, Z_BUF_ERROR (destination too small),
 *                  Z_DATA_ERROR with the reference's message text in zng_rocm_last_error() ("incorrect header
 *                  check", "header crc mismatch" (gzip FHCRC, inflate.c:686-692), "incorrect data check",
 *                  "incorrect length check", decoder messages, incomplete stream).
 * compress2_index_dev: compress2_dev that also hands back a zng_rocm_inflate_index (above) of the stream it writes -- taken from
 *                  what the compressor knows, with no byte of the stream decoded and no plaintext-sized scratch.  The bytes at
 *                  d_dst, *dst_len and the return value are compress2_dev's for the same d_src, src_len, level, format (level
 *                  -1 and 0..9, formats 0/1/2), and so are the does-not-fit (-5), bad-level (-2) and ZNG_ROCM_ENODEV answers
 *                  with their zng_rocm_last_error() texts.  span_bytes as zng_rocm_inflate_index_build_dev: 0 (= 1 MiB) or
 *                  64 KiB .. 1 GiB; anything else, or out == NULL, is ZNG_ROCM_EINVAL before any other check, with nothing
 *                  launched, no device byte written, *dst_len untouched and *out = NULL (when out is given); after that the
 *                  checks run in compress2_dev's order.  An index exists only on return 0; on every other return *out = NULL
 *                  and *dst_len is untouched.  Its head is {format, header_len = 0 / 2 / 10, src_end = *dst_len, plain_len =
 *                  src_len, span_bytes}; it is an ordinary index for _read_dev, _points, _plain_len, _export (blob version
 *                  1), _import_dev and _destroy.
 *                  The points: every block of the stream is a candidate {bit of the file where it begins, plaintext offset of
 *                  its first byte}, in stream order.  Levels 1..9: one kernel behind the compressor's own, one thread per
 *                  block of the engine (a block per 61440 positions, each ending on a byte boundary), writes the block's byte
 *                  in the deflate data and the first byte it codes -- its first position if a token starts there, otherwise
 *                  the next token start -- and these 16 bytes per block come down with the compressed size, before the
 *                  windows are gathered.  Level 0: stored block j is {8 * (header_len + 65540 * j), 65535 * j}, worked out on
 *                  the host.  Point 0 is {8 * header_len, 0, 0}; walking the candidates, one becomes a point when its out_off
 *                  is at least span_bytes past the last point and in front of src_len.  The windows, min(32768, out_off)
 *                  bytes each, are gathered from the PLAINTEXT d_src into memory the index owns.
 *                  THE BOUND no decode-built index gives: neighbouring candidates are at most 61440 + 257 plaintext bytes
 *                  apart (65535 at level 0), so for every k   out_off[k + 1] - out_off[k] < span_bytes + 65536   and
 *                  plain_len - out_off[last] < span_bytes + 65536: a read never decodes more than that in front of its range,
 *                  however well the data compresses.
 *                  At most one host synchronisation more than compress2_dev makes (the window gather's).  Synchronous.  One
 *                  stream below 4 GiB, strategy 0, windowBits 15, as compress2_dev. */
size_t zng_rocm_compress_bound(size_t source_len, int format);
int    zng_rocm_compress2_dev(uint8_t *d_dst, size_t *dst_len, const uint8_t *d_src, size_t src_len, int level,
                              int format, void *stream);
int    zng_rocm_compress2_index_dev(uint8_t *d_dst, size_t *dst_len, const uint8_t *d_src, size_t src_len, int level, int format,
                                    uint64_t span_bytes, zng_rocm_inflate_index **out, void *stream);
int    zng_rocm_uncompress2_dev(uint8_t *d_dst, size_t *dst_len, const uint8_t *src, size_t *src_len, int format,
                                void *stream);

/* ---- the coarse boundary: what DEFLATE_HOOK / INFLATE_TYPEDO_HOOK call ---------------------------------------
 * A `zng_rocm_hook` is the content of an arch/rocm backend's arch_deflate_state / arch_inflate_state
 * (deflate.h:319-321, inflate.h:160-162; precedent arch/s390/dfltcc_common.h): the stream's 32 KiB of history in
 * device memory, a bounded staging buffer, a HIP stream of its own.  Host pointers in and out -- zng_stream's next_in /
 * next_out are the caller's memory (SURVEY.md 8b "Ownership").  The reference-side adapter that keeps next_in /
 * avail_in / next_out / avail_out / total_* / adler and answers need_more / block_done / finish_started /
 * finish_done (deflate.h:336-341, deflate.c:1039-1083) is integration/arch/rocm/rocm_deflate.c, rocm_inflate.c.
 * Every function returns ZNG_ROCM_ENODEV after a zng_rocm_shutdown() (the adapter then continues in software). */
typedef struct zng_rocm_hook zng_rocm_hook;
int    zng_rocm_hook_create(zng_rocm_hook **h, size_t block_bytes);       /* ENODEV without a device */
void   zng_rocm_hook_destroy(zng_rocm_hook *h);
int    zng_rocm_hook_reset(zng_rocm_hook *h);                             /* forget the history: deflateResetKeep (deflate.c:567), Z_FULL_FLUSH (deflate.c:1073-1080), inflateResetKeep */
/* deflateSetDictionary / inflateSetDictionary (deflate.c:456-531, inflate.c:1214-1261): the last 32 KiB become the history */
int    zng_rocm_hook_set_history(zng_rocm_hook *h, const uint8_t *dict, uint32_t len);
/* deflateGetDictionary / inflateGetDictionary (deflate.c:521-545, inflate.c:1195-1212): dict may be NULL (length only) */
int    zng_rocm_hook_get_history(zng_rocm_hook *h, uint8_t *dict, uint32_t *len);
/* deflateCopy / inflateCopy (deflate.c:1131-1181, inflate.c:1379-1413): both memcpy the state block, which is enough for
 * DFLTCC's plain-data arch block and not for one that owns a hook.  *out = a new hook with a HIP stream, check words and
 * staging of its own and the source's history, copied device to device behind everything already enqueued on the source's
 * stream and complete when the call returns: source and clone share nothing and may be used and destroyed in either order.
 * The clone has the default block room, not what the source's buffers have grown to (they grow on first use, as any
 * hook's).  The plaintext the source's last zng_rocm_hook_inflate* call handed out is NOT part of the clone: it is hook
 * memory, valid until the next call, and whoever copies a stream with some of it undelivered copies it himself
 * (rocm_inflate.c).  ZNG_ROCM_EINVAL for a null argument, ZNG_ROCM_ENODEV before zng_rocm_init() or for a source from before
 * a zng_rocm_shutdown(), ZNG_ROCM_ENOMEM / ZNG_ROCM_EHIP otherwise; *out = NULL on every failure, the source untouched always. */
int    zng_rocm_hook_clone(const zng_rocm_hook *src, zng_rocm_hook **out);
size_t zng_rocm_hook_deflate_bound(size_t in_len);
/* One block of the stream: `in` (host) is compressed at `level` (0..9, as zng_rocm_deflate_block_dev) against the
 * history, the block lands at `out` (host, out_cap >= zng_rocm_hook_deflate_bound(in_len)) and always ends on a byte
 * boundary; flags = ZNG_ROCM_BLOCK_*; the input becomes history.  check: 0 none, 1 Adler-32, 2 CRC-32 of `in`,
 * continuing *check_value (what DEFLATE_NEED_CHECKSUM = 0 leaves to the backend, deflate.c:1197-1212). */
int    zng_rocm_hook_deflate_block(zng_rocm_hook *h, int level, const uint8_t *in, size_t in_len, uint32_t flags, int check,
                                   uint32_t *check_value, uint8_t *out, size_t out_cap, size_t *out_len);
/* the same block at zlib's `strategy` (0..4, as zng_rocm_deflate_strategy_block_dev; the strategy may change from one
 * block to the next, as deflateParams allows); history, check value and flags as above */
int    zng_rocm_hook_deflate_block_strategy(zng_rocm_hook *h, int level, int strategy, const uint8_t *in, size_t in_len,
                                            uint32_t flags, int check, uint32_t *check_value, uint8_t *out, size_t out_cap,
                                            size_t *out_len);
/* the same block for a stream opened with windowBits `window_bits` (9..15, as zng_rocm_deflate_window_block_dev; the reference
 * has turned 8 into 9 before a hook sees it, deflate.c:322-323; anything else is ZNG_ROCM_EINVAL).  At 15 it gives the bytes of
 * the call above.  The hook keeps 32 KiB of history whatever the window; deflateGetDictionary's at-most-w_size rule
 * (deflate.c:523-527) is the adapter's (rocm_deflate.c) */
int    zng_rocm_hook_deflate_block_window(zng_rocm_hook *h, int level, int strategy, int window_bits, const uint8_t *in,
                                          size_t in_len, uint32_t flags, int check, uint32_t *check_value, uint8_t *out,
                                          size_t out_cap, size_t *out_len);
/* A complete raw deflate stream (or the rest of one) at `in`, continuing the history: returns 1 (Z_STREAM_END) with the
 * plaintext at *out (host memory owned by the hook, valid until its next call), *out_len, *in_used and the check of the
 * plaintext; -5 when the stream does not end inside in_len (nothing consumed: the adapter gathers more input);
 * -3 (Z_DATA_ERROR) with the reference's strm->msg text in *msg; negative ZNG_ROCM_E* on a device failure. */
int    zng_rocm_hook_inflate(zng_rocm_hook *h, const uint8_t *in, size_t in_len, int check, uint32_t *check_value,
                             const uint8_t **out, size_t *out_len, size_t *in_used, const char **msg);
/* Streaming form of zng_rocm_hook_inflate: `in` (host) holds the stream from the byte that contains bit `start_bit`
 * (0..7) on.  Every complete block is decoded against the history and becomes history; *out / *out_len = its plaintext
 * (hook memory, valid until the next call), check continues *check_value over it.  Returns 1 / 0 / -3 with *end_bit as
 * zng_rocm_inflate_tokens_decode_blocks; negative ZNG_ROCM_E* = device failure, nothing produced, history unchanged.
 * in_len == 0 returns 0 with *end_bit = start_bit and no launch.  A refused argument returns ZNG_ROCM_EINVAL, which has
 * the value of Z_DATA_ERROR but leaves *msg NULL (a data error always sets it).  From 4 MiB of input on the blocks are
 * decoded in parts on the device (as zng_rocm_hook_inflate). */
int    zng_rocm_hook_inflate_blocks(zng_rocm_hook *h, const uint8_t *in, size_t in_len, unsigned start_bit, int check,
                                    uint32_t *check_value, const uint8_t **out, size_t *out_len, uint64_t *end_bit,
                                    const char **msg);

/* ---- measurement hooks --------------------------------------------------
 * Between trace_begin and trace_end every (sampled) launch of the DOMINANT kernel of a *_dev entry point (the
 * streaming kernel, not its finalize step) carries a pair of HIP events attached to its own dispatch
 * (hipExtLaunchKernelGGL): the start / stop timestamps of the kernel itself, the quantity rocprofv3
 * --kernel-trace reports, with no additional packets in the stream.  trace_end synchronises, writes the
 * per-launch durations (ms) into `ms_out` (up to `cap`) and returns how many launches were recorded
 * (negative = error).  Used by bench.py for the roofline figure; no reference counterpart (the reference
 * measures with Google Benchmark, test/benchmarks/). */
int zng_rocm_trace_begin(int max_launches);
int zng_rocm_trace_end(float *ms_out, int cap);
/* Time only every n-th marked launch (n >= 1; 1 = all, the default): a timed loop can sample its kernel instead of
 * attaching events to every step.  Takes effect at the next zng_rocm_trace_begin(). */
int zng_rocm_trace_stride(int n);

#ifdef __cplusplus
}
#endif
#endif /* ZNG_ROCM_H */
