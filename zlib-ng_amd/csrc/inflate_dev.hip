// inflate_dev.hip -- slot `inflate_fast` (inffast_tpl.h:53-318) together with the block decoding around it
// (inflate.c:735-917: stored / fixed / dynamic block headers, inftrees.c:32-297 table construction) as ONE device
// kernel for MANY independent raw deflate streams that are already in device memory -- the shape of the reference's
// many-stream model (test/pigz/CMakeLists.txt:123-200) on the decode side, and the inverse of
// zng_rocm_deflate_quick_dev: compress on the device, decompress on the device, nothing crosses PCIe.
//
// One wavefront per stream.  A deflate stream is a serial bit parse, so the parse itself is wave-UNIFORM work: the
// bit buffer, the table entry, the position all live in scalar registers (every lane would compute the same), and the
// 64 lanes are used where the stream offers width:
//   * the compressed words are fetched 64 at a time (one dword per lane, the next 64 prefetched) and handed to the
//     bit buffer with v_readlane -- the parse never waits on a memory load;
//   * Huffman tables are built lane-parallel (counting sort by ballots, one table entry per lane per pass);
//   * a match copy moves up to 64 bytes per pass, a stored block 1 KiB per pass;
//   * the last kRing output bytes live in an LDS ring (the device form of inflate's sliding window, inflate.c:325-378):
//     literals and near matches never touch HBM, the ring leaves in aligned 16-byte stores, and only a match that
//     reaches further back than the ring reads its source from HBM (the stream's own earlier output, or the
//     dictionary / previous window that precedes `out`).
// This kernel scales with the NUMBER of streams; ONE large stream is cut into parts at block starts found on the device
// and every part is a job of this kernel in part mode (inflate_large.hip).  The decode loop itself is hand-written
// (ZR_INFLATE_FAST_LOOP below).
//
// Status and messages are the reference's (inflate.c strm->msg texts, via zng_rocm_inflate_message).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "context.h"
#include "deflate_dev.h"
#include "inflate_dev.h"

namespace zr {

// Diagnostic builds (-DZR_INFLATE_BOUNDS, tools/micro/inflate_bounds.sh): every index the table builder computes from
// stream data is checked against the array it goes into; a violation is counted (zng_rocm_debug_inflate_bounds()) and the
// index clamped.  Round 2's aperture violation was traced to addressing, not to an index; this build is the
// evidence that no index leaves its array on the mutated-stream corpus either.
// Diagnostic builds (-DZR_INFLATE_STATS, tools/micro/inflate_stats.sh): how often the hand-written loop hands a symbol to the
// general code, and why (zng_rocm_debug_inflate_stats()).
#ifdef ZR_INFLATE_STATS
__device__ unsigned long long g_inflate_stats[16];
__device__ unsigned long long g_inflate_span[2 * 16384];         // per job (the first 16384): s_memtime at its start and end
#ifdef ZR_INFLATE_STATS_EXITS
#define ZR_STAT(i) do { if (lane == 0) atomicAdd(&g_inflate_stats[i], 1ull); } while (0)
#else
#define ZR_STAT(i) do { } while (0)
#endif
#else
#define ZR_STAT(i) do { } while (0)
#endif
#ifdef ZR_INFLATE_BOUNDS
__device__ unsigned int g_inflate_bounds_violations;
__device__ __forceinline__ uint32_t zr_idx(uint32_t i, uint32_t n) {
    if (i < n) return i;
    atomicAdd(&g_inflate_bounds_violations, 1u);
    return 0;
}
#define ZR_IDX(i, n) zr_idx((uint32_t)(i), (uint32_t)(n))
#else
#define ZR_IDX(i, n) (i)
#endif

}  // namespace zr

#include "inflate_tables.h"     // table entries, LDS layouts, build_code, long_code

namespace zr {


// The decode loop's fast paths, hand-written (inffast_tpl.h:151-226 is the loop this stands for).  The parse is
// wave-uniform and serial: it runs on the CU's one scalar unit, a wave gets an instruction issued every four or five
// cycles, and a CU holds at most 16 streams (LDS) -- so what counts is the NUMBER of instructions and taken branches per
// symbol.  The compiler's version of this loop spent 27 scalar instructions on a literal and about 80 on a match, most of
// them carrying loop-exit conditions around as lane masks; here a root-table literal costs 7 and a short copy about 40.
// The loop handles, per symbol:
//   * a refill of the bit buffer from the 64 fetched words (it leaves when the 64 are used up);
//   * a literal whose code fits the root table: into the waiting run (`lit`, literal j in lane j);
//   * a length symbol whose code fits the root table + a distance whose code fits its root table, when the copy is one of
//     the common shapes and nothing else is due (op + len <= oplim: room in `out`, no flush; 64 per pass): source in the
//     ring without overlap (dist <= kNear, dist >= len), source already flushed (dist > kNear: read back from HBM), or
//     -- parts only -- source in front of the part (ZR_INFLATE_BEFORE_PART).
// Anything else leaves the loop with `stage` = what has been consumed of the next symbol: 0 nothing, 1 the length (`len`
// valid), 2 length and distance (`len`, `dist` valid); the C++ code below finishes that symbol in full generality and
// comes back.  Positions: `opb` is the position of the first waiting literal, op = opb + npend.
// (A variant that looked both tables up at 64 bit offsets at once -- lane j with the buffer shifted by j, the next
// symbol's entry then a v_readlane away -- removed two of three table accesses and was no faster for one wave and 12 %
// slower for 16 per CU: the accesses are not what a symbol waits for.)
// Hazards (the assembler inserts no wait states into inline asm): on gfx950 a VALU write of an SGPR/VCC needs two
// instructions before a VALU reads it -- the v_cmp / masked-operation pairs below are spaced accordingly; LDS operations
// of one wave execute in order, so a ds_read after a ds_write of the same bytes needs no wait.
#define ZR_INFLATE_FAST_LOOP(RD, WR, GL, BEFORE, WLIM)                                                                     \
    "s_mov_b32 s43, 0\n\t"                                                                                             \
    /* Inside the loop the two counters the literal path tests live BIASED, so that the instruction that updates them    \
       sets SCC and no compare is needed (the scalar unit is what sixteen streams per CU share): cnt as cnt - 32 (a       \
       borrow = fewer than 32 bits left), npend as npend - 64 (a carry = the run is full), with opb + 64 and lane - 64   \
       beside it.  The C++ around the statement converts. */                                                          \
    "L_top_%=:\n\t"                                                                                                    \
    "s_cmp_lt_i32 %[cnt], 0\n\t"                                                                                       \
    "s_cbranch_scc0 L_look_%=\n\t"                                                                                     \
    "L_refill_%=:\n\t"                                                                                                 \
    "s_cmp_eq_u32 %[widx], " WLIM "\n\t"                                                                              \
    "s_cbranch_scc1 L_exit0_%=\n\t"                                                                                    \
    "v_readlane_b32 s42, %[cur], %[widx]\n\t"                                                                          \
    "s_add_u32 %[widx], %[widx], 1\n\t"                                                                                \
    "s_add_u32 %[t0], %[cnt], 32\n\t"                                                                                  \
    "s_lshl_b64 s[44:45], s[42:43], %[t0]\n\t"                                                                         \
    "s_or_b64 s[40:41], s[40:41], s[44:45]\n\t"                                                                        \
    "s_add_u32 %[cnt], %[cnt], 32\n\t"                                                                                 \
    "L_look_%=:\n\t"                                                                                                   \
    "v_bfe_u32 %[va], s40, 0, %[litroot]\n\t"                                                                          \
    "v_lshl_add_u32 %[va], %[va], 1, %[litb]\n\t"                                                                      \
    "ds_read_u16 %[vb], %[va]\n\t"                                                                                     \
    "v_cmp_eq_u32 vcc, %[npend], %[laneb]\n\t"                                                                         \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                         \
    "v_readfirstlane_b32 %[e], %[vb]\n\t"                                                                              \
    "v_lshrrev_b32 %[vb], 4, %[vb]\n\t"                                                                                \
    "s_cmpk_gt_u32 %[e], 0xfff\n\t"                                                                                    \
    "s_cbranch_scc1 L_notlit_%=\n\t"                                                                                   \
    "s_and_b32 %[t0], %[e], 15\n\t"                                                                                    \
    "v_cndmask_b32 %[lit], %[lit], %[vb], vcc\n\t"                                                                     \
    "s_lshr_b64 s[40:41], s[40:41], %[t0]\n\t"                                                                         \
    "s_add_u32 %[npend], %[npend], 1\n\t"                                                                              \
    "s_cbranch_scc1 L_full_%=\n\t"                                                                                     \
    "s_sub_u32 %[cnt], %[cnt], %[t0]\n\t"                                                                              \
    "s_cbranch_scc0 L_look_%=\n\t"                                                                                     \
    "s_branch L_refill_%=\n\t"                                                                                         \
    "L_full_%=:\n\t"                                                                                                   \
    "s_sub_u32 %[cnt], %[cnt], %[t0]\n\t"                                                                              \
    "s_branch L_exit0_%=\n\t"                                                                                          \
    "L_notlit_%=:\n\t"                                                                                                 \
    /* e - 0x1010 = code length | (symbol - 257) << 4; symbols 257..285 only (256, 286.., the long and bad marks leave) */ \
    "s_sub_u32 %[t1], %[e], 0x1010\n\t"                                                                                \
    "s_cmpk_gt_u32 %[t1], 0x1cf\n\t"                                                                                   \
    "s_cbranch_scc1 L_exit0_%=\n\t"                                                                                    \
    "s_and_b32 %[t0], %[e], 15\n\t"                                                                                    \
    "s_lshr_b32 %[t1], %[t1], 4\n\t"                                                                                   \
    "s_lshr_b64 s[40:41], s[40:41], %[t0]\n\t"                                                                         \
    "s_sub_u32 %[cnt], %[cnt], %[t0]\n\t"                                                                              \
    "s_add_u32 %[len], %[t1], 3\n\t"                                                                                   \
    "s_cmp_lt_u32 %[t1], 8\n\t"                                                                                        \
    "s_cbranch_scc1 L_havelen_%=\n\t"                                                                                  \
    "s_movk_i32 %[len], 258\n\t"                                                                                       \
    "s_cmp_eq_u32 %[t1], 28\n\t"                                                                                       \
    "s_cbranch_scc1 L_havelen_%=\n\t"                                                                                  \
    "s_sub_u32 %[t0], %[t1], 4\n\t"                                                                                    \
    "s_lshr_b32 %[t0], %[t0], 2\n\t"                                                                                   \
    "s_and_b32 %[t1], %[t1], 3\n\t"                                                                                    \
    "s_or_b32 %[t1], %[t1], 4\n\t"                                                                                     \
    "s_lshl_b32 %[t1], %[t1], %[t0]\n\t"                                                                               \
    "s_bfm_b32 %[len], %[t0], 0\n\t"                                                                                   \
    "s_and_b32 %[len], %[len], s40\n\t"                                                                                \
    "s_add_u32 %[len], %[len], %[t1]\n\t"                                                                              \
    "s_add_u32 %[len], %[len], 3\n\t"                                                                                  \
    "s_lshr_b64 s[40:41], s[40:41], %[t0]\n\t"                                                                         \
    "s_sub_u32 %[cnt], %[cnt], %[t0]\n\t"                                                                              \
    "L_havelen_%=:\n\t"                                                                                                \
    "s_cmp_lt_i32 %[cnt], 0\n\t"                                                                                       \
    "s_cbranch_scc0 L_dist_%=\n\t"                                                                                     \
    "s_cmp_eq_u32 %[widx], " WLIM "\n\t"                                                                              \
    "s_cbranch_scc1 L_exit1_%=\n\t"                                                                                    \
    "v_readlane_b32 s42, %[cur], %[widx]\n\t"                                                                          \
    "s_add_u32 %[widx], %[widx], 1\n\t"                                                                                \
    "s_add_u32 %[t0], %[cnt], 32\n\t"                                                                                  \
    "s_lshl_b64 s[44:45], s[42:43], %[t0]\n\t"                                                                         \
    "s_or_b64 s[40:41], s[40:41], s[44:45]\n\t"                                                                        \
    "s_add_u32 %[cnt], %[cnt], 32\n\t"                                                                                 \
    "L_dist_%=:\n\t"                                                                                                   \
    "v_bfe_u32 %[va], s40, 0, %[distroot]\n\t"                                                                   \
    "v_lshl_add_u32 %[va], %[va], 2, %[distb]\n\t"                                                                     \
    "ds_read_b32 %[vb], %[va]\n\t"                                                                                     \
    "s_add_u32 %[op], %[opb], %[npend]\n\t"                                                                            \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                         \
    "v_readfirstlane_b32 %[e], %[vb]\n\t"                                                                              \
    "s_cmp_gt_u32 %[e], 0xffffffe0\n\t"                                                                                \
    "s_cbranch_scc1 L_exit1_%=\n\t"                                                                                    \
    "s_and_b32 %[t0], %[e], 15\n\t"                                                                                    \
    "s_bfe_u32 %[t1], %[e], 0x40004\n\t"                                                                               \
    "s_lshr_b64 s[40:41], s[40:41], %[t0]\n\t"                                                                         \
    "s_sub_u32 %[cnt], %[cnt], %[t0]\n\t"                                                                              \
    "s_lshr_b32 %[dist], %[e], 8\n\t"                                                                                  \
    "s_bfm_b32 %[t0], %[t1], 0\n\t"                                                                                    \
    "s_and_b32 %[t0], %[t0], s40\n\t"                                                                                  \
    "s_add_u32 %[dist], %[dist], %[t0]\n\t"                                                                            \
    "s_lshr_b64 s[40:41], s[40:41], %[t1]\n\t"                                                                         \
    "s_sub_u32 %[cnt], %[cnt], %[t1]\n\t"                                                                              \
    /* nothing else due (room in `out`, no flush)? */                                                                 \
    "s_add_u32 %[t1], %[op], %[len]\n\t"                                                                               \
    "s_cmp_gt_u32 %[t1], %[oplim]\n\t"                                                                                 \
    "s_cbranch_scc1 L_exit2_%=\n\t"                                                                                    \
    /* the waiting literals go to the ring: lane j < npend -> position opb + j */                                     \
    "s_cmp_eq_u32 %[npend], 0xffffffc0\n\t"                                                                             \
    "s_cbranch_scc1 L_copy_%=\n\t"                                                                                     \
    "v_cmp_gt_u32 vcc, %[npend], %[laneb]\n\t"                                                                          \
    "s_add_u32 %[e], %[opb], %[a0m]\n\t"                                                                               \
    "v_add_u32 %[va], %[e], %[lane]\n\t"                                                                               \
    "v_and_b32 %[va], %[mask], %[va]\n\t"                                                                              \
    "v_lshl_add_u32 %[va], %[va], %[sh], %[ringb]\n\t"                                                                 \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    WR " %[va], %[lit]\n\t"                                                                                            \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "s_add_u32 %[opb], %[op], 64\n\t"                                                                                   \
    "s_mov_b32 %[npend], 0xffffffc0\n\t"                                                                               \
    "L_copy_%=:\n\t"                                                                                                   \
    /* destination: ring slot of op + lane, lanes below len */                                                        \
    "v_cmp_gt_u32 vcc, %[len], %[lane]\n\t"                                                                            \
    "s_add_u32 %[e], %[op], %[a0]\n\t"                                                                                 \
    "v_add_u32 %[va], %[e], %[lane]\n\t"                                                                               \
    "v_subrev_u32 %[vb], %[dist], %[va]\n\t"                                                                           \
    "v_and_b32 %[va], %[mask], %[va]\n\t"                                                                              \
    "v_lshl_add_u32 %[va], %[va], %[sh], %[ringb]\n\t"                                                                 \
    "s_cmp_gt_u32 %[dist], %[op]\n\t"                                                                                  \
    "s_cbranch_scc1 L_before_%=\n\t"                                                                                   \
    "s_cmp_gt_u32 %[dist], %[near]\n\t"                                                                                \
    "s_cbranch_scc1 L_far_%=\n\t"                                                                                      \
    "s_cmp_lt_u32 %[dist], %[len]\n\t"                                                                                 \
    "s_cbranch_scc1 L_overlap_%=\n\t"                                                                                  \
    /* source in the ring; no overlap, or a distance of 64 and more (every pass of 64 then reads what is already there: \
       LDS operations of one wave execute in order) */                                                                \
    "L_plain_%=:\n\t"                                                                                                  \
    "v_and_b32 %[vb], %[mask], %[vb]\n\t"                                                                              \
    "v_lshl_add_u32 %[vb], %[vb], %[sh], %[ringb]\n\t"                                                                 \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    RD " %[vb], %[vb]\n\t"                                                                                             \
    "s_add_u32 %[opb], %[opb], %[len]\n\t"                                                                             \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                         \
    WR " %[va], %[vb]\n\t"                                                                                             \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "s_cmp_gt_u32 %[len], 64\n\t"                                                                                      \
    "s_cbranch_scc1 L_nearmore_%=\n\t"                                                                                 \
    "s_branch L_top_%=\n\t"                                                                                            \
    /* 65 .. 258: the other chunks of 64 (no overlap: the chunks are independent of each other) */                    \
    "L_nearmore_%=:\n\t"                                                                                               \
    "s_mov_b32 %[t1], 64\n\t"                                                                                          \
    "L_nearloop_%=:\n\t"                                                                                               \
    "s_sub_u32 %[t0], %[len], %[t1]\n\t"                                                                               \
    "v_cmp_gt_u32 vcc, %[t0], %[lane]\n\t"                                                                             \
    "s_add_u32 %[e], %[op], %[a0]\n\t"                                                                                 \
    "s_add_u32 %[e], %[e], %[t1]\n\t"                                                                                  \
    "v_add_u32 %[va], %[e], %[lane]\n\t"                                                                               \
    "v_subrev_u32 %[vb], %[dist], %[va]\n\t"                                                                           \
    "v_and_b32 %[va], %[mask], %[va]\n\t"                                                                              \
    "v_and_b32 %[vb], %[mask], %[vb]\n\t"                                                                              \
    "v_lshl_add_u32 %[va], %[va], %[sh], %[ringb]\n\t"                                                                 \
    "v_lshl_add_u32 %[vb], %[vb], %[sh], %[ringb]\n\t"                                                                 \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    RD " %[vb], %[vb]\n\t"                                                                                             \
    "s_add_u32 %[t1], %[t1], 64\n\t"                                                                                   \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                         \
    WR " %[va], %[vb]\n\t"                                                                                             \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "s_cmp_lt_u32 %[t1], %[len]\n\t"                                                                                   \
    "s_cbranch_scc1 L_nearloop_%=\n\t"                                                                                 \
    "s_branch L_top_%=\n\t"                                                                                            \
    /* dist < len and dist < 64: the copy repeats the dist bytes in front of it (runs, short periods -- a block of zeros is \
       nothing else).  Lane j of a pass at offset o reads pattern byte (o + j) mod dist from [op - dist, op), which no pass \
       writes: r = j mod dist by six compare-free steps (r = min(r, r - dist * 2^k), unsigned), then r += 64 mod dist per \
       pass. */                                                                                                       \
    "L_overlap_%=:\n\t"                                                                                                \
    "s_cmp_gt_u32 %[dist], 63\n\t"                                                                                     \
    "s_cbranch_scc1 L_plain_%=\n\t"                                                                                    \
    "s_lshl_b32 %[t0], %[dist], 5\n\t"                                                                                 \
    "v_subrev_u32 %[vb], %[t0], %[lane]\n\t"                                                                           \
    "s_lshl_b32 %[t0], %[dist], 4\n\t"                                                                                 \
    "v_min_u32 %[vr], %[vb], %[lane]\n\t"                                                                              \
    "v_subrev_u32 %[vb], %[t0], %[vr]\n\t"                                                                             \
    "s_lshl_b32 %[t0], %[dist], 3\n\t"                                                                                 \
    "v_min_u32 %[vr], %[vb], %[vr]\n\t"                                                                                \
    "v_subrev_u32 %[vb], %[t0], %[vr]\n\t"                                                                             \
    "s_lshl_b32 %[t0], %[dist], 2\n\t"                                                                                 \
    "v_min_u32 %[vr], %[vb], %[vr]\n\t"                                                                                \
    "v_subrev_u32 %[vb], %[t0], %[vr]\n\t"                                                                             \
    "s_lshl_b32 %[t0], %[dist], 1\n\t"                                                                                 \
    "v_min_u32 %[vr], %[vb], %[vr]\n\t"                                                                                \
    "v_subrev_u32 %[vb], %[t0], %[vr]\n\t"                                                                             \
    "v_min_u32 %[vr], %[vb], %[vr]\n\t"                                                                                \
    "v_subrev_u32 %[vb], %[dist], %[vr]\n\t"                                                                           \
    "v_min_u32 %[vr], %[vb], %[vr]\n\t"                                                                                \
    "s_add_u32 %[opb], %[opb], %[len]\n\t"                                                                             \
    "s_nop 0\n\t"                                                                                                      \
    "v_readlane_b32 %[t2], %[vr], 63\n\t"                                                                              \
    "s_mov_b32 %[t1], 0\n\t"                                                                                           \
    "s_add_u32 %[t2], %[t2], 1\n\t"                                                                                    \
    "s_cmp_eq_u32 %[t2], %[dist]\n\t"                                                                                  \
    "s_cselect_b32 %[t2], 0, %[t2]\n\t"                                                                                \
    "L_patloop_%=:\n\t"                                                                                                \
    "s_sub_u32 %[t0], %[len], %[t1]\n\t"                                                                               \
    "v_cmp_gt_u32 vcc, %[t0], %[lane]\n\t"                                                                             \
    "s_add_u32 %[e], %[op], %[a0]\n\t"                                                                                 \
    "s_sub_u32 %[t0], %[e], %[dist]\n\t"                                                                               \
    "s_add_u32 %[e], %[e], %[t1]\n\t"                                                                                  \
    "v_add_u32 %[vb], %[t0], %[vr]\n\t"                                                                                \
    "v_add_u32 %[va], %[e], %[lane]\n\t"                                                                               \
    "v_and_b32 %[vb], %[mask], %[vb]\n\t"                                                                              \
    "v_and_b32 %[va], %[mask], %[va]\n\t"                                                                              \
    "v_lshl_add_u32 %[vb], %[vb], %[sh], %[ringb]\n\t"                                                                 \
    "v_lshl_add_u32 %[va], %[va], %[sh], %[ringb]\n\t"                                                                 \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    RD " %[vb], %[vb]\n\t"                                                                                             \
    "s_add_u32 %[t1], %[t1], 64\n\t"                                                                                   \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                         \
    WR " %[va], %[vb]\n\t"                                                                                             \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "v_add_u32 %[vr], %[t2], %[vr]\n\t"                                                                                \
    "v_subrev_u32 %[vb], %[dist], %[vr]\n\t"                                                                           \
    "s_cmp_lt_u32 %[t1], %[len]\n\t"                                                                                   \
    "v_min_u32 %[vr], %[vb], %[vr]\n\t"                                                                                \
    "s_cbranch_scc1 L_patloop_%=\n\t"                                                                                  \
    "s_branch L_top_%=\n\t"                                                                                            \
    /* source behind the ring's reach: it has been flushed (op - flushed < kFlushAt < kNear - 64), so it is in HBM,   \
       and the flush had its stores acknowledged */                                                                   \
    "L_far_%=:\n\t"                                                                                                    \
    /* up to five passes of 64: ALL their loads first (one address register, instruction offsets 64, 128, ... elements), \
       one wait, then the writes -- a pass at a time this was a memory round trip per 64 symbols, and a block of long     \
       copies at a distance just beyond the ring was the slowest part of a foreign stream */                           \
    "s_sub_u32 %[t0], %[op], %[dist]\n\t"                                                                              \
    "v_add_u32 %[vb], %[t0], %[lane]\n\t"                                                                              \
    "v_lshlrev_b32 %[vb], %[sh], %[vb]\n\t"                                                                            \
    "s_add_u32 %[opb], %[opb], %[len]\n\t"                                                                             \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    GL " %[vd0], %[vb], %[outp]\n\t"                                                                                   \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "s_cmp_gt_u32 %[len], 64\n\t"                                                                                      \
    "s_cbranch_scc0 L_farw_%=\n\t"                                                                                     \
    "s_sub_u32 %[t0], %[len], 64\n\t"                                                                                  \
    "v_cmp_gt_u32 vcc, %[t0], %[lane]\n\t"                                                                             \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    GL " %[vd1], %[vb], %[outp] offset:%[o1]\n\t"                                                                      \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "s_cmp_gt_u32 %[len], 128\n\t"                                                                                     \
    "s_cbranch_scc0 L_farw_%=\n\t"                                                                                     \
    "s_sub_u32 %[t0], %[len], 128\n\t"                                                                                 \
    "v_cmp_gt_u32 vcc, %[t0], %[lane]\n\t"                                                                             \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    GL " %[vd2], %[vb], %[outp] offset:%[o2]\n\t"                                                                      \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "s_cmp_gt_u32 %[len], 192\n\t"                                                                                     \
    "s_cbranch_scc0 L_farw_%=\n\t"                                                                                     \
    "s_sub_u32 %[t0], %[len], 192\n\t"                                                                                 \
    "v_cmp_gt_u32 vcc, %[t0], %[lane]\n\t"                                                                             \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    GL " %[vd3], %[vb], %[outp] offset:%[o3]\n\t"                                                                      \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "s_cmp_gt_u32 %[len], 256\n\t"                                                                                     \
    "s_cbranch_scc0 L_farw_%=\n\t"                                                                                     \
    "s_sub_u32 %[t0], %[len], 256\n\t"                                                                                 \
    "v_cmp_gt_u32 vcc, %[t0], %[lane]\n\t"                                                                             \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    GL " %[vd4], %[vb], %[outp] offset:%[o4]\n\t"                                                                      \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "L_farw_%=:\n\t"                                                                                                   \
    "v_cmp_gt_u32 vcc, %[len], %[lane]\n\t"                                                                            \
    "s_waitcnt vmcnt(0)\n\t"                                                                                           \
    "s_nop 0\n\t"                                                                                                      \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    WR " %[va], %[vd0]\n\t"                                                                                            \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "s_cmp_gt_u32 %[len], 64\n\t"                                                                                      \
    "s_cbranch_scc0 L_top_%=\n\t"                                                                                      \
    "s_sub_u32 %[t0], %[len], 64\n\t"                                                                                  \
    "s_add_u32 %[e], %[e], 64\n\t"                                                                                     \
    "v_cmp_gt_u32 vcc, %[t0], %[lane]\n\t"                                                                             \
    "v_add_u32 %[va], %[e], %[lane]\n\t"                                                                               \
    "v_and_b32 %[va], %[mask], %[va]\n\t"                                                                              \
    "v_lshl_add_u32 %[va], %[va], %[sh], %[ringb]\n\t"                                                                 \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    WR " %[va], %[vd1]\n\t"                                                                                            \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "s_cmp_gt_u32 %[len], 128\n\t"                                                                                     \
    "s_cbranch_scc0 L_top_%=\n\t"                                                                                      \
    "s_sub_u32 %[t0], %[len], 128\n\t"                                                                                 \
    "s_add_u32 %[e], %[e], 64\n\t"                                                                                     \
    "v_cmp_gt_u32 vcc, %[t0], %[lane]\n\t"                                                                             \
    "v_add_u32 %[va], %[e], %[lane]\n\t"                                                                               \
    "v_and_b32 %[va], %[mask], %[va]\n\t"                                                                              \
    "v_lshl_add_u32 %[va], %[va], %[sh], %[ringb]\n\t"                                                                 \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    WR " %[va], %[vd2]\n\t"                                                                                            \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "s_cmp_gt_u32 %[len], 192\n\t"                                                                                     \
    "s_cbranch_scc0 L_top_%=\n\t"                                                                                      \
    "s_sub_u32 %[t0], %[len], 192\n\t"                                                                                 \
    "s_add_u32 %[e], %[e], 64\n\t"                                                                                     \
    "v_cmp_gt_u32 vcc, %[t0], %[lane]\n\t"                                                                             \
    "v_add_u32 %[va], %[e], %[lane]\n\t"                                                                               \
    "v_and_b32 %[va], %[mask], %[va]\n\t"                                                                              \
    "v_lshl_add_u32 %[va], %[va], %[sh], %[ringb]\n\t"                                                                 \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    WR " %[va], %[vd3]\n\t"                                                                                            \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "s_cmp_gt_u32 %[len], 256\n\t"                                                                                     \
    "s_cbranch_scc0 L_top_%=\n\t"                                                                                      \
    "s_sub_u32 %[t0], %[len], 256\n\t"                                                                                 \
    "s_add_u32 %[e], %[e], 64\n\t"                                                                                     \
    "v_cmp_gt_u32 vcc, %[t0], %[lane]\n\t"                                                                             \
    "v_add_u32 %[va], %[e], %[lane]\n\t"                                                                               \
    "v_and_b32 %[va], %[mask], %[va]\n\t"                                                                              \
    "v_lshl_add_u32 %[va], %[va], %[sh], %[ringb]\n\t"                                                                 \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    WR " %[va], %[vd4]\n\t"                                                                                            \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "s_branch L_top_%=\n\t"                                                                                            \
    "L_before_%=:\n\t"                                                                                                 \
    BEFORE                                                                                                             \
    "L_exit2_%=:\n\t"                                                                                                  \
    "s_mov_b32 %[stage], 2\n\t"                                                                                        \
    "s_branch L_end_%=\n\t"                                                                                            \
    "L_exit1_%=:\n\t"                                                                                                  \
    "s_mov_b32 %[stage], 1\n\t"                                                                                        \
    "s_branch L_end_%=\n\t"                                                                                            \
    "L_exit0_%=:\n\t"                                                                                                  \
    "s_mov_b32 %[stage], 0\n\t"                                                                                        \
    "L_end_%=:\n\t"

// a source in front of `out`.  Whole streams: the dictionary -- the general code's business.  Parts: the bytes in front of
// a part are not known yet, the copy writes their NAMES (symbol 256 + 32768 + position, position < 0); done here when the
// whole copy lies in front (a copy that crosses into the part is left to the general code), after the reference's
// "too far back" test and with the furthest reach noted.
#define ZR_INFLATE_BEFORE_STREAM "s_branch L_exit2_%=\n\t"
#define ZR_INFLATE_BEFORE_PART                                                                                         \
    "s_add_u32 %[t1], %[op], %[dictlen]\n\t"                                                                           \
    "s_cmp_gt_u32 %[dist], %[t1]\n\t"                                                                                  \
    "s_cbranch_scc1 L_exit2_%=\n\t"                                                                                    \
    "s_sub_u32 %[t0], %[dist], %[op]\n\t"                                                                              \
    "s_max_u32 %[reach], %[reach], %[t0]\n\t"                                                                          \
    "s_cmp_gt_u32 %[len], %[t0]\n\t"                                                                                   \
    "s_cbranch_scc1 L_exit2_%=\n\t"                                                                                    \
    "s_sub_u32 %[t1], 33024, %[t0]\n\t"                                                                                \
    "v_add_u32 %[vb], %[t1], %[lane]\n\t"                                                                              \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    "ds_write_b16 %[va], %[vb]\n\t"                                                                                    \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "s_add_u32 %[opb], %[opb], %[len]\n\t"                                                                             \
    "s_cmp_gt_u32 %[len], 64\n\t"                                                                                      \
    "s_cbranch_scc1 L_beforemore_%=\n\t"                                                                               \
    "s_branch L_top_%=\n\t"                                                                                            \
    "L_beforemore_%=:\n\t"                                                                                             \
    "s_mov_b32 %[t0], 64\n\t"                                                                                          \
    "L_beforeloop_%=:\n\t"                                                                                             \
    "s_sub_u32 %[e], %[len], %[t0]\n\t"                                                                                \
    "v_cmp_gt_u32 vcc, %[e], %[lane]\n\t"                                                                              \
    "s_add_u32 %[e], %[op], %[a0]\n\t"                                                                                 \
    "s_add_u32 %[e], %[e], %[t0]\n\t"                                                                                  \
    "v_add_u32 %[va], %[e], %[lane]\n\t"                                                                               \
    "s_add_u32 %[e], %[t1], %[t0]\n\t"                                                                                 \
    "v_and_b32 %[va], %[mask], %[va]\n\t"                                                                              \
    "v_add_u32 %[vb], %[e], %[lane]\n\t"                                                                               \
    "v_lshl_add_u32 %[va], %[va], %[sh], %[ringb]\n\t"                                                                 \
    "s_and_saveexec_b64 s[44:45], vcc\n\t"                                                                             \
    "ds_write_b16 %[va], %[vb]\n\t"                                                                                    \
    "s_mov_b64 exec, s[44:45]\n\t"                                                                                     \
    "s_add_u32 %[t0], %[t0], 64\n\t"                                                                                   \
    "s_cmp_lt_u32 %[t0], %[len]\n\t"                                                                                   \
    "s_cbranch_scc1 L_beforeloop_%=\n\t"                                                                               \
    "s_branch L_top_%=\n\t"

// PART = false: a job is a whole stream, the output is bytes (the many-stream entry points).
// PART = true (inflate_large.hip): a job is a PART of one large stream -- the decode starts at bit starts[job] of the
// stream, in the middle of it, and runs until a block ends exactly on a later entry of `starts` (or the stream ends).
// What lies in front of a part is not known while it is decoded, so the output is 16-bit SYMBOLS in the format of
// inflate_resolve.hip: a byte, or 256 + k = "byte k of the 32 KiB in front of this part"; copies move symbols, so
// unresolved references propagate by themselves, and the context chain of inflate_resolve.hip turns them into bytes.
// Results per part: 8 words {symbols produced, end bit (lo, hi), status, message, furthest reach in front of the part,
// index of the start it ended on, BFINAL seen}.  `marks` (parts only, may be null): 4 words per part, the state where its
// last block that ended inside the input ended {symbols produced, bit (lo, hi), furthest reach} -- what a part that ran
// out of input can still deliver (the streaming hook's blocks mode).
// SUB (parts only, zng_rocm_inflate_large_ex_dev with ZNG_ROCM_INFLATE_SUBBLOCK): a start may lie INSIDE a block.  keys[job]
// names the start: 0 a block start, 1 a symbol boundary inside a fixed-code block, H + 2 one inside the dynamic block whose
// header is at bit H.  A part hands off at such a sub-start -- stops there, `hit` = its index -- only when it decodes a
// block of the same identity (fixed; or the dynamic block whose header it read at H), stands at a symbol boundary and its
// bit position is exactly the start's: decoding on from there with the same tables is what the sub-part does.  A block end
// stops a part only on a block start (key 0).  The keys follow the njobs start bits in `starts`.  `marks` is then `side`: 8 words per part {symbols, bit (lo, hi), reach where its FIRST
// block ended (fixed-code sub-parts only: ~0 = not reached), handed off at a sub-start, BFINAL of the block it handed off
// in (2 = unknown: a fixed-code sub-part still in its first block), 0, 0}.
template <int RING, bool PART, bool COMPACT = false, bool SUB = false>
__global__ __launch_bounds__(64)
void inflate_streams_kernel(const InflateJobDev *__restrict__ jobs, uint32_t njobs, uint32_t *__restrict__ results,
                            const unsigned long long *__restrict__ starts, uint32_t *__restrict__ marks) {
    constexpr bool DICT = false, SPAN = false;
    const uint8_t *const hist_end = nullptr;
    const InflateSpanDev *const spans = nullptr;
#include "inflate_streams_body.h"
}

// The dictionary form (zng_rocm_uncompress_streams_dict_dev): the dict_len bytes of history of a job are the LAST dict_len
// bytes of one window shared by the whole launch, which ends at hist_end (a job decodes with all of it or, dict_len 0, none).
template <int RING>
__global__ __launch_bounds__(64)
void inflate_streams_dict_kernel(const InflateJobDev *__restrict__ jobs, uint32_t njobs, uint32_t *__restrict__ results,
                                 const uint8_t *__restrict__ hist_end) {
    constexpr bool PART = false, COMPACT = false, SUB = false, DICT = true, SPAN = false;
    const unsigned long long *const starts = nullptr;
    uint32_t *const marks = nullptr;
    const InflateSpanDev *const spans = nullptr;
#include "inflate_streams_body.h"
}

// The span form (zng_rocm_inflate_index_read_dev): a job is one span of an indexed stream.  It starts spans[job].start_bit
// bits into its first byte, its dict_len bytes of history are its OWN window, which ends at spans[job].hist_end (so the "too
// far back" test holds a damaged file inside that window), and it ends with status 1 where its output reaches out_cap -- at
// a block end or inside a block.
template <int RING>
__global__ __launch_bounds__(64)
void inflate_streams_span_kernel(const InflateJobDev *__restrict__ jobs, uint32_t njobs, uint32_t *__restrict__ results,
                                 const InflateSpanDev *__restrict__ spans) {
    constexpr bool PART = false, COMPACT = false, SUB = false, DICT = false, SPAN = true;
    const unsigned long long *const starts = nullptr;
    uint32_t *const marks = nullptr;
    const uint8_t *const hist_end = nullptr;
#include "inflate_streams_body.h"
}

int launch_inflate_streams_span_device(const InflateJobDev *d_jobs, size_t njobs, uint32_t *d_results, const InflateSpanDev *d_spans,
                                       hipStream_t st) {
    if (!njobs) return ZNG_ROCM_OK;
    ZR_LAUNCH_TRACED((inflate_streams_span_kernel<4096>), dim3((unsigned)njobs), dim3(64), st, d_jobs, (uint32_t)njobs, d_results,
                     d_spans);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

int launch_inflate_streams_dict_device(const InflateJobDev *d_jobs, size_t njobs, uint32_t *d_results, const uint8_t *d_hist_end,
                                       hipStream_t st) {
    if (!njobs) return ZNG_ROCM_OK;
    ZR_LAUNCH_TRACED((inflate_streams_dict_kernel<4096>), dim3((unsigned)njobs), dim3(64), st, d_jobs, (uint32_t)njobs, d_results,
                     d_hist_end);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

int launch_inflate_streams_device(const InflateJobDev *d_jobs, size_t njobs, uint32_t *d_results, hipStream_t st) {
    if (!njobs) return ZNG_ROCM_OK;
    // ring size: 4 KiB -> 16 streams per CU; 8 KiB (11 per CU) measured 25 % slower on both corpora.  The other
    // instantiations exist in measurement builds only (-DZR_MEASURE_FORMS, ZNG_ROCM_INFLATE_RING); the product reads no
    // environment variable.
#ifdef ZR_MEASURE_FORMS
    static const int ring = [] {
        const char *r = getenv("ZNG_ROCM_INFLATE_RING");
        return r ? atoi(r) : 4096;
    }();
    if (ring == 8192) ZR_LAUNCH_TRACED((inflate_streams_kernel<8192, false>), dim3((unsigned)njobs), dim3(64), st, d_jobs, (uint32_t)njobs, d_results, (const unsigned long long *)nullptr, (uint32_t *)nullptr);
    else if (ring == 16384) ZR_LAUNCH_TRACED((inflate_streams_kernel<16384, false>), dim3((unsigned)njobs), dim3(64), st, d_jobs, (uint32_t)njobs, d_results, (const unsigned long long *)nullptr, (uint32_t *)nullptr);
    else if (ring == 32768) ZR_LAUNCH_TRACED((inflate_streams_kernel<32768, false>), dim3((unsigned)njobs), dim3(64), st, d_jobs, (uint32_t)njobs, d_results, (const unsigned long long *)nullptr, (uint32_t *)nullptr);
    else
#endif
    ZR_LAUNCH_TRACED((inflate_streams_kernel<4096, false>), dim3((unsigned)njobs), dim3(64), st, d_jobs, (uint32_t)njobs, d_results, (const unsigned long long *)nullptr, (uint32_t *)nullptr);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

// the parts of ONE large stream (inflate_large.hip): d_starts = sorted start bits, one per job; results: 8 words per part
// `many`: more parts of real work than a chip holds at 12 per CU -- then the packed LDS layout (InflateLdsPart: 13 per CU)
// decodes more symbols per second (the cfg3 stream of this library's level-6 class: 8.2 -> 7.4 ms).  With fewer parts the
// call lasts as long as its longest part, and a part is faster in the plain layout among 12 (a CPython stream: 12.4
// against 13.2 ms): two instantiations, chosen per call.
int launch_inflate_parts_device(const InflateJobDev *d_jobs, size_t njobs, uint32_t *d_results, const unsigned long long *d_starts,
                                bool many, hipStream_t st, uint32_t *d_marks, uint32_t *d_side) {
    if (!njobs) return ZNG_ROCM_OK;
    if (d_side) {                                        // starts inside blocks (SUB): instantiations of their own
        if (many)
            ZR_LAUNCH_TRACED((inflate_streams_kernel<4096, true, true, true>), dim3((unsigned)njobs), dim3(64), st, d_jobs, (uint32_t)njobs, d_results, d_starts, d_side);
        else
            ZR_LAUNCH_TRACED((inflate_streams_kernel<4096, true, false, true>), dim3((unsigned)njobs), dim3(64), st, d_jobs, (uint32_t)njobs, d_results, d_starts, d_side);
        ZR_HIP(hipGetLastError());
        return ZNG_ROCM_OK;
    }
#ifdef ZR_MEASURE_FORMS
    static const int ring = [] {
        const char *r = getenv("ZNG_ROCM_PART_RING");
        return r ? atoi(r) : 4096;
    }();
    if (ring == 2048 && many) {
        ZR_LAUNCH_TRACED((inflate_streams_kernel<2048, true, true>), dim3((unsigned)njobs), dim3(64), st, d_jobs, (uint32_t)njobs, d_results, d_starts, d_marks);
        ZR_HIP(hipGetLastError());
        return ZNG_ROCM_OK;
    }
#endif
    if (many)
        ZR_LAUNCH_TRACED((inflate_streams_kernel<4096, true, true>), dim3((unsigned)njobs), dim3(64), st, d_jobs, (uint32_t)njobs, d_results, d_starts, d_marks);
    else
        ZR_LAUNCH_TRACED((inflate_streams_kernel<4096, true, false>), dim3((unsigned)njobs), dim3(64), st, d_jobs, (uint32_t)njobs, d_results, d_starts, d_marks);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}


// ---- sub-starts: the dry parse that turns a guessed bit into a symbol boundary (zng_rocm_inflate_large_ex_dev) ----------
// A region of the stream begins at a start the finder gave (inflate_large.hip); the block there (or, behind a stored block,
// the next one) is read once: fixed codes, or a dynamic header decoded and its tables built in LDS with the part kernel's
// builder.  Then each lane takes one guess G
// inside the region and parses kSyncSymbols symbols from it with those tables, writing nothing: a parse that starts
// off the symbol grid falls onto it within a few symbols (codes of a prefix code resynchronise), so the bit it ends on
// is, with high probability, a true symbol boundary B of the block -- and where it is not, nothing is lost: a part hands
// off only where a genuine decode stands exactly on B with the same tables (inflate_streams_kernel<..., SUB>).  A code the
// tables do not have (fixed: literal/length 286, 287, distance 30, 31; dynamic: the hole of an incomplete code), or an
// end-of-block code within the first kSyncSymbols / 2 symbols, means the parse is off the grid (or outside the block): it
// starts again one bit further on, up to kSyncRestarts times, and then reports no start.  An end-of-block code after that
// ends the parse on the boundary in front of it.  K = 128: on fixed-code data 99.9 % of guesses end on a true boundary,
// against 98.9 % with 64 (tests/test_subblock_sync_cpu.py walks a stream and checks).
constexpr int kSyncSymbols = 128, kSyncRestarts = 32;

__device__ __forceinline__ unsigned long long sync_bits_at(const uint8_t *src, unsigned long long src_len, unsigned long long bit) {
    const unsigned long long byte = bit >> 3;
    unsigned long long lo = 0, hi = 0;
    if (byte + 16 <= src_len) {
        const u32x4_unaligned v = load_u128(src + byte);
        lo = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
        hi = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
    } else {
        for (unsigned k = 0; k < 16 && byte + k < src_len; ++k) {
            const unsigned long long b = load_u8(src + byte + k);
            if (k < 8) lo |= b << (8 * k);
            else hi |= b << (8 * (k - 8));
        }
    }
    const unsigned s = (unsigned)(bit & 7ull);
    return s ? (lo >> s) | (hi << (64 - s)) : lo;
}

// a code longer than the root, per lane (long_code is the wave-uniform form)
template <typename LDS>
__device__ __forceinline__ uint32_t lane_long_code(LDS &L, int which, int root, const uint16_t *sorted, unsigned long long w) {
    const uint32_t rev15 = __builtin_bitreverse32((uint32_t)w & 0x7fffu) >> 17;
    const int max = (int)L.cnt(which)[0];
    for (int len = root + 1; len <= max; ++len) {
        const uint32_t d = (rev15 >> (15 - len)) - L.first(which)[len];
        if (d < L.cnt(which)[len]) return make_entry((uint32_t)len, sorted[ZR_IDX(L.offs(which)[len] + d, which == kCodeLit ? 288 : 32)]);
    }
    return kBadMark;
}

__global__ __launch_bounds__(64)
void subblock_sync_kernel(const uint8_t *__restrict__ src0, unsigned long long src_len0, const SubRegionDev *__restrict__ regions,
                          uint32_t nregions, unsigned long long *__restrict__ out_bit, unsigned long long *__restrict__ out_key) {
    constexpr int kLR = kLitRootStream, kDR = kDistRootStream;
    __shared__ InflateLdsStream<16, uint8_t, kDR, kLR> L;
    const int lane = threadIdx.x;
    const uint32_t r = blockIdx.x;
    if (r >= nregions) return;
    const SubRegionDev R = regions[r];
    // (a batch of streams: the region names its own; bit positions and keys are that stream's)
    const uint8_t *const src = R.src ? R.src : src0;
    const unsigned long long src_len = R.src ? R.src_len : src_len0;
    unsigned long long s0 = R.start;
    uint32_t type = (uint32_t)(sync_bits_at(src, src_len, s0) >> 1) & 3u;
    if (type == 0u) {
        // a stored block (the last of a chain the finder's byte pattern gave): the block behind it is the region's
        const unsigned long long q = (s0 + 3ull + 7ull) & ~7ull;
        s0 = q + 32ull + 8ull * ((uint32_t)sync_bits_at(src, src_len, q) & 0xffffu);
        type = (s0 >> 3) + 16 <= src_len ? (uint32_t)(sync_bits_at(src, src_len, s0) >> 1) & 3u : 3u;
    }
    bool ok = type == 1u || type == 2u;
    unsigned long long pos = s0 + 3;
    if (type == 2u) {
        // the dynamic header (inflate.c:814-917), wave-uniform, as the part kernel reads it
        unsigned long long w = sync_bits_at(src, src_len, pos);
        const uint32_t nlen = ((uint32_t)w & 31u) + 257u, ndist = ((uint32_t)(w >> 5) & 31u) + 1u, ncode = ((uint32_t)(w >> 10) & 15u) + 4u;
        pos += 14;
        if (nlen > 286 || ndist > 30) ok = false;
        if (lane < 19) L.cl_lens()[lane] = 0;
        wave_sync();
        w = sync_bits_at(src, src_len, pos);
        if (lane == 0)
            for (uint32_t i = 0; i < ncode; ++i) L.cl_lens()[kClOrder[i]] = (uint8_t)((w >> (3 * i)) & 7u);
        pos += 3ull * ncode;
        wave_sync();
        if (ok && uni((uint32_t)build_code(L, kCodeCl, L.cl_lens(), 19, kClRoot, L.cl(), L.sorted_cl(), lane))) ok = false;
        uint32_t have = 0;
        while (ok && have < nlen + ndist) {
            w = sync_bits_at(src, src_len, pos);
            const uint32_t e = uni(L.cl()[(uint32_t)w & ((1u << kClRoot) - 1u)]);
            const uint32_t nb = e & 15u, sym = e >> 4;
            pos += nb;
            w >>= nb;
            if (sym < 16) {
                if (lane == 0) L.lens[ZR_IDX(have, 320)] = (uint8_t)sym;
                ++have;
                continue;
            }
            uint32_t rep, val = 0;
            if (sym == 16) {
                rep = 3u + ((uint32_t)w & 3u);
                pos += 2;
                if (have == 0) { ok = false; break; }
                wave_sync();
                val = uni(L.lens[have - 1]);
            } else if (sym == 17) {
                rep = 3u + ((uint32_t)w & 7u);
                pos += 3;
            } else {
                rep = 11u + ((uint32_t)w & 127u);
                pos += 7;
            }
            if (have + rep > nlen + ndist) { ok = false; break; }
            for (uint32_t k = (uint32_t)lane; k < rep; k += 64) L.lens[ZR_IDX(have + k, 320)] = (uint8_t)val;
            have += rep;
        }
        wave_sync();
        if (ok && uni(L.lens[256]) == 0) ok = false;
        if (ok && uni((uint32_t)build_code(L, kCodeLit, L.lens, (int)nlen, kLR, L.lit, L.sorted_lit, lane))) ok = false;
        if (ok && uni((uint32_t)build_code(L, kCodeDist, L.lens + nlen, (int)ndist, kDR, reinterpret_cast<uint16_t *>(L.dist),
                                           L.sorted_dist, lane)))
            ok = false;
        if ((pos >> 3) > src_len) ok = false;
    }
    const uint16_t *dist16 = reinterpret_cast<const uint16_t *>(L.dist);
    // fixed codes in the odd slots when the region does not begin with them itself (a noise start inside fixed-code data
    // reads as a dynamic header, a stored block's pattern, or nothing valid at all)
    const bool fixed_too = type != 1u && R.fixed_too;
    if (type == 2u && !R.dynamic) ok = false;
    for (uint32_t t = (uint32_t)lane; t < 2u * R.n; t += 64) {
        const uint32_t g = t >> 1, ty = (t & 1u) ? 1u : type;       // odd slots: fixed codes in a dynamic region
        const unsigned long long key = ty == 1u ? 1ull : s0 + 2ull;
        unsigned long long g0 = R.start + (unsigned long long)(R.k0 + g + 1u) * R.spacing, B = ~0ull;
        const bool go = (t & 1u) ? fixed_too : ok;
        const unsigned long long lo = (t & 1u) ? R.start + 3ull : pos;
        for (int again = 0; go && g0 >= lo && B == ~0ull && again <= kSyncRestarts; ++again, ++g0) {
            unsigned long long p = g0;
            // 32 bytes per load, refilled when fewer than 48 bits (one symbol at most) are left: the parse is a chain of
            // dependent loads, and one per symbol made the kernel as long as its slowest lane's 128 load latencies
            unsigned long long q0 = 0, q1 = 0, q2 = 0, q3 = 0, wbase = 0;
            int k = 0;
            for (; k < kSyncSymbols; ++k) {
                if ((p >> 3) + 16 > src_len) break;
                if (k == 0 || p - wbase > 256 - 48 - 7) {
                    wbase = p & ~7ull;
                    const unsigned long long byte = p >> 3;
                    if (byte + 32 <= src_len) {
                        const u32x4_unaligned a = load_u128(src + byte), b = load_u128(src + byte + 16);
                        q0 = (unsigned long long)a.x | ((unsigned long long)a.y << 32);
                        q1 = (unsigned long long)a.z | ((unsigned long long)a.w << 32);
                        q2 = (unsigned long long)b.x | ((unsigned long long)b.y << 32);
                        q3 = (unsigned long long)b.z | ((unsigned long long)b.w << 32);
                    } else {
                        q0 = sync_bits_at(src, src_len, wbase);
                        q1 = sync_bits_at(src, src_len, wbase + 64);
                        q2 = q3 = 0;
                    }
                }
                const unsigned o = (unsigned)(p - wbase);              // < 256 - 48: the 64 bits at p lie in q0..q3
                const unsigned long long x0 = o < 64 ? q0 : o < 128 ? q1 : o < 192 ? q2 : q3;
                const unsigned long long x1 = o < 64 ? q1 : o < 128 ? q2 : q3;
                const unsigned sh = o & 63u;
                unsigned long long w = sh ? (x0 >> sh) | (x1 << (64 - sh)) : x0;
                uint32_t sym, nb;
                if (ty == 1u) {                            // fixed codes (RFC 1951 3.2.6) from the first 9 bits, MSB first
                    const uint32_t r9 = __builtin_bitreverse32((uint32_t)w & 0x1ffu) >> 23;
                    if ((r9 >> 2) < 24u) { sym = 256u + (r9 >> 2); nb = 7; }
                    else if ((r9 >> 1) < 0xc0u) { sym = (r9 >> 1) - 0x30u; nb = 8; }
                    else if ((r9 >> 1) < 0xc8u) { sym = 280u + (r9 >> 1) - 0xc0u; nb = 8; }
                    else { sym = 144u + r9 - 0x190u; nb = 9; }
                } else {
                    uint32_t e = L.lit[(uint32_t)w & ((1u << kLR) - 1u)];
                    if (e == kLongMark) e = lane_long_code(L, kCodeLit, kLR, L.sorted_lit, w);
                    sym = e >> 4;
                    nb = e & 15u;
                }
                if (sym == 256u) break;                    // end of block: the boundary in front of it, if enough came before
                if (sym > 285u) { k = -1; break; }         // (includes the builder's marks for "no code")
                p += nb;
                w >>= nb;
                if (sym < 256u) continue;
                const uint32_t lk = sym - 257u;
                const uint32_t lx = lk < 8u || lk == 28u ? 0u : (lk - 4u) >> 2;
                p += lx;
                w >>= lx;
                uint32_t dsym, dnb;
                if (ty == 1u) {
                    dsym = __builtin_bitreverse32((uint32_t)w & 31u) >> 27;
                    dnb = 5;
                } else {
                    uint32_t e = dist16[(uint32_t)w & ((1u << kDR) - 1u)];
                    if (e == kLongMark) e = lane_long_code(L, kCodeDist, kDR, L.sorted_dist, w);
                    dsym = e >> 4;
                    dnb = e & 15u;
                }
                if (dsym > 29u) { k = -1; break; }
                p += dnb + (dsym < 4u ? 0u : (dsym - 2u) >> 1);
            }
            if (k >= kSyncSymbols / 2) B = p;
            else if (k >= 0 && (p >> 3) + 16 > src_len) break;     // the input's end, not the grid: no start
        }
        out_bit[R.first + t] = B;
        out_key[R.first + t] = key;
    }
}

int launch_subblock_sync(const uint8_t *d_src, size_t src_len, const SubRegionDev *d_regions, size_t nregions,
                         unsigned long long *d_bit, unsigned long long *d_key, hipStream_t st) {
    if (!nregions) return ZNG_ROCM_OK;
    ZR_LAUNCH_TRACED(subblock_sync_kernel, dim3((unsigned)nregions), dim3(64), st, d_src, (unsigned long long)src_len, d_regions,
                     (uint32_t)nregions, d_bit, d_key);
    ZR_HIP(hipGetLastError());
    return ZNG_ROCM_OK;
}

}  // namespace zr

using namespace zr;

extern "C" {

#ifdef ZR_INFLATE_STATS
void zng_rocm_debug_inflate_spans(unsigned long long *out, unsigned n) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(zr::g_inflate_span), (size_t)(n < 16384u ? n : 16384u) * 16);
}
void zng_rocm_debug_inflate_stats(unsigned long long *out16, int reset) {
    (void)hipMemcpyFromSymbol(out16, HIP_SYMBOL(zr::g_inflate_stats), 16 * sizeof(unsigned long long));
    if (reset) {
        unsigned long long z[16] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(zr::g_inflate_stats), z, sizeof z);
    }
}
#endif
#ifdef ZR_INFLATE_BOUNDS
unsigned int zng_rocm_debug_inflate_bounds(void) {
    unsigned int v = 0;
    (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(zr::g_inflate_bounds_violations), sizeof v);
    return v;
}
#endif

const char *zng_rocm_inflate_message(uint32_t id) {
    static const char *const text[kMsgCount] = {
        "", "invalid block type", "invalid stored block lengths", "too many length or distance symbols",
        "invalid code lengths set", "invalid bit length repeat", "invalid code -- missing end-of-block",
        "invalid literal/lengths set", "invalid distances set", "invalid literal/length code", "invalid distance code",
        "invalid distance too far back", "input ended before the final block", "output buffer too small",
        "incorrect header check", "unknown compression method", "invalid window size", "header crc mismatch",
        "need dictionary", "incorrect data check", "incorrect length check"};
    return id < kMsgCount ? text[id] : "";
}

int zng_rocm_inflate_streams_dev(const zng_rocm_inflate_dev_job *jobs, size_t njobs, uint32_t *d_results, void *stream) {
    if (!ctx()) {
        set_error("zng_rocm_init() has not succeeded");
        return ZNG_ROCM_ENODEV;
    }
    if (!njobs) return ZNG_ROCM_OK;
    if (!jobs || !d_results || njobs > 0x7fffffffull) return ZNG_ROCM_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard dev;
    Workspace *ws = workspace_for(st);
    if (!ws) return ZNG_ROCM_ENOMEM;
    std::lock_guard<std::mutex> use(ws->mu);
    InflateJobDev *d_jobs = nullptr, *h_jobs = nullptr;
    if (int rc = scratch_reserve(ws, kScrInflateDevJobs, njobs * sizeof(InflateJobDev), false, (void **)&d_jobs)) return rc;
    if (int rc = host_tables_acquire(ws)) return rc;
    if (int rc = scratch_reserve(ws, kScrInflateDevJobsHost, njobs * sizeof(InflateJobDev), true, (void **)&h_jobs)) return rc;
    for (size_t i = 0; i < njobs; ++i) {
        const zng_rocm_inflate_dev_job &j = jobs[i];
        if ((j.in_len && !j.in) || (j.out_cap && !j.out) || j.in_len > 0x7fffffffull || j.out_cap > 0x7fffffffull ||
            j.dict_len > 32768u || (j.dict_len && !j.out) || j.flags) {
            set_error("job %zu: null buffer, a stream or output of 2 GiB and more, dict_len above 32768, or unknown flags", i);
            return ZNG_ROCM_EINVAL;
        }
        h_jobs[i] = InflateJobDev{(const uint8_t *)j.in, (uint8_t *)j.out, j.in_len, j.out_cap, j.dict_len, j.flags};
    }
    ZR_HIP(hipMemcpyAsync(d_jobs, h_jobs, njobs * sizeof(InflateJobDev), hipMemcpyHostToDevice, st));
    if (int rc = host_tables_release(ws, st)) return rc;
    if (int rc = launch_inflate_streams_device(d_jobs, njobs, d_results, st)) return rc;
    return ZNG_ROCM_OK;
}

}  // extern "C"
