// inflate_large_plan.h -- the host steps between the kernel launches of inflate_large.hip (pass_run, and the finder in front
// of it).  Plain C++ over integers and the part tables, no HIP: every rule that decides what a valid result is -- how a
// finder pass is cut into work items, how many survivors it has room for and whose they are, which candidates become
// starts, where guesses go, how large a slot is, where the tables lie in scratch, which parts run again, which parts are
// genuine, how parts are grouped for the context chain and laid out in the symbol array, and how the pieces loop steps from
// one piece to the next (where a piece ends, where its pass's buffer begins, which bytes are its history, what the sequential
// decoder is given) -- lives here, and a CPU test (tests/test_large_plan_cpu.py) drives them with hand-written tables.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "inflate_dev_types.h"
#include "inflate_large_limits.h"

namespace zr {

constexpr uint32_t kSpacingBytes = 2u << 10;      // least compressed bytes between two starts -- applied only when there are
constexpr uint32_t kPartsUnthinned = 12288;       // more candidates than this.  (Thinning a short list loses real starts:
                                                  // about one random bit position in 10^6 passes F1 + F2, and a false start
                                                  // within the spacing in front of a real one would take its place; a false
                                                  // start that is kept costs one wasted part and nothing else.)
constexpr uint32_t kSegmentBytes = 40u << 10;     // parts are grouped into segments of at least this much OUTPUT for the
                                                  // context chain (which looks one segment back: >= 32 KiB each)
constexpr uint32_t kSlotRatio = 64;               // symbols of slot per compressed byte of the part ...
constexpr uint32_t kSlotSlack = 640u << 10;       // ... plus this (a 512 KiB run of one byte is ~600 bytes of deflate data)

struct PartCopy {
    const uint16_t *src;      // the part's slot
    uint64_t        dst;      // its first symbol's index in the stream's symbol array
    uint64_t        gstart;   // first symbol of the SEGMENT (group of consecutive parts) it belongs to
    uint32_t        n;
    uint32_t        first;    // chain index of the segment's first part
};

// One device pass of zng_rocm_inflate_large_pieces_dev over a piece of the stream.  The pass's buffer (d_src, src_len of
// inflate_large_try) begins at or in front of the piece -- at the header of the dynamic block a sub-start lies in, when it
// does -- and ends at the piece's end; the finder scans from `scan_lo` on.  Scratch is checked against caps that depend on
// the piece size alone (`q` = the largest piece, in compressed bytes); a pass that would need more asks to be run again
// with half the piece.
struct PiecePass {
    uint64_t scan_lo = 0;         // byte of the buffer where the piece (and the finder's scan) begins
    uint64_t key0 = 0;            // key of the first start: 0 a block start, 1 inside a fixed-code block, H + 2 (buffer bits)
    int      fin0 = -1;           // BFINAL of the fixed-code block a key-1 first start lies in (-1 unknown)
    bool     last = false;        // the piece reaches the end of the stream: stream mode (truncation, in_used, errors)
    uint64_t q = 0;
    // out
    bool     stopped = false;     // the chain stopped at a part that ran out of the piece: the next piece starts there
    uint64_t next_bit = 0, next_key = 0;
    int      next_fin = -1;
    bool     halve = false;       // the scratch caps were exceeded
};
// caps of one pass in bytes, q = piece bytes (the device scratch of a pieces call is their sum: DESIGN 3.10, zng_rocm.h)
constexpr uint32_t kPieceMaxParts = 65535;                      // also the compaction grid's y limit
inline uint64_t piece_cap_sub(uint64_t q) { return q / 8 + (1u << 20); }
inline uint64_t piece_cap_retry(uint64_t q) { return 32 * q; }
inline uint64_t piece_cap_sym(uint64_t q) { return 48 * q; }

// ---- scratch layouts ----------------------------------------------------------------------------------------------------
// tables one behind the other in one scratch buffer, each at a multiple of 256 bytes: add() gives the next table's offset
struct TableLayout {
    size_t bytes = 0;
    size_t add(size_t n) {
        const size_t at = bytes;
        bytes += (n + 255) & ~(size_t)255;
        return at;
    }
};

// The part tables of one launch over `np` parts: jobs | starts (| keys) | results (| marks, or | side words) | slots.  The
// keys (SUBBLOCK: 8 bytes per part) follow the starts, and the marks (blocks mode: 4 words per part) or side words (SUBBLOCK:
// 8 words per part) follow the 8 result words per part, so that jobs | starts | keys go up in one copy and results | marks
// or side words come down in one.  The pinned mirror has the same offsets without the slots.
struct PartTables {
    size_t jobs = 0, starts = 0, keys = 0, res = 0, extra = 0, slots = 0;      // byte offsets (keys / extra: where they would be)
    size_t up_bytes = 0;                                  // jobs | starts (| keys), from offset 0
    size_t res_words = 8;                                 // words per part that come down, from `res`
    size_t mirror_bytes = 0, device_bytes = 0;
};
inline PartTables part_tables(size_t np, bool sub, bool blocks, uint64_t slot_symbols) {
    PartTables t;
    TableLayout l;
    t.jobs = l.add(np * sizeof(InflateJobDev));
    t.starts = l.add(np * (sub ? 16 : 8));
    t.keys = t.starts + np * 8;
    t.up_bytes = t.starts + np * (sub ? 16 : 8);
    t.res_words = 8 + (blocks ? 4 : 0) + (sub ? 8 : 0);
    t.res = l.add(np * 4 * t.res_words);
    t.extra = t.res + np * 32;
    t.slots = t.mirror_bytes = l.bytes;
    t.device_bytes = t.mirror_bytes + (size_t)slot_symbols * 2;
    return t;
}

// what the device path takes: shorter streams are the sequential decoder's, and a bit position has to fit the tables' words
inline bool large_length_ok(uint64_t src_len) { return src_len >= (128u << 10) && src_len < (1ull << 31); }

// ---- candidates -> starts ---------------------------------------------------------------------------------------------
// a candidate is its bit position, bit 62 set for "a stored block" (light work)
inline bool by_bit(unsigned long long x, unsigned long long y) { return (x & ~(1ull << 62)) < (y & ~(1ull << 62)); }

// One finder pass over `ns` streams, stream k scanned over lens[k] bytes (one stream is a table of one).  The scan is cut
// into work items, one workgroup each, that tile each stream in order.  About 4096 of them, whatever the pass's bytes:
// that is 16 per CU and twice what the chip holds at once, so no CU is left with a share more (one 101 MB stream in 3529
// items of 28 KiB ran F1 4 % longer than in 4096 of 24 KiB).  `share` is a 4096th of the pass's bytes within 4 .. 64 KiB; a
// stream is cut into as few EQUAL items as stay within it; item_bytes, `share` in whole rounds of the pattern scan (4096
// bytes), is the bound no item passes.  cap1 / cap2: room for the survivors of F1 and of F2 (or of the pattern pass) of ALL
// the streams, a survivor per 64 and per 512 bytes and 4096 per stream -- starts are 2 KiB apart in the end; a pass with
// more is no deflate data.  `first`: as many survivors as come back with the counts.
struct FindPlan {
    uint64_t item_bytes = 0, share = 0;
    size_t   nitems = 0;
    uint32_t cap1 = 0, cap2 = 0, first = 0;
};
inline FindPlan find_plan(const uint64_t *lens, size_t ns) {
    FindPlan p;
    uint64_t total = 0;
    for (size_t k = 0; k < ns; ++k) total += lens[k];
    p.item_bytes = std::max<uint64_t>(4096, std::min<uint64_t>(65536, (total / 4096 + 4095) & ~4095ull));
    p.share = std::max<uint64_t>(4096, std::min<uint64_t>(p.item_bytes, (total + 4095) / 4096));
    for (size_t k = 0; k < ns; ++k) p.nitems += (size_t)((lens[k] + p.share - 1) / p.share);
    p.cap1 = (uint32_t)(total / 64 + 4096 * ns);
    p.cap2 = (uint32_t)(total / 512 + 4096 * ns);
    p.first = (uint32_t)std::min<size_t>(p.cap2, 16384 + 64 * ns);
    return p;
}
// the plan's nitems work items, written where they go up from (the host prepares a pass while the device waits for it)
inline void find_items(const uint64_t *lens, size_t ns, uint64_t share, FindItemDev *items) {
    for (size_t k = 0; k < ns; ++k) {
        const uint64_t n = (lens[k] + share - 1) / share, each = n ? (lens[k] + n - 1) / n : 0;
        for (uint64_t i = 0; i < n; ++i) *items++ = FindItemDev{std::min(i * each, lens[k]), std::min((i + 1) * each, lens[k]), (uint32_t)k, 0u};
    }
}
// The pass's survivors (two runs of the one list: what came back with the counts, and the rest) -> one list per stream,
// sorted: a survivor goes by its tag, which is taken off together with the "behind a marker" bit 63 (bit 62, "a stored
// block", stays); a tag that names no stream of the table is dropped.
inline std::vector<std::vector<unsigned long long>> find_demux(const unsigned long long *a, size_t na, const unsigned long long *b,
                                                               size_t nb, size_t ns) {
    std::vector<std::vector<unsigned long long>> per(ns);
    for (auto &list : per) list.reserve((na + nb) / ns + 1);                     // (one stream: the whole list, grown once)
    for (size_t i = 0; i < na + nb; ++i) {
        const unsigned long long c = i < na ? a[i] : b[i - na];
        const size_t k = (size_t)((c & kFindTagMask) >> kFindTagShift);
        if (k < ns) per[k].push_back(c & ~kFindTagMask & ~(1ull << 63));
    }
    for (auto &list : per) std::sort(list.begin(), list.end(), by_bit);
    return per;
}

// as many of the pattern pass's survivors as come back with its counts; a longer list is not one the patterns cut
inline uint32_t patterns_first(size_t scan_len) { return (uint32_t)std::min<size_t>(scan_len / 512 + 4096, 16384u); }

// Do the byte patterns alone (sync markers, byte-aligned stored blocks; `good` sorted by bit) cut the stream [start_bit,
// end_bit)?  "Enough" = no stretch of more than 128 KiB without one (a count would not do: the stored blocks of one
// incompressible region are thousands of starts and say nothing about the Huffman blocks elsewhere).
inline bool patterns_cut(const std::vector<unsigned long long> &good, unsigned long long start_bit, unsigned long long end_bit) {
    if (good.size() < 64u) return false;
    const unsigned long long gap = 8ull * (128u << 10);
    unsigned long long prev = start_bit;
    for (unsigned long long b62 : good) {
        const unsigned long long b = b62 & ~(1ull << 62);
        if (b - prev > gap) return false;
        prev = b;
    }
    return end_bit - prev <= gap;
}

// the sorted candidates thinned into starts; `heavy` counts the parts that are not a stored block: the ones that take time
inline void thin_starts(const std::vector<unsigned long long> &good, unsigned long long start_bit, uint64_t src_len,
                        std::vector<unsigned long long> &starts, size_t &heavy) {
    starts.assign(1, start_bit);                          // (candidates in front of it, or on it, fall to the spacing test)
    heavy = 1;
    const unsigned long long spacing = good.size() > kPartsUnthinned ? 8ull * kSpacingBytes : 1ull;
    for (unsigned long long b62 : good) {
        const unsigned long long b = b62 & ~(1ull << 62);
        if (b >= starts.back() + spacing && (b >> 3) + 16 < src_len) {
            starts.push_back(b);
            heavy += !(b62 >> 62);
        }
    }
}

// ---- SUBBLOCK: starts inside blocks -------------------------------------------------------------------------------------
// Guesses go into every gap between two starts found (and behind the last), one every `step` compressed bits.  The sync
// kernel reads the block at the gap's start (fixed codes, or a dynamic header and its tables) and turns each guess into a
// symbol boundary B with that identity.  `split_dynamic`: guesses with a dynamic block's tables; `fixed_first` (the stream's
// first block has fixed codes): every gap that does not begin with fixed codes gets fixed-code guesses as well -- about one
// bit position in 10^6 of fixed-code data passes F1 + F2 and one byte in 2^23 looks like a stored block's header, and the
// gap behind such a noise start would otherwise be one long part.
// `key0` (pieces) is the key of starts[0], which may lie inside a block itself: a key-1 one gets fixed-code guesses, a
// key-(H + 2) one the tables of the header at H, with the guesses placed behind it.
// `src` / `src_len`: the regions' own stream (a batch of streams in one launch), or null / 0 for the launch's.
// Appends to `regions`; `nguess` counts guess slots, two per guess.
inline void plan_sub_regions(const std::vector<unsigned long long> &starts, unsigned long long end_bit, unsigned long long step,
                             uint32_t split_dynamic, bool fixed_first, unsigned long long key0, const uint8_t *src,
                             unsigned long long src_len, std::vector<SubRegionDev> &regions, uint32_t &nguess) {
    for (size_t i = 0; i < starts.size() && (split_dynamic || fixed_first); ++i) {
        const unsigned long long s0 = starts[i], e0 = i + 1 < starts.size() ? starts[i + 1] : end_bit;
        const unsigned long long pieces = (e0 - s0 + step / 2) / step;
        if (pieces < 2) continue;
        unsigned long long rs = s0;
        const unsigned long long spacing = (e0 - s0) / pieces;
        uint32_t j0 = 0, dyn = split_dynamic, ft = fixed_first ? 1u : 0u;
        if (i == 0 && key0 == 1u) {                       // (what the sync kernel reads at s0 is no header: fixed guesses)
            dyn = 0u;
            ft = 1u;
        } else if (i == 0 && key0 >= 2u) {                // the region reads the header at H; its guesses begin behind s0
            rs = key0 - 2u;
            j0 = (uint32_t)((s0 - rs) / spacing);
        }
        // one work item (wavefront) per 64 guesses: a long gap is not one wavefront's serial work
        for (uint32_t k0 = 0; k0 < (uint32_t)(pieces - 1); k0 += 64u) {
            const uint32_t n = std::min<uint32_t>(64u, (uint32_t)(pieces - 1) - k0);
            regions.push_back(SubRegionDev{rs, spacing, nguess, n, dyn, ft, j0 + k0, 0u, src, src_len});
            nguess += 2u * n;
        }
    }
}

// The sync kernel's answers h_bit / h_key [first, last) (a boundary and its key, or ~0 = none) merged into the stream's
// starts and keys, sorted and deduplicated.  Returns the number of starts that now lie inside a block (key != 0); they are
// heavy parts.
inline size_t merge_sub_starts(std::vector<unsigned long long> &starts, std::vector<unsigned long long> &keys,
                               const unsigned long long *h_bit, const unsigned long long *h_key, uint32_t first, uint32_t last,
                               unsigned long long start_bit, uint64_t src_len, size_t &heavy) {
    std::vector<std::pair<unsigned long long, unsigned long long>> all;
    all.reserve(starts.size() + (last - first));
    for (size_t i = 0; i < starts.size(); ++i) all.emplace_back(starts[i], keys[i]);       // (keys[0]: a piece's key0)
    for (uint32_t g = first; g < last; ++g) {
        const unsigned long long b = h_bit[g];
        if (b != ~0ull && b > start_bit && (b >> 3) + 16 < src_len) all.emplace_back(b, h_key[g]);
    }
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    starts.clear();
    keys.clear();
    size_t inside = 0;
    for (const auto &a : all) {
        starts.push_back(a.first);
        keys.push_back(a.second);
        inside += a.second != 0;
    }
    heavy += inside;
    return inside;
}

// ---- slots --------------------------------------------------------------------------------------------------------------
// what every part's slot gets on top of kSlotRatio symbols per compressed byte, `np` parts in the launch (pieces: the parts'
// slack together stays within 8 symbols per compressed byte of the largest piece, 4 Ki at least)
inline uint64_t slot_slack(size_t np, const PiecePass *pp) {
    return pp ? std::max<uint64_t>(4u << 10, std::min<uint64_t>(kSlotSlack, 8 * pp->q / np))
              : std::max<uint64_t>(64u << 10, std::min<uint64_t>(kSlotSlack, (2ull << 30) / np));
}
// The `n` parts of one stream: part_bytes[i] = its compressed bytes (to the next start, the last one to end_bit),
// slot_off[i + 1] = slot_off[i] + its slot in symbols (slot_off[0] is the caller's: the stream's first slot).
inline void slot_caps(const unsigned long long *starts, size_t n, unsigned long long end_bit, uint64_t slack, uint64_t *slot_off,
                      uint64_t *part_bytes) {
    for (size_t i = 0; i < n; ++i) {
        part_bytes[i] = ((i + 1 < n ? starts[i + 1] : end_bit) - starts[i] + 7) >> 3;
        slot_off[i + 1] = slot_off[i] + ((part_bytes[i] * kSlotRatio + slack + 7) & ~7ull);
    }
}
// a part whose slot was too small (more than kSlotRatio : 1) is run once more with room for deflate's worst case, 1032 : 1
inline uint64_t retry_cap(uint64_t part_bytes) { return (part_bytes * 1032u + kSlotSlack + 7) & ~7ull; }

// Which parts run again after a launch (result words `res`, 8 per part; part_bytes per part), for streams whose parts are
// rows [first, first + n) of the tables (`spans`): every part that said kMsgOutFull, with retry_cap's room, one behind the
// other in ONE retry buffer.  A stream whose parts together want more than `limit_bytes` is reported in `over` and
// contributes nothing (it leaves the pass); the other streams' parts are still planned.
struct RetryPlan {
    std::vector<size_t> again;                            // rows of the tables
    std::vector<uint64_t> off, cap;                       // per entry of `again`: place and room in the retry buffer, in symbols
    uint64_t total = 0;                                   // symbols
    std::vector<size_t> over;                             // indices into `spans`
};
inline RetryPlan plan_retry(const uint32_t *res, const std::vector<std::pair<size_t, size_t>> &spans, const uint64_t *part_bytes,
                            uint64_t limit_bytes) {
    RetryPlan r;
    for (size_t k = 0; k < spans.size(); ++k) {
        const size_t i0 = spans[k].first, i1 = i0 + spans[k].second;
        uint64_t own = 0;
        for (size_t i = i0; i < i1; ++i)
            if (res[8 * i + 4] == kMsgOutFull) own += retry_cap(part_bytes[i]);
        if (own * 2 > limit_bytes) {
            r.over.push_back(k);
            continue;
        }
        for (size_t i = i0; i < i1; ++i) {
            if (res[8 * i + 4] != kMsgOutFull) continue;
            r.again.push_back(i);
            r.off.push_back(r.total);
            r.cap.push_back(retry_cap(part_bytes[i]));
            r.total += r.cap.back();
        }
    }
    return r;
}

// A stream that is over that limit need not leave: a candidate that was noise is never reached, and what is never reached
// needs no room (a stored block's payload may hold thousands of headers that promise 65535 bytes each, and every one of those
// parts says kMsgOutFull).  What the CHAIN needs is found by following the links from the stream's first part, rows
// [i0, i1) of the tables: the row of the first full part on it, i1 when the chain ends (BFINAL, or the input's end in a piece)
// without one, ~0 when it breaks (a message, a bad link).  pass_run runs that one part again and asks once more.
// This is a shorter statement of walk_chain, which stays the arbiter of what is delivered: it leaves out the FINAL fixed-code
// sub-part's early end, `past` and the piece's symbol cap, so it may follow the links FARTHER than walk_chain will.  That is
// safe: a full part found behind the place where walk_chain stops costs one rerun whose result nobody reads, never a wrong
// byte; a full part walk_chain reaches is always met here first, because up to there both follow the same links.
constexpr int kChainRetryTurns = 16;
inline size_t first_full_on_chain(const uint32_t *res, size_t i0, size_t i1) {
    for (size_t cur = i0;;) {
        const uint32_t *r = &res[8 * cur];
        if (r[4] == kMsgOutFull) return cur;
        if (r[4] == kMsgStarved) return i1;
        if (r[4] != kMsgNone) return ~(size_t)0;
        if (r[3] == 1u) return i1;
        if (r[6] <= cur || r[6] >= i1) return ~(size_t)0;
        cur = r[6];
    }
}

// ---- the chain from the stream's first part ---------------------------------------------------------------------------
// Part 0 is genuine, the part that starts where it ended is therefore genuine too, ...; a candidate that was noise is never
// reached.  Result words of a part (inflate_streams_kernel<PART>): r[0] symbols, r[1..2] the bit it ended on, r[3] = 1 when
// that was the end of the BFINAL block, r[4] message, r[5] the farthest a distance reached in front of the part, r[6] the
// part (index in the launch's tables) that starts where it ended, or ~0.  SUBBLOCK side words: s[0] symbols of the part's
// first block (~0: it did not end inside the input), s[1..2] the bit that block ended on, s[3] the reach within it, s[4]
// != 0 when the part handed off inside a block, whose BFINAL is s[5] (2: unknown).  Blocks mode marks: m[0] symbols of the
// part's complete blocks, m[1..2] where they end, m[3] the reach within them.
struct Chain {
    std::vector<PartCopy> copies;                         // the genuine parts in order; gstart / first: symbol_tables
    uint64_t produced = 0;
    unsigned long long end_bit = 0;
    bool final = false;                                   // the BFINAL block is among what was delivered
    size_t subparts = 0;                                  // of the parts, those that began inside a block
    // `record` (an index is being built: inflate_index_plan.h): every genuine part that begins at a block start, as {its bit,
    // the symbols produced in front of it} -- positions in the pass's own buffer and output
    bool record = false;
    std::vector<std::pair<unsigned long long, uint64_t>> cands;
    // a failed walk: why, and when it was a part's own result (message, no end), which part of the stream
    const char *reason = nullptr;
    size_t bad_part = ~(size_t)0;
};

// One stream's walk.  res / side / marks / slot_ptr are the launch's tables, the stream's parts are [pbase, pbase + np)
// of them; starts / keys (SUBBLOCK) are the stream's own.  Modes: `sub` (side words, keys), `blocks` (the input may end
// inside a block: the chain stops at the first part that ran out of it and keeps that part's complete blocks), `pp` (a
// piece: see PiecePass; its out fields are set here).  false = irregular (c.reason): the caller decides what that means.
inline bool walk_chain(const uint32_t *res, const uint32_t *side, const uint32_t *marks, uint16_t *const *slot_ptr, size_t pbase,
                       size_t np, const unsigned long long *starts, const unsigned long long *keys, uint32_t window_len,
                       uint64_t src_len, bool sub, bool blocks, PiecePass *pp, Chain &c) {
    const bool piece = pp && !pp->last;                   // the input ends at the piece's end, not the stream's
    auto fail = [&](const char *reason) {
        c.reason = reason;
        return false;
    };
    c.end_bit = starts[0];
    int fin = pp ? pp->fin0 : -1;                         // SUBBLOCK: BFINAL of the block the current part began inside
    for (size_t cur = 0;;) {
        const size_t g = pbase + cur;
        const uint32_t *r = &res[8 * g], *s = sub ? &side[8 * g] : nullptr;
        const bool ended = r[3] == 1u;
        // (pieces: an end behind the piece's input is no end yet -- the next piece decodes that part again)
        const bool past = piece && sub && s[0] != 0xffffffffu && ((unsigned long long)s[1] | ((unsigned long long)s[2] << 32)) > 8ull * src_len;
        if (sub && keys[cur] == 1u && fin == 1 && s[0] != 0xffffffffu && !past) {
            // a fixed-code sub-part inside the FINAL block (its header, read by a part in front, said so): the stream ends
            // where its first block ended, whatever it decoded behind that
            c.end_bit = (unsigned long long)s[1] | ((unsigned long long)s[2] << 32);
            if (c.end_bit > 8ull * src_len) return fail("the final block runs past the input");
            if ((uint64_t)s[3] > c.produced + window_len) return fail("a distance reaches in front of the stream");
            if (s[0]) c.copies.push_back(PartCopy{slot_ptr[g], c.produced, 0, s[0], 0u});
            c.produced += s[0];
            ++c.subparts;
            c.final = true;
            return true;
        }
        if (pp) {
            // pieces: the first part on the chain that ran out of the piece's input is where the next piece begins; so is a
            // part whose symbols would take the symbol array past its cap (in the last piece too; in front of the array lie
            // the pass's tables: 32 bytes per copy, at most 40 per segment, the closing triple, the window entry and padding)
            const bool full = r[4] == kMsgNone && ((c.produced + r[0] + 32768 + 64) * 2 + 72 * (c.copies.size() + 1) + 1536 >
                                                   piece_cap_sym(pp->q));
            if ((piece && r[4] == kMsgStarved) || full || (past && keys[cur] == 1u && fin == 1)) {
                if (cur == 0) {
                    pp->halve = full;
                    return fail(full ? "the piece's first part needs more scratch than its cap"
                                     : "no start behind the piece's first is landed on");
                }
                pp->stopped = true;
                pp->next_bit = starts[cur];
                pp->next_key = sub ? keys[cur] : 0ull;
                pp->next_fin = fin;
                c.end_bit = starts[cur];
                return true;
            }
        }
        if (blocks && r[4] == kMsgStarved) {              // the input ends in this part: its complete blocks, and no more
            const uint32_t *m = &marks[4 * g];
            if ((uint64_t)m[3] > c.produced + window_len) return fail("a distance reaches in front of the stream");
            if (m[0]) c.copies.push_back(PartCopy{slot_ptr[g], c.produced, 0, m[0], 0u});
            c.produced += m[0];
            c.end_bit = (unsigned long long)m[1] | ((unsigned long long)m[2] << 32);
            return true;
        }
        if (r[4] != kMsgNone || !(ended || r[6] != 0xffffffffu)) {                // error / truncation on the chain
            c.bad_part = cur;
            return fail("a part's message, or no end");
        }
        if ((uint64_t)r[5] > c.produced + window_len) return fail("a distance reaches in front of the stream");
        if (c.record && (!sub || keys[cur] == 0)) c.cands.emplace_back(starts[cur], c.produced);
        c.copies.push_back(PartCopy{slot_ptr[g], c.produced, 0, r[0], 0u});
        c.produced += r[0];
        c.end_bit = (unsigned long long)r[1] | ((unsigned long long)r[2] << 32);
        if (ended) {
            c.final = true;
            return true;
        }
        if (sub) {
            c.subparts += keys[cur] != 0;
            // handed off inside a block: the next part starts there and learns that block's BFINAL from here (2: this part
            // did not know it either -- a fixed-code sub-part still in its first block -- so it stays what it was)
            if (s[4]) fin = s[5] == 2u ? fin : (int)s[5];
            else fin = -1;
        }
        // a part ends on a LATER start of its own stream (so a bad word cannot send the walk round in a circle)
        if (r[6] <= g || r[6] >= pbase + np) return fail("bad chain link");
        cur = r[6] - pbase;
    }
}

// Segments for the context chain: consecutive parts until kSegmentBytes of output are together; what is left at the end
// joins the last segment unless it is a segment's worth (32 KiB) itself (only the stream's LAST segment may be short).
// Returns the index in `copies` of every segment's first part, and copies.size() behind them.
inline std::vector<size_t> group_segments(const std::vector<PartCopy> &copies, uint64_t produced) {
    std::vector<size_t> seg_first;
    size_t first = 0;
    for (size_t c = 0; c < copies.size(); ++c) {
        if (copies[c].dst + copies[c].n - copies[first].dst >= kSegmentBytes || c + 1 == copies.size()) {
            seg_first.push_back(first);
            first = c + 1;
        }
    }
    if (seg_first.size() > 1 && produced - copies[seg_first.back()].dst < 32768u) seg_first.pop_back();
    seg_first.push_back(copies.size());
    return seg_first;
}

// ---- the symbol array ---------------------------------------------------------------------------------------------------
// The streams of a pass one behind the other in ONE symbol array, each behind its own gap of 32768 symbols (its window: the
// layout of inflate_resolve_batch), stream k at v_k = v_(k-1) + produced_(k-1) + 32768, the first at 32768.  A stream that
// produced nothing has no place (v = 0).  Per stream in: the copies of its chain (dst counted from the stream's first
// symbol), what it produced, and the address of its destination.  Out, for the compaction and the resolve:
//   copies   all streams' copies, dst re-based to the array, gstart = the first symbol of the copy's segment and first = the
//            index in `copies` of that segment's first copy (group_segments decides the segments)
//   segs     a triple per segment as inflate_resolve.hip wants them -- only [3 s + 1], the segment's first symbol, is used --
//            and the closing triple with v_end, the end of the last stream
//   seg_dst  the address the segment's first byte goes to; seg_end: where its bytes end in the array (a stream's last segment
//            runs on through the gap behind it for the context chain, its bytes do not)
struct SymStream {
    const std::vector<PartCopy> *copies;
    uint64_t produced, dst;
    uint64_t v = 0;                                       // out
};
struct SymTables {
    std::vector<PartCopy> copies;
    std::vector<uint64_t> segs, seg_dst, seg_end;
    uint64_t v_end = 0;
};
inline SymTables symbol_tables(std::vector<SymStream> &streams) {
    SymTables t;
    uint64_t v = 32768;
    for (SymStream &s : streams) {
        if (!s.produced) continue;
        s.v = v;
        const std::vector<PartCopy> &sc = *s.copies;
        const std::vector<size_t> seg_first = group_segments(sc, s.produced);
        const uint32_t c0 = (uint32_t)t.copies.size();
        for (size_t g = 0; g + 1 < seg_first.size(); ++g) {
            const uint64_t o0 = sc[seg_first[g]].dst;
            const uint64_t o1 = g + 2 < seg_first.size() ? sc[seg_first[g + 1]].dst : s.produced;
            for (size_t c = seg_first[g]; c < seg_first[g + 1]; ++c) {
                PartCopy p = sc[c];
                p.dst += v;
                p.gstart = v + o0;
                p.first = c0 + (uint32_t)seg_first[g];
                t.copies.push_back(p);
            }
            t.segs.insert(t.segs.end(), {0, v + o0, 0});
            t.seg_dst.push_back(s.dst + o0);
            t.seg_end.push_back(v + o1);
        }
        t.v_end = v + s.produced;
        v = t.v_end + 32768;
    }
    if (!t.copies.empty()) t.segs.insert(t.segs.end(), {0, t.v_end, 0});
    return t;
}

// ---- pieces: the loop of zng_rocm_inflate_large_pieces_dev --------------------------------------------------------------
// What the loop carries from one turn to the next.  A turn is a device pass over the next piece (piece_next, then
// piece_after_pass or piece_halve), or the sequential decoder from the anchor (seq_input .. piece_after_blocks).
struct PiecesState {
    uint64_t bit = 0, key = 0;        // where the next piece begins (a bit of the stream) and that start's key (0 a block start, 1
                                      // inside a fixed-code block, H + 2 inside the dynamic block whose header is at stream bit H)
    int      fin = -1;                // PiecePass::fin0 of the next pass
    uint64_t produced = 0;            // bytes delivered
    uint64_t abit = 0, aout = 0;      // the anchor: the last BLOCK start delivered up to, and the output in front of it
    uint64_t p = 0;                   // the piece size of the next pass: piece_bytes, halved while passes ask for it
};
inline PiecesState pieces_begin(uint64_t piece_bytes) {
    PiecesState s;
    s.p = piece_bytes;
    return s;
}

// The next piece: [bit >> 3, end) of the stream; one that would leave less than a quarter piece behind it ends a quarter
// piece early (so the last piece is never a sliver).  The pass's buffer [base, end) begins at the piece, or at the header of
// the dynamic block its first start lies in when that is in front of it, rounded down to 256 bytes; bit positions of the
// pass -- the first start, a key of 2 and more -- count from the buffer's first byte (keys 0 and 1 are no positions).
struct NextPiece {
    bool      any = false;            // input is left at the state's bit (else the sequential decoder says how the stream ends)
    uint64_t  end = 0, base = 0;
    uint64_t  start_bit = 0;          // the state's bit as a bit of the buffer: start_bit >> 3 == pp.scan_lo
    PiecePass pp;                     // in fields set
    uint64_t len() const { return end - base; }
    uint64_t stream_byte(uint64_t used) const { return base + used; }      // a byte count of the buffer, as one of the stream
};
inline NextPiece piece_next(const PiecesState &s, uint64_t src_len, uint64_t piece_bytes) {
    NextPiece n;
    const uint64_t sbyte = s.bit >> 3;
    n.any = sbyte < src_len;
    if (!n.any) return n;
    n.end = sbyte + s.p;
    if (n.end >= src_len) n.end = src_len;
    else if (src_len - n.end < s.p / 4) n.end = src_len - s.p / 4;
    n.base = (s.key >= 2 ? std::min<uint64_t>(sbyte, (s.key - 2) >> 3) : sbyte) & ~(uint64_t)255;
    n.start_bit = s.bit - 8 * n.base;
    n.pp.scan_lo = sbyte - n.base;
    n.pp.key0 = s.key >= 2 ? s.key - 8 * n.base : s.key;
    n.pp.fin0 = s.fin;
    n.pp.last = n.end == src_len;
    n.pp.q = piece_bytes;
    return n;
}

// After a pass that returned 1 with `out` bytes and `used` bytes of its buffer: the stream ended in the piece (done, with the
// call's in_used), or the next piece begins where the chain stopped -- that start and its key back in stream positions, the
// BFINAL the chain carried to it, the full piece size again; a stop at a block start moves the anchor there.
struct PieceStep {
    bool     done = false;
    uint64_t in_used = 0;
    bool     anchored = false;        // the anchor moved (to the state's bit and produced)
};
inline PieceStep piece_after_pass(PiecesState &s, const NextPiece &n, uint64_t out, uint64_t used, uint64_t piece_bytes) {
    PieceStep r;
    s.produced += out;
    if (!n.pp.stopped) {
        r.done = true;
        r.in_used = n.stream_byte(used);
        return r;
    }
    s.bit = n.pp.next_bit + 8 * n.base;
    s.key = n.pp.next_key >= 2 ? n.pp.next_key + 8 * n.base : n.pp.next_key;
    s.fin = n.pp.next_fin;
    s.p = piece_bytes;
    r.anchored = s.key == 0;
    if (r.anchored) {
        s.abit = s.bit;
        s.aout = s.produced;
    }
    return r;
}
// the block starts a pass recorded (Chain::cands: the pass's own positions) as positions of the stream and the call's output
inline void piece_cands(const std::vector<std::pair<unsigned long long, uint64_t>> &pass, const NextPiece &n, const PiecesState &s,
                        std::vector<std::pair<uint64_t, uint64_t>> &out) {
    for (const auto &c : pass) out.emplace_back(c.first + 8 * n.base, s.produced + c.second);
}
// A pass over its scratch caps (PiecePass::halve): the same start with half the piece, while that is a piece the call takes
inline bool piece_halve(PiecesState &s) {
    if (s.p / 2 < kPieceMin) return false;
    s.p /= 2;
    return true;
}

// The history of a pass (or of the sequential decoder's tokens) at output position `pos`: the last min(32768, pos +
// window_len) bytes in front of it.  They lie in the call's output, or -- nothing delivered yet -- are the caller's window as
// it stands, or are spliced: the window's last `from_window` bytes, then the `from_dst` bytes delivered.
struct PieceHistory {
    enum Where { kInDst, kWindow, kSpliced };
    uint32_t len = 0;
    Where    where = kInDst;
    uint64_t dst_off = 0;             // kInDst: where it begins in the output
    uint64_t window_off = 0, from_window = 0, from_dst = 0;       // kSpliced
};
inline PieceHistory piece_history(uint64_t pos, uint32_t window_len) {
    PieceHistory h;
    const uint64_t n = std::min<uint64_t>(32768u, pos + window_len);
    h.len = (uint32_t)n;
    if (pos >= n) {
        h.dst_off = pos - n;
    } else if (pos == 0) {
        h.where = PieceHistory::kWindow;
    } else {
        h.where = PieceHistory::kSpliced;
        h.from_window = n - pos;
        h.window_off = window_len - h.from_window;
        h.from_dst = pos;
    }
    return h;
}

// The sequential decoder takes the stream from the anchor: byte a0, bit sb of it.  It is given complete blocks' worth of input:
// at least two pieces, and the piece the device could not do whole; twice as much while no block completes (status 0, the
// end bit still sb) and more input exists.
struct SeqInput {
    uint64_t a0 = 0, sb = 0, span = 0;
    uint64_t len(uint64_t src_len) const { return std::min<uint64_t>(src_len - a0, span); }
    uint64_t stream_byte(uint64_t used) const { return a0 + used; }
};
inline SeqInput seq_input(const PiecesState &s) {
    SeqInput in;
    in.a0 = s.abit >> 3;
    in.sb = s.abit & 7u;
    in.span = std::max<uint64_t>(2 * s.p, (s.bit >> 3) - in.a0 + s.p);
    return in;
}
inline bool seq_wants_more(SeqInput &in, uint64_t src_len, int status, uint64_t eb) {
    if (!(status == 0 && eb == in.sb && in.len(src_len) < src_len - in.a0)) return false;
    in.span *= 2;
    return true;
}
// The blocks form's answer stands when it ended the stream (1), completed a block (0, the end bit moved) or ran out of memory
// (-4); a data error, or the end of the input inside the first block, is decoded once more in the stream form, whose status,
// message and counts are the reference's.
inline bool seq_stream_form(int status, uint64_t eb, uint64_t sb) {
    return status != 1 && !(status == 0 && eb != sb) && status != -4;
}
inline uint64_t seq_blocks_bytes(uint64_t eb) { return (eb + 7) >> 3; }          // input bytes the complete blocks took, from a0
// After the sequential decoder's complete blocks, which end at bit `eb` (counted from byte a0) with `produced` bytes delivered
// in all (the anchor's and theirs): the next piece begins there, at a block start, which is the new anchor.
inline void piece_after_blocks(PiecesState &s, const SeqInput &in, uint64_t eb, uint64_t produced, uint64_t piece_bytes) {
    s.produced = produced;
    s.bit = 8 * in.a0 + eb;
    s.key = 0;
    s.fin = -1;
    s.abit = s.bit;
    s.aout = s.produced;
    s.p = piece_bytes;
}

}  // namespace zr
