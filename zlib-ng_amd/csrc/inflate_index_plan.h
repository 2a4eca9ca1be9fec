// inflate_index_plan.h -- the host steps of zng_rocm_inflate_index_build_dev, _read_dev, _export and _import_dev
// (inflate_index.hip): random access into ONE plain deflate, zlib or gzip stream that sits in device memory -- what zran.c
// and indexed_gzip do on a CPU.  Plain C++ over integers and tables, no HIP: which of the block starts a build met become
// access points, the plan that turns a batch of plaintext ranges into span jobs, slots, slices and rounds, what a range
// reports once the engine has spoken, and the check of a saved index.  tests/test_inflate_index_cpu.py drives them through
// tests/c/inflate_index_plan_driver.cpp without a GPU.
//
// An access point is {in_bit, out_off, window_len}: a deflate block begins at bit in_bit of the file, its first byte is byte
// out_off of the plaintext, and the window_len = min(32768, out_off) bytes in front of it are kept with the index.  The SPAN
// of point k is the plaintext [out_off_k, out_off_(k+1)), the last one ends at plain_len: one job of the one-wavefront engine
// in its span form (inflate_streams_span_kernel) decodes it, or a prefix of it, from the point alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

#include "../../include/zng_rocm.h"
#include "gf2.h"      // ZR_HD

namespace zr {

constexpr uint32_t kIndexWindow = 32768u;
constexpr uint64_t kIndexSpanDefault = 1ull << 20, kIndexSpanMin = 64ull << 10, kIndexSpanMax = 1ull << 30;
constexpr uint64_t kIndexScratchDefault = 256ull << 20, kIndexScratchMin = 1ull << 20, kIndexScratchMax = 4ull << 30;
constexpr uint64_t kIndexSpanEngineEnd = 1ull << 31;  // a span of this much output and more is not the one-wavefront engine's
constexpr uint32_t kIndexRoundJobs = 1u << 22;        // a round is closed behind the range that takes it past as many jobs
constexpr uint64_t kIndexDirect = ~0ull;              // IndexReadJob::slot of an interior span
constexpr uint32_t kIndexNoJob = 0xffffffffu;         // IndexReadPart::job of a part on a span the engine does not take

// span_bytes / scratch_bytes as the caller gives them -> the value used, or 0 for one the call refuses
inline uint64_t index_span_bytes(uint64_t span_bytes) {
    if (!span_bytes) return kIndexSpanDefault;
    return span_bytes < kIndexSpanMin || span_bytes > kIndexSpanMax ? 0u : span_bytes;
}
inline uint64_t index_scratch_bytes(uint64_t scratch_bytes) {
    if (!scratch_bytes) return kIndexScratchDefault;
    return scratch_bytes < kIndexScratchMin || scratch_bytes > kIndexScratchMax ? 0u : scratch_bytes;
}
inline uint32_t index_window_len(uint64_t out_off) { return out_off < kIndexWindow ? (uint32_t)out_off : kIndexWindow; }

// ---- the build: candidates -> points --------------------------------------------------------------------------------------
// A candidate is a block start the build's decode met on its way: bit of the FILE, offset in the plaintext.
struct IndexCand {
    uint64_t bit, out_off;
};

// Point 0 is {8 * header_len, 0, 0}.  The candidates are walked in the order they were met; one is taken when its out_off is
// at least `span` past the last point taken and in front of plain_len (a candidate AT plain_len -- the start of an empty
// final block -- has no byte to serve).  Candidates that repeat (a piece's last stop is the next piece's first part), that
// share an out_off (empty blocks) or that step back (a stretch decoded twice) fall to the same test.
inline void index_select(const IndexCand *cands, size_t n, uint64_t span, uint64_t plain_len, uint64_t header_len,
                         std::vector<zng_rocm_access_point> &pts) {
    pts.assign(1, zng_rocm_access_point{8 * header_len, 0u, 0u, 0u});
    for (size_t i = 0; i < n; ++i) {
        const IndexCand &c = cands[i];
        if (c.out_off < pts.back().out_off + span || c.out_off >= plain_len || c.bit <= pts.back().in_bit) continue;
        pts.push_back(zng_rocm_access_point{c.bit, c.out_off, index_window_len(c.out_off), 0u});
    }
}

// where point k's window begins in the windows stored one behind the other at their real lengths: woff[k], woff[n] = all
inline void index_window_offsets(const zng_rocm_access_point *pts, size_t n, std::vector<uint64_t> &woff) {
    woff.assign(n + 1, 0);
    for (size_t k = 0; k < n; ++k) woff[k + 1] = woff[k] + pts[k].window_len;
}

// ---- the saved form --------------------------------------------------------------------------------------------------------
// Little-endian, one behind the other:
//   0   u32 magic "ZRIX"      4  u32 version (1)     8  u32 format (0 raw, 1 zlib, 2 gzip)     12  u32 0
//   16  u64 header_len        24 u64 src_end (the indexed member's end in the file)          32  u64 plain_len
//   40  u64 span_bytes        48 u64 npoints
//   56  npoints rows of 24 bytes: u64 in_bit, u64 out_off, u32 window_len, u32 0
//   then the windows, point 0's first, each at its window_len
constexpr uint32_t kIndexMagic = 0x5849525au, kIndexVersion = 1u;
constexpr size_t kIndexBlobHead = 56, kIndexBlobRow = 24;

inline void put_le32(uint8_t *p, uint32_t v) { for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k)); }
inline void put_le64(uint8_t *p, uint64_t v) { for (int k = 0; k < 8; ++k) p[k] = (uint8_t)(v >> (8 * k)); }
inline uint32_t get_le32(const uint8_t *p) { uint32_t v = 0; for (int k = 0; k < 4; ++k) v |= (uint32_t)p[k] << (8 * k); return v; }
inline uint64_t get_le64(const uint8_t *p) { uint64_t v = 0; for (int k = 0; k < 8; ++k) v |= (uint64_t)p[k] << (8 * k); return v; }

struct IndexHead {
    uint32_t format;
    uint64_t header_len, src_end, plain_len, span_bytes;
};

inline uint64_t index_blob_bytes(const zng_rocm_access_point *pts, size_t n) {
    uint64_t w = 0;
    for (size_t k = 0; k < n; ++k) w += pts[k].window_len;
    return kIndexBlobHead + kIndexBlobRow * (uint64_t)n + w;
}
// header and rows (kIndexBlobHead + kIndexBlobRow * n bytes at buf); the windows follow them
inline void index_blob_write(const IndexHead &h, const zng_rocm_access_point *pts, size_t n, uint8_t *buf) {
    put_le32(buf, kIndexMagic);
    put_le32(buf + 4, kIndexVersion);
    put_le32(buf + 8, h.format);
    put_le32(buf + 12, 0u);
    put_le64(buf + 16, h.header_len);
    put_le64(buf + 24, h.src_end);
    put_le64(buf + 32, h.plain_len);
    put_le64(buf + 40, h.span_bytes);
    put_le64(buf + 48, n);
    for (size_t k = 0; k < n; ++k) {
        uint8_t *r = buf + kIndexBlobHead + kIndexBlobRow * k;
        put_le64(r, pts[k].in_bit);
        put_le64(r + 8, pts[k].out_off);
        put_le32(r + 16, pts[k].window_len);
        put_le32(r + 20, 0u);
    }
}

enum IndexBlobWhy : uint32_t {
    kBlobOk = 0, kBlobShort, kBlobMagic, kBlobVersion, kBlobFormat, kBlobSpan, kBlobCount, kBlobPoint0, kBlobInBit, kBlobOutOff,
    kBlobWindow, kBlobReserved, kBlobInside, kBlobSize
};
inline const char *index_blob_why(uint32_t why) {
    switch (why) {
    case kBlobShort: return "shorter than its header";
    case kBlobMagic: return "wrong magic";
    case kBlobVersion: return "unknown version";
    case kBlobFormat: return "format is none of 0, 1, 2";
    case kBlobSpan: return "span_bytes outside 64 KiB .. 1 GiB";
    case kBlobCount: return "no point, or more rows than the blob holds";
    case kBlobPoint0: return "point 0 is not {8 * header_len, 0, 0}";
    case kBlobInBit: return "in_bit is not ascending";
    case kBlobOutOff: return "out_off is not ascending, or not in front of plain_len";
    case kBlobWindow: return "window_len is not min(32768, out_off)";
    case kBlobReserved: return "a reserved word is not 0";
    case kBlobInside: return "a point begins behind src_end";
    case kBlobSize: return "the size does not match rows and windows";
    default: return "";
    }
}
// everything import checks, before any allocation; on kBlobOk `head` and `pts` are the blob's, the windows follow the rows
inline uint32_t index_blob_check(const uint8_t *buf, size_t len, IndexHead &head, std::vector<zng_rocm_access_point> &pts) {
    pts.clear();
    if (len < kIndexBlobHead) return kBlobShort;
    if (get_le32(buf) != kIndexMagic) return kBlobMagic;
    if (get_le32(buf + 4) != kIndexVersion) return kBlobVersion;
    head = IndexHead{get_le32(buf + 8), get_le64(buf + 16), get_le64(buf + 24), get_le64(buf + 32), get_le64(buf + 40)};
    if (head.format > 2u) return kBlobFormat;
    if (get_le32(buf + 12) != 0u) return kBlobReserved;
    if (head.span_bytes < kIndexSpanMin || head.span_bytes > kIndexSpanMax) return kBlobSpan;
    const uint64_t n = get_le64(buf + 48);
    if (!n || n > (len - kIndexBlobHead) / kIndexBlobRow) return kBlobCount;
    uint64_t windows = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const uint8_t *r = buf + kIndexBlobHead + kIndexBlobRow * k;
        const zng_rocm_access_point p = {get_le64(r), get_le64(r + 8), get_le32(r + 16), get_le32(r + 20)};
        if (p.reserved) return kBlobReserved;
        if (k == 0) {
            if (head.header_len > (~0ull >> 3) || p.in_bit != 8 * head.header_len || p.out_off || p.window_len) return kBlobPoint0;
        } else {
            if (p.in_bit <= get_le64(r - kIndexBlobRow)) return kBlobInBit;
            if (p.out_off <= get_le64(r - kIndexBlobRow + 8) || p.out_off >= head.plain_len) return kBlobOutOff;
        }
        if (p.window_len != index_window_len(p.out_off)) return kBlobWindow;
        if ((p.in_bit >> 3) > head.src_end) return kBlobInside;
        windows += p.window_len;
    }
    if (len - kIndexBlobHead - kIndexBlobRow * n != windows) return kBlobSize;
    pts.resize((size_t)n);
    for (uint64_t k = 0; k < n; ++k) {
        const uint8_t *r = buf + kIndexBlobHead + kIndexBlobRow * k;
        pts[(size_t)k] = zng_rocm_access_point{get_le64(r), get_le64(r + 8), get_le32(r + 16), 0u};
    }
    return kBlobOk;
}

// ---- the read: ranges -> jobs, slots, slices, rounds ----------------------------------------------------------------------
// the span that holds plaintext byte uoff: the last point with out_off <= uoff (out_off_0 = 0: there always is one)
inline size_t index_span_of(const zng_rocm_access_point *pts, size_t n, uint64_t uoff) {
    size_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (pts[mid].out_off <= uoff) lo = mid;
        else hi = mid;
    }
    return lo;
}
inline uint64_t index_span_end(const zng_rocm_access_point *pts, size_t n, size_t k, uint64_t plain_len) {
    return k + 1 < n ? pts[k + 1].out_off : plain_len;
}
inline uint64_t index_up16(uint64_t v) { return (v + 15) & ~15ull; }

struct IndexRangeIn {       // what the plan reads of a zng_rocm_inflate_range
    uint64_t uoff, len;
};
struct IndexReadJob {       // one span, or the front of one, through the engine
    uint64_t span;          // which point it starts from
    uint64_t slot;          // kIndexDirect: interior, decoded to the range's destination at `at`; else the byte offset of its
                            // slot in the round's scratch
    uint64_t out_cap;       // interior: the span's length; edge: the furthest byte any range of the round wants from it
    uint64_t at;            // interior: offset in that destination
    uint32_t range;         // interior: whose destination
};
struct IndexReadPart {      // the bytes one span contributes to one range, in range order
    uint32_t range;
    uint32_t job;           // index into IndexReadPlan::jobs, or kIndexNoJob (a span of 2 GiB and more)
    uint64_t at;            // offset in the range's destination
    uint64_t off, len;      // offset in the span's plaintext, bytes
    uint32_t slice;         // 1: copied from the job's slot by the slices kernel
};
struct IndexReadRound {
    size_t range_begin, range_end;
    size_t job_begin, job_end;
    size_t part_begin, part_end;
    uint64_t slot_bytes;    // the edge slots one behind the other, each at a multiple of 16
    uint32_t slices;
};
struct IndexReadPlan {
    std::vector<uint64_t> clipped;        // per range: the clipped length
    std::vector<IndexReadJob> jobs;
    std::vector<IndexReadPart> parts;
    std::vector<IndexReadRound> rounds;
    uint64_t decoded = 0, direct = 0;
};

// Ranges in order.  Per range the spans that hold its bytes: a span wholly inside the range is interior (one job of its own,
// straight into the destination, out_cap = its length), one the range only cuts is an edge (a range has at most two):
// decoded once per round into a slot, however many ranges of the round cut it, only as far as the furthest of them needs,
// and every such range gets a slice.  A round ends in front of the range with which its slots would pass `scratch` -- so only
// a round of ONE range, whose own edges are larger, is ever above it -- or behind the range that takes it past `round_jobs`
// jobs.  A span of kIndexSpanEngineEnd bytes and more gets no job: its parts carry kIndexNoJob.
inline void index_read_plan(const zng_rocm_access_point *pts, size_t n, uint64_t plain_len, const IndexRangeIn *ranges, size_t nranges,
                            uint64_t scratch, uint64_t round_jobs, IndexReadPlan &plan) {
    plan.clipped.assign(nranges, 0);
    plan.jobs.clear();
    plan.parts.clear();
    plan.rounds.clear();
    plan.decoded = plan.direct = 0;
    std::unordered_map<uint64_t, uint32_t> edge_job;      // span -> its job in the open round
    IndexReadRound cur = {0, 0, 0, 0, 0, 0, 0, 0};
    auto close = [&](size_t range_end) {
        cur.range_end = range_end;
        cur.job_end = plan.jobs.size();
        cur.part_end = plan.parts.size();
        uint64_t off = 0;                                 // the slots' places: known once the round's needs are
        for (size_t j = cur.job_begin; j < cur.job_end; ++j) {
            if (plan.jobs[j].slot == kIndexDirect) continue;
            plan.jobs[j].slot = off;
            off += index_up16(plan.jobs[j].out_cap);
        }
        cur.slot_bytes = off;
        if (cur.job_end > cur.job_begin) plan.rounds.push_back(cur);
        cur = IndexReadRound{range_end, range_end, plan.jobs.size(), plan.jobs.size(), plan.parts.size(), plan.parts.size(), 0, 0};
        edge_job.clear();
    };
    for (size_t r = 0; r < nranges; ++r) {
        const uint64_t uoff = ranges[r].uoff;
        const uint64_t len = uoff >= plain_len ? 0u : (ranges[r].len < plain_len - uoff ? ranges[r].len : plain_len - uoff);
        plan.clipped[r] = len;
        if (!len) continue;
        const uint64_t end = uoff + len;
        const size_t first = index_span_of(pts, n, uoff), last = index_span_of(pts, n, end - 1);
        // what this range would add to the open round's slots: its first and its last span, when they are cut
        auto growth = [&](size_t i) -> uint64_t {
            const uint64_t s = pts[i].out_off, e = index_span_end(pts, n, i, plain_len);
            if ((s >= uoff && e <= end) || e - s >= kIndexSpanEngineEnd) return 0u;
            const uint64_t need = (e < end ? e : end) - s;
            const auto hit = edge_job.find(i);
            if (hit == edge_job.end()) return index_up16(need);
            const uint64_t have = plan.jobs[hit->second].out_cap;
            return need > have ? index_up16(need) - index_up16(have) : 0u;
        };
        const uint64_t add = growth(first) + (last != first ? growth(last) : 0u);
        if (cur.slot_bytes + add > scratch && plan.jobs.size() > cur.job_begin) close(r);
        for (size_t i = first; i <= last; ++i) {
            const uint64_t s = pts[i].out_off, e = index_span_end(pts, n, i, plain_len);
            const uint64_t lo = s > uoff ? s : uoff, hi = e < end ? e : end;
            if (e - s >= kIndexSpanEngineEnd) {
                plan.parts.push_back(IndexReadPart{(uint32_t)r, kIndexNoJob, lo - uoff, lo - s, hi - lo, 0u});
                continue;
            }
            if (lo == s && hi == e) {
                plan.jobs.push_back(IndexReadJob{i, kIndexDirect, e - s, lo - uoff, (uint32_t)r});
                plan.parts.push_back(IndexReadPart{(uint32_t)r, (uint32_t)(plan.jobs.size() - 1), lo - uoff, 0u, e - s, 0u});
                ++plan.direct;
                ++plan.decoded;
                continue;
            }
            auto hit = edge_job.find(i);
            if (hit == edge_job.end()) {
                plan.jobs.push_back(IndexReadJob{i, 0u, hi - s, 0u, 0u});
                hit = edge_job.emplace(i, (uint32_t)(plan.jobs.size() - 1)).first;
                cur.slot_bytes += index_up16(hi - s);
                ++plan.decoded;
            } else if (hi - s > plan.jobs[hit->second].out_cap) {
                cur.slot_bytes += index_up16(hi - s) - index_up16(plan.jobs[hit->second].out_cap);
                plan.jobs[hit->second].out_cap = hi - s;
            }
            plan.parts.push_back(IndexReadPart{(uint32_t)r, hit->second, lo - uoff, lo - s, hi - lo, 1u});
            ++cur.slices;
        }
        if (plan.jobs.size() - cur.job_begin >= round_jobs) close(r + 1);
    }
    close(nranges);
}

// ---- what the engine said -> what a range reports -------------------------------------------------------------------------
struct IndexJobVerdict {    // of one job
    int32_t  status;        // 1 (the span decoded and gave exactly out_cap bytes), -3, -5
    uint32_t msg;           // -3: the engine's message id, or kIndexMsgMismatch; -5: 0, or kIndexMsgTooLong
};
constexpr uint32_t kIndexMsgMismatch = 0xffffffffu;    // "the stream ends in front of the span's end: the index is not this file's"
constexpr uint32_t kIndexMsgTooLong = 0xfffffffeu;     // "span too long for the one-wavefront engine"

// res: the engine's four words {produced, consumed, status, message id}.  The same rule decides in the slices kernel whether
// a slice is copied.
ZR_HD bool index_job_delivers(const uint32_t *res, uint32_t out_cap) { return (int32_t)res[2] == 1 && res[0] == out_cap; }
inline IndexJobVerdict index_job_verdict(const uint32_t *res, uint32_t out_cap) {
    if (index_job_delivers(res, out_cap)) return IndexJobVerdict{1, 0u};
    if ((int32_t)res[2] == 1) return IndexJobVerdict{-3, kIndexMsgMismatch};
    if ((int32_t)res[2] == -5) return IndexJobVerdict{-5, 0u};
    return IndexJobVerdict{-3, res[3]};
}

struct IndexRangeOut {
    int32_t  status;        // 1, -3, -5
    uint64_t out_len;
    uint32_t msg;           // of the first failing span
};
// parts[0, nparts): the parts of ONE range in order; verdicts indexed by IndexReadPart::job.  The FIRST failing span decides:
// its status, its message, and out_len = the bytes of the range in front of its part.
inline IndexRangeOut index_range_result(const IndexReadPart *parts, size_t nparts, const IndexJobVerdict *verdicts, uint64_t clipped) {
    for (size_t k = 0; k < nparts; ++k) {
        const IndexJobVerdict v = parts[k].job == kIndexNoJob ? IndexJobVerdict{-5, kIndexMsgTooLong} : verdicts[parts[k].job];
        if (v.status != 1) return IndexRangeOut{v.status, parts[k].at, v.msg};
    }
    return IndexRangeOut{1, clipped, 0u};
}

}  // namespace zr
