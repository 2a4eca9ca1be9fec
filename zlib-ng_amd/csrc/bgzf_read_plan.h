// bgzf_read_plan.h -- the host steps of zng_rocm_bgzf_index_dev, zng_rocm_bgzf_read_dev and the virtual offsets
// (bgzf_read.hip): random access into a BGZF file (SAM specification 4.1; htslib bgzf.c) that sits in device memory.  Plain
// C++ over integers and tables, no HIP: the chain walk that turns the candidate table into the members table (what follows a
// member is judged as gz_look judges it, gzread.c.in:81-154), the check of a members table a caller hands in, the plan that
// turns a batch of plaintext ranges into decode jobs, slices and rounds, what a range's result is once the engine has spoken,
// and htslib's virtual offsets.  tests/test_bgzf_read_cpu.py drives them through tests/c/bgzf_read_plan_driver.cpp without a
// GPU.
//
// What is believed and what is not.  The index is what the file CLAIMS: BSIZE from the 'BC' subfield, CRC-32 and ISIZE from
// the eight bytes in front of the claimed end; nothing is decoded to make it.  A read believes no row: every member a range
// touches goes through the one-wavefront engine as a gzip member (header, payload, CRC-32 and ISIZE verified on the device),
// and a member delivers bytes only when it decoded with status 1, consumed exactly the row's src_len and produced exactly
// the row's out_len.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

#include "../../include/zng_rocm.h"
#include "gf2.h"      // ZR_HD

namespace zr {

constexpr uint32_t kBgzfReadMaxMember = 65536u;       // BSIZE + 1 at its largest; also the most plaintext a member may claim
constexpr uint32_t kBgzfReadMinMember = 28u;          // 18 bytes of header, 2 of deflate, 8 of trailer: the end-of-file block
constexpr uint64_t kBgzfReadSlot = 65536u;            // an edge member's plaintext in scratch
constexpr uint64_t kBgzfReadScratchDefault = 256ull << 20, kBgzfReadScratchMin = 128ull << 10, kBgzfReadScratchMax = 4ull << 30;
constexpr uint32_t kBgzfReadRoundJobs = 1u << 22;     // a round is closed behind the range that takes it past as many members:
                                                      // its job and result tables stay bounded (64 MiB of result rows) like its slots
constexpr uint32_t kBgzfReadDirect = 0xffffffffu;     // BgzfReadJob::slot of an interior member

// ---- the index: candidate rows -> members ---------------------------------------------------------------------------------
// One row per candidate, as bgzf_index_link_kernel writes it and the host reads it back.
constexpr uint32_t kIdxBgzf = 1u;         // the header was accepted (wrapper_parse_rules) and carries 'BC': `end` is pos + BSIZE + 1
constexpr uint32_t kIdxCut = 2u;          // the header kernel ran out of bytes inside the header
constexpr uint32_t kIdxInside = 4u;       // end <= src_len
constexpr uint32_t kIdxRoom = 8u;         // end - pos >= header_len + 2 + 8
constexpr uint32_t kIdxTrailer = 16u;     // crc / isize were read (kIdxInside and kIdxRoom)
constexpr uint32_t kIdxNextMagic = 32u;   // two bytes exist at `end` and are 1f 8b
struct BgzfIndexRow {
    uint64_t pos;
    uint64_t end;           // kIdxBgzf: pos + BSIZE + 1, else pos
    uint32_t header_len;    // kIdxBgzf: bytes in front of the deflate data
    uint32_t crc, isize;    // kIdxTrailer: the eight bytes at end - 8, least significant byte first
    uint32_t flags;
};

// the flags of a row, written once for the kernel and for the CPU test's tables
ZR_HD uint32_t bgzf_index_flags(bool bgzf, bool cut, uint64_t pos, uint64_t end, uint64_t header_len, uint64_t src_len) {
    uint32_t f = cut ? kIdxCut : 0u;
    if (!bgzf) return f;
    f |= kIdxBgzf;
    if (end <= src_len) f |= kIdxInside;
    if (end - pos >= header_len + 2u + 8u) f |= kIdxRoom;
    if ((f & kIdxInside) && (f & kIdxRoom)) f |= kIdxTrailer;
    return f;
}

enum BgzfIndexWhy : uint32_t {
    kIdxOk = 0,
    kIdxWhyNoHeader,        // -3: 1f 8b (or the file's first byte) where no accepted BGZF header begins
    kIdxWhyNoRoom,          // -3: BSIZE leaves no room for header, deflate data and trailer
    kIdxWhyIsize,           // -3: ISIZE above 65536
    kIdxWhyCutHeader,       // -5: the file ends inside the header
    kIdxWhyCutMember,       // -5: the BSIZE end lies behind the file's end
};
struct BgzfIndexWalk {
    int      status;        // 0, -3, -5
    uint32_t why;
    uint64_t at;            // where the walk stopped: the end of the last member
    uint64_t plain_len;
    size_t   nmembers;      // the true count; rows beyond members_cap are counted and not written
};

// index of the row at `at`, or n
inline uint32_t bgzf_index_at(const BgzfIndexRow *rows, uint32_t n, uint64_t at) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rows[mid].pos < at) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && rows[lo].pos == at ? lo : n;
}

// The chain from offset 0: a member begins at the file's first byte or where the member in front ends (its BSIZE says so),
// and candidates inside a member's bytes are never looked at.  Behind a complete member: fewer than two bytes, or two bytes
// other than 1f 8b, are trailing garbage (gz_look asks avail_in > 1, gzread.c.in:127) and end the walk with 0; 1f 8b has to
// be a BGZF member.  `look`: the bytes of a candidate the header kernel is shown at most (a header that is cut although that
// many bytes exist is one this call refuses, -3, not one the file's end cuts; 1f 8b with fewer than two bytes behind it is a
// header the file's end cuts).  At offset 0 nothing is in front to excuse anything: a file shorter than a BGZF header is cut
// (-5), any other beginning that is no member is refused (-3).
inline BgzfIndexWalk bgzf_index_walk(const BgzfIndexRow *rows, uint32_t n, uint64_t src_len, uint64_t look, zng_rocm_gzip_member *members,
                                     size_t members_cap) {
    BgzfIndexWalk w = {0, kIdxOk, 0, 0, 0};
    if (!src_len) return w;
    bool magic = true;                                   // are the two bytes at w.at 1f 8b?  (offset 0: judged by the row there)
    for (;;) {
        if (w.at >= src_len || !magic) return w;
        const uint32_t i = bgzf_index_at(rows, n, w.at);
        auto stop = [&](int status, uint32_t why) {
            w.status = status;
            w.why = why;
            return w;
        };
        if (i == n)                                      // (fewer than four bytes cannot be a candidate: 1f 8b and the file's end)
            return src_len - w.at < 4u || (w.at == 0 && src_len < 18u) ? stop(-5, kIdxWhyCutHeader) : stop(-3, kIdxWhyNoHeader);
        const BgzfIndexRow &r = rows[i];
        if ((r.flags & kIdxCut) && src_len - r.pos <= look) return stop(-5, kIdxWhyCutHeader);
        if (!(r.flags & kIdxBgzf)) return stop(-3, kIdxWhyNoHeader);
        if (!(r.flags & kIdxInside)) return stop(-5, kIdxWhyCutMember);
        if (!(r.flags & kIdxRoom)) return stop(-3, kIdxWhyNoRoom);
        if (r.isize > kBgzfReadMaxMember) return stop(-3, kIdxWhyIsize);
        if (w.nmembers < members_cap) members[w.nmembers] = zng_rocm_gzip_member{r.pos, r.end - r.pos, w.plain_len, r.isize, r.crc, 1u};
        ++w.nmembers;
        w.plain_len += r.isize;
        w.at = r.end;
        magic = (r.flags & kIdxNextMagic) != 0;
    }
}

// ---- a members table the caller hands in ----------------------------------------------------------------------------------
enum BgzfRowsWhy : uint32_t { kRowsOk = 0, kRowsOrder, kRowsOutside, kRowsDstOff, kRowsNotBgzf, kRowsSrcLen, kRowsOutLen };
// the first row zng_rocm_bgzf_read_dev refuses (*bad) and why, or kRowsOk
inline uint32_t bgzf_read_rows_check(const zng_rocm_gzip_member *m, size_t n, uint64_t src_len, size_t *bad) {
    uint64_t src_end = 0, dst_end = 0;
    for (size_t i = 0; i < n; ++i) {
        *bad = i;
        if (m[i].src_len < kBgzfReadMinMember || m[i].src_len > kBgzfReadMaxMember) return kRowsSrcLen;
        if (m[i].out_len > kBgzfReadMaxMember) return kRowsOutLen;
        if (m[i].bgzf != 1u) return kRowsNotBgzf;
        if (m[i].src_off < src_end) return kRowsOrder;
        if (m[i].src_off > src_len || m[i].src_len > src_len - m[i].src_off) return kRowsOutside;
        if (m[i].dst_off != dst_end) return kRowsDstOff;
        src_end = m[i].src_off + m[i].src_len;
        dst_end += m[i].out_len;
    }
    *bad = n;
    return kRowsOk;
}
inline uint64_t bgzf_plain_len(const zng_rocm_gzip_member *m, size_t n) { return n ? m[n - 1].dst_off + m[n - 1].out_len : 0u; }

// scratch_bytes as the caller gives it -> edge slots per round, or 0 for a value the call refuses
inline uint64_t bgzf_read_slots(uint64_t scratch_bytes) {
    if (!scratch_bytes) scratch_bytes = kBgzfReadScratchDefault;
    if (scratch_bytes < kBgzfReadScratchMin || scratch_bytes > kBgzfReadScratchMax) return 0;
    return scratch_bytes / kBgzfReadSlot;
}

// index of the first member whose plaintext ends behind uoff (the member that holds byte uoff), or n
inline size_t bgzf_member_of(const zng_rocm_gzip_member *m, size_t n, uint64_t uoff) {
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (m[mid].dst_off + m[mid].out_len <= uoff) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- the plan -------------------------------------------------------------------------------------------------------------
struct BgzfRangeIn {        // what the plan reads of a zng_rocm_bgzf_range
    uint64_t uoff, len;
};
struct BgzfReadJob {        // one member through the engine
    uint64_t member;
    uint32_t slot;          // kBgzfReadDirect: interior, decoded to the range's destination at `at`; else the round's edge slot
    uint32_t range;         // interior: whose destination
    uint64_t at;            // interior: offset in that destination
};
struct BgzfReadPart {       // the bytes one member contributes to one range, in range order
    uint32_t range;
    uint32_t job;           // index into BgzfReadPlan::jobs
    uint64_t at;            // offset in the range's destination
    uint32_t off, len;      // offset in the member's plaintext, bytes; direct parts: off 0, len = out_len
    uint32_t slice;         // 1: copied from the job's slot by bgzf_slices_kernel
};
struct BgzfReadRound {
    size_t range_begin, range_end;
    size_t job_begin, job_end;
    size_t part_begin, part_end;
    uint32_t slots, slices;
};
struct BgzfReadPlan {
    std::vector<uint64_t> clipped;        // per range: the clipped length
    std::vector<BgzfReadJob> jobs;
    std::vector<BgzfReadPart> parts;
    std::vector<BgzfReadRound> rounds;
    uint64_t decoded = 0, direct = 0;
};

// Ranges in order.  Per range the members that hold its bytes, empty ones skipped: a member wholly inside the range is
// interior (one job of its own, straight into the destination), one the range only cuts is an edge: decoded once per round
// into a slot, however many ranges of the round cut it, and every such range gets a slice.  A round ends in front of the
// range whose new edges would not find a slot (a range has at most two, and `slots` is at least two), or behind the range
// that takes it past `round_jobs` jobs.
inline void bgzf_read_plan(const zng_rocm_gzip_member *m, size_t n, const BgzfRangeIn *ranges, size_t nranges, uint64_t slots,
                           uint64_t round_jobs, BgzfReadPlan &plan) {
    plan.clipped.assign(nranges, 0);
    plan.jobs.clear();
    plan.parts.clear();
    plan.rounds.clear();
    plan.decoded = plan.direct = 0;
    const uint64_t plain_len = bgzf_plain_len(m, n);
    std::unordered_map<uint64_t, uint32_t> edge_job;      // member -> its job in the open round
    BgzfReadRound cur = {0, 0, 0, 0, 0, 0, 0, 0};
    auto close = [&](size_t range_end) {
        cur.range_end = range_end;
        cur.job_end = plan.jobs.size();
        cur.part_end = plan.parts.size();
        if (cur.job_end > cur.job_begin) plan.rounds.push_back(cur);
        cur = BgzfReadRound{range_end, range_end, plan.jobs.size(), plan.jobs.size(), plan.parts.size(), plan.parts.size(), 0, 0};
        edge_job.clear();
    };
    for (size_t r = 0; r < nranges; ++r) {
        const uint64_t uoff = ranges[r].uoff;
        const uint64_t len = uoff >= plain_len ? 0u : (ranges[r].len < plain_len - uoff ? ranges[r].len : plain_len - uoff);
        plan.clipped[r] = len;
        if (!len) continue;
        const uint64_t end = uoff + len;
        const size_t first = bgzf_member_of(m, n, uoff);
        // the edges this range would add to the open round: its first and its last member, when they are cut
        size_t last = first;
        for (size_t i = first; i < n && m[i].dst_off < end; ++i)
            if (m[i].out_len) last = i;
        auto fresh_edge = [&](size_t i) {
            const bool whole = m[i].dst_off >= uoff && m[i].dst_off + m[i].out_len <= end;
            return !whole && !edge_job.count(i) ? 1u : 0u;
        };
        const uint32_t fresh = fresh_edge(first) + (last != first ? fresh_edge(last) : 0u);
        if (cur.slots + fresh > slots && plan.jobs.size() > cur.job_begin) close(r);
        for (size_t i = first; i <= last; ++i) {
            if (!m[i].out_len) continue;
            const uint64_t lo = m[i].dst_off > uoff ? m[i].dst_off : uoff;
            const uint64_t hi = m[i].dst_off + m[i].out_len < end ? m[i].dst_off + m[i].out_len : end;
            if (lo == m[i].dst_off && hi == m[i].dst_off + m[i].out_len) {
                plan.jobs.push_back(BgzfReadJob{i, kBgzfReadDirect, (uint32_t)r, lo - uoff});
                plan.parts.push_back(BgzfReadPart{(uint32_t)r, (uint32_t)(plan.jobs.size() - 1), lo - uoff, 0u, (uint32_t)m[i].out_len, 0u});
                ++plan.direct;
                ++plan.decoded;
                continue;
            }
            auto hit = edge_job.find(i);
            if (hit == edge_job.end()) {
                plan.jobs.push_back(BgzfReadJob{i, cur.slots++, 0u, 0u});
                hit = edge_job.emplace(i, (uint32_t)(plan.jobs.size() - 1)).first;
                ++plan.decoded;
            }
            plan.parts.push_back(BgzfReadPart{(uint32_t)r, hit->second, lo - uoff, (uint32_t)(lo - m[i].dst_off), (uint32_t)(hi - lo), 1u});
            ++cur.slices;
        }
        if (plan.jobs.size() - cur.job_begin >= round_jobs) close(r + 1);
    }
    close(nranges);
}

// ---- what the engine said -> what a range reports -----------------------------------------------------------------------
struct BgzfJobVerdict {     // of one job
    int32_t  status;        // 1 (the member verified and is what the row says), -3, -5
    uint32_t msg;           // -3: the engine's message id, or kBgzfMsgRow
};
constexpr uint32_t kBgzfMsgRow = 0xffffffffu;          // "index row does not match the file"

// res: the engine's four words {produced, consumed, status, message id}.  The same rule decides in bgzf_slices_kernel
// whether a slice is copied.
ZR_HD bool bgzf_member_delivers(const uint32_t *res, uint32_t want_used, uint32_t want_out) {
    return (int32_t)res[2] == 1 && res[1] == want_used && res[0] == want_out;
}
inline BgzfJobVerdict bgzf_job_verdict(const uint32_t *res, const zng_rocm_gzip_member &row) {
    if (bgzf_member_delivers(res, (uint32_t)row.src_len, (uint32_t)row.out_len)) return BgzfJobVerdict{1, 0u};
    if ((int32_t)res[2] == 1) return BgzfJobVerdict{-3, kBgzfMsgRow};
    if ((int32_t)res[2] == -5) return BgzfJobVerdict{-5, 0u};
    return BgzfJobVerdict{-3, res[3]};
}

struct BgzfRangeOut {
    int32_t  status;        // 1, -3, -5
    uint64_t out_len;
    uint32_t msg;           // -3: message id of the first member that failed with -3
    bool     has_msg;
};
// parts[0, nparts): the parts of ONE range in order; verdicts indexed by BgzfReadPart::job.  A data or check failure (-3)
// anywhere in the range outweighs a truncated member (-5); out_len counts the bytes in front of the first part that failed.
inline BgzfRangeOut bgzf_range_result(const BgzfReadPart *parts, size_t nparts, const BgzfJobVerdict *verdicts, uint64_t clipped) {
    BgzfRangeOut o = {1, clipped, 0u, false};
    bool failed = false;
    for (size_t k = 0; k < nparts; ++k) {
        const BgzfJobVerdict &v = verdicts[parts[k].job];
        if (v.status == 1) continue;
        if (!failed) o.out_len = parts[k].at;
        failed = true;
        if (v.status == -3 && !o.has_msg) {
            o.status = -3;
            o.msg = v.msg;
            o.has_msg = true;
        } else if (o.status == 1) {
            o.status = -5;
        }
    }
    return o;
}

// ---- virtual offsets (htslib: coffset << 16 | uoffset) ------------------------------------------------------------------
// voff = src_off << 16 | (uoff - dst_off) of the member that holds uoff.  An offset at a member's end is offset 0 of the
// next non-empty member; plain_len, which no member holds, maps to the start of the last row (the end-of-file block of a
// complete file), as bgzf_tell says it behind the last byte.
inline bool bgzf_voffset(const zng_rocm_gzip_member *m, size_t n, uint64_t uoff, uint64_t *voff) {
    if (!n || uoff > bgzf_plain_len(m, n)) return false;
    size_t i = bgzf_member_of(m, n, uoff);
    if (i == n) i = n - 1;
    if (m[i].src_off >= (1ull << 48)) return false;
    const uint64_t in = uoff - m[i].dst_off;
    if (in > 0xffffu) return false;                      // (plain_len behind a last row of 65536 bytes: sixteen bits cannot say it)
    *voff = (m[i].src_off << 16) | in;
    return true;
}
inline bool bgzf_uoffset(const zng_rocm_gzip_member *m, size_t n, uint64_t voff, uint64_t *uoff) {
    const uint64_t coff = voff >> 16, in = voff & 0xffffu;
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (m[mid].src_off < coff) lo = mid + 1;
        else hi = mid;
    }
    if (lo == n || m[lo].src_off != coff || in > m[lo].out_len) return false;
    *uoff = m[lo].dst_off + in;
    return true;
}

}  // namespace zr
