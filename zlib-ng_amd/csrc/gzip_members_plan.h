// gzip_members_plan.h -- the host steps of zng_rocm_gunzip_members_dev (gzip_members.hip): every member of a gzip file that
// sits in device memory, as gz_look / gz_decomp read it (gzread.c.in:81-154, :161-207).  Plain C++ over integers and the
// candidate table, no HIP: the rules that decide what a member is live here -- which positions are candidates, where a
// candidate's member is guessed to end, which members are decoded together and where their plaintext goes, what makes a
// decoded member genuine, and what the bytes behind the last member mean -- and a CPU test (tests/test_gzip_members_cpu.py)
// drives them with hand-written tables.  The two rules the kernels apply as well (member_candidate, member_next) are
// written once for host and device.
//
// Nothing found on the device is believed before it is decoded: a candidate is a place where a member MAY begin (the four
// bytes are just as likely inside a stored block or a file name), its end is a guess (BSIZE, or the next candidate), its
// plaintext length is a guess (the four bytes in front of the guessed end).  A member counts when it was decoded from a
// position that is the file's first byte or the end of a member that counts, with status 1 (so check value and ISIZE
// agree), exactly the guessed bytes consumed and exactly the guessed bytes produced; it writes only inside the guessed
// output, so a wrong guess cannot touch a neighbour that counts.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "framing_parse.h"
#include "gf2.h"

namespace zr {

constexpr uint64_t kMembersSmallBelow = 128u << 10;   // spans below this go to the one-wavefront engine: the large engine's
                                                      // own floor (large_length_ok), under which it decodes on the host
constexpr uint64_t kMembersLargeEnd = 1ull << 31;     // spans from here on are decoded alone (the pieces engine)
constexpr int kMembersMaxReplans = 8;                 // wrong guesses answered with a new plan; behind them the plain loop
constexpr uint32_t kCandBgzf = 1u, kCandTrailer = 2u; // CandRow::flags
// What discovery may cost on a file made to hurt.  A candidate is four bytes anyone can write, one per four bytes of a stored
// block at the worst, and a header with FNAME / FCOMMENT reads up to the first zero byte -- the end of the file, if the file
// has none -- with an FHCRC pass over as much behind it.  gzread and the caller's loop parse only real headers.  So the header
// kernel is shown at most kMembersHeaderLook bytes of a candidate (every header a common writer makes is a few dozen bytes; a
// legal one can pass 64 KiB of FEXTRA): a header that does not end inside them comes back "cut" (-5) like one the file's end
// cuts, and the plan decodes such a candidate alone, at full length, if the chain really reaches it -- results do not change.
// And a file with more than kMembersMaxCandidates candidates (a BGZF file of 1 TiB has as many members) gets no table at all:
// it goes through the plain loop of single calls.  Discovery therefore examines at most src_len (the scan) +
// min(src_len / 4, kMembersMaxCandidates) * 2 * kMembersHeaderLook bytes (header and FHCRC pass), and its tables are bounded.
constexpr uint64_t kMembersHeaderLook = 4096;
constexpr uint32_t kMembersMaxCandidates = 1u << 24;
constexpr uint32_t kMembersTooMany = 0xffffffffu;     // the candidate count the device reports beyond kMembersMaxCandidates

// position p is a candidate iff src[p .. p + 3] is 1f 8b 08 F with F & 0xe0 == 0: the bytes every header that
// wrapper_parse_rules accepts begins with (inflate.c:556-567).  `w` = the four bytes, least significant first.
ZR_HD bool member_candidate(uint32_t w) { return (w & 0xe0ffffffu) == 0x00088b1fu; }

// the bytes of the candidate at p that the header kernel is shown
ZR_HD uint64_t member_header_look(uint64_t src_len, uint64_t p) {
    return src_len - p < kMembersHeaderLook ? src_len - p : kMembersHeaderLook;
}

// host restatement of the scan kernel: every candidate of src[0, n) in order
inline void scan_candidates(const uint8_t *src, uint64_t n, std::vector<uint64_t> &pos) {
    pos.clear();
    for (uint64_t p = 0; p + 4 <= n; ++p)
        if (member_candidate(wrapper_le32(src + p))) pos.push_back(p);
}

// One row per candidate, as the link kernel writes it and the host reads it back.
struct CandRow {
    uint64_t pos;           // where in the file
    uint64_t header_len;    // status 0: bytes in front of the deflate data
    uint32_t next;          // the candidate the member is guessed to end on; n (the candidates' number) = the end of the file
    int32_t  status;        // the header's verdict (WrapperHead): 0 accepted, -3 refused (msg), -5 the file ends inside it
    uint32_t msg;
    uint32_t flags;         // kCandBgzf: a 'BC' subfield gave BSIZE; kCandTrailer: crc / isize were read
    uint32_t crc, isize;    // the eight bytes in front of the guessed end
};

// index of the candidate at `at`, or n
ZR_HD uint32_t member_at(const uint64_t *pos, uint32_t n, uint64_t at) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pos[mid] < at) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && pos[lo] == at ? lo : n;
}

// Where candidate i's member is guessed to end: a BGZF member says so itself (BSIZE + 1 bytes) and is believed when
// another candidate, or the end of the file, is there -- candidates inside it are hopped over; any other member is guessed
// to reach the next candidate.
ZR_HD uint32_t member_next(const uint64_t *pos, uint32_t n, uint32_t i, bool has_bsize, uint32_t bsize, uint64_t src_len) {
    if (has_bsize) {
        const uint64_t end = pos[i] + bsize + 1u;
        if (end == src_len) return n;
        const uint32_t j = member_at(pos, n, end);
        if (j < n && j > i) return j;
    }
    return i + 1;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------
enum MemberEngine : uint32_t { kEngineSmall = 0, kEngineLarge = 1 };

struct PlannedMember {
    uint32_t cand;
    uint32_t engine;
    uint64_t src_off, span;       // the guessed member
    uint64_t dst_off, out_guess;  // its plaintext: out_guess is also its output capacity, to the byte
    uint32_t crc, bgzf;
    bool     to_end;              // the span reaches the end of the file: bytes may be left behind the member
};

struct MembersPlan {
    std::vector<PlannedMember> items;
    uint32_t solo = 0;            // alone: the candidate the chain reached that is not decoded on a guess
    bool     alone = false;
    bool     bad_guess = false;   // alone because the guess about it cannot be right (a wrong guess like one the engines refute:
                                  // a re-plan), not because of what it is (header not accepted, dst_cap, a span of 2 GiB)
    uint64_t dst_end = 0;         // where the plaintext of the last planned member is guessed to end
};

// The chain from candidate `start` (whose position is the file's first byte or a member's end) along `next`, the ISIZE
// guesses summed into dst_off from `dst_off` on.  The chain stops in front of a candidate that cannot be decoded on a guess,
// which is then decoded alone (MembersPlan::alone) with the capacity that is really left:
//   its header was not accepted (its trouble is the call's, told by the single call), its guess passes dst_cap, or its span
//   is one for the pieces engine;
//   or the guess cannot be right (bad_guess) -- the guessed end leaves no room for header and trailer, so it is a candidate
//   inside the member; or the guessed length is more than 1032 times the span, deflate's best.
inline void plan_members(const CandRow *rows, uint32_t n, uint64_t src_len, uint32_t start, uint64_t dst_off, uint64_t dst_cap,
                         MembersPlan &plan) {
    plan.items.clear();
    plan.alone = plan.bad_guess = false;
    plan.solo = 0;
    for (uint32_t i = start; i < n;) {
        const CandRow &r = rows[i];
        const bool to_end = r.next >= n;
        const uint64_t end = to_end ? src_len : rows[r.next].pos;
        const uint64_t span = end - r.pos;
        const bool bad_guess = r.status == 0 && (!(r.flags & kCandTrailer) || (uint64_t)r.isize > span * 1032u);
        if (r.status != 0 || bad_guess || r.next <= i || span >= kMembersLargeEnd || (uint64_t)r.isize > dst_cap - dst_off) {
            plan.alone = true;
            plan.bad_guess = bad_guess;
            plan.solo = i;
            break;
        }
        plan.items.push_back(PlannedMember{i, span < kMembersSmallBelow ? kEngineSmall : kEngineLarge, r.pos, span, dst_off, r.isize, r.crc,
                                           (r.flags & kCandBgzf) ? 1u : 0u, to_end});
        dst_off += r.isize;
        i = r.next;
    }
    plan.dst_end = dst_off;
}

struct MemberResult {             // what an engine said about a planned member
    int32_t  status;
    uint64_t out_len, in_used;
};

// is the planned member genuine?  (The trailer was compared on the device: status 1 says check value and ISIZE agree.)  Only
// the member that was guessed to reach the end of the file may stop short of its span: what is left is the next member, or
// garbage.
inline bool member_verified(const PlannedMember &m, const MemberResult &r) {
    return r.status == 1 && r.out_len == m.out_guess && (m.to_end ? r.in_used <= m.span && r.in_used > 0 : r.in_used == m.span);
}

// index of the first planned member that is not genuine (every one behind it began at a guess that it refutes), or items.size()
inline size_t first_unverified(const MembersPlan &plan, const MemberResult *res) {
    for (size_t k = 0; k < plan.items.size(); ++k)
        if (!member_verified(plan.items[k], res[k])) return k;
    return plan.items.size();
}

// ---- behind a complete member (gz_look, gzread.c.in:122-140) ------------------------------------------------------------
enum AfterMember { kAfterDone = 0,   // nothing, one byte (gz_look asks avail_in > 1) or no 1f 8b: trailing garbage, ignored
                   kAfterMember };   // 1f 8b: a member that has to decode
// b0 / b1: the two bytes at `at` (looked at only when they exist)
inline AfterMember after_member(uint64_t at, uint64_t src_len, uint32_t b0, uint32_t b1) {
    if (src_len - at < 2) return kAfterDone;
    return b0 == 0x1fu && b1 == 0x8bu ? kAfterMember : kAfterDone;
}

}  // namespace zr
