// Drives zlib-ng_amd/csrc/bgzf_read_plan.h on the host (tests/test_bgzf_read_cpu.py; tools/sanitize_bgzf_read_plan.sh runs
// "self" under ASan / UBSan).  The command is argv[1]; its numbers come from standard input, separated by white space.
//   flags    BGZF CUT POS END HEADER_LEN SRC_LEN                  "<flags>" (bgzf_index_flags)
//   walk     SRC_LEN LOOK CAP N, then N rows POS END HEADER_LEN CRC ISIZE FLAGS
//                                                                 "<status> <why> <at> <plain_len> <nmembers>", then the rows written
//   check    SRC_LEN N, then N members                            "<why> <bad>" (bgzf_read_rows_check)
//   slots    SCRATCH_BYTES                                        "<slots>" (0: refused)
//   plan     SLOTS ROUND_JOBS N NRANGES, then N members, then NRANGES ranges UOFF LEN
//                                                                 "<decoded> <direct> <jobs> <parts> <rounds>", the clipped lengths on one
//                                                                 line, then "J member slot range at", "P range job at off len slice",
//                                                                 "R range_begin range_end job_begin job_end part_begin part_end slots slices"
//   verdict  PRODUCED CONSUMED STATUS MSG SRC_LEN OUT_LEN         "<status> <msg>" (bgzf_job_verdict)
//   result   CLIPPED NPARTS NVERDICTS, then NPARTS parts JOB AT, then NVERDICTS verdicts STATUS MSG
//                                                                 "<status> <out_len> <has_msg> <msg>" (bgzf_range_result)
//   voff     N K, then N members, then K plaintext offsets        per offset "<voff>" or "refused"
//   uoff     N K, then N members, then K virtual offsets          per offset "<uoff>" or "refused"
//   self     a fixed run through every function, for the sanitizers; prints "ok"
// A member is SRC_OFF SRC_LEN DST_OFF OUT_LEN CRC BGZF.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bgzf_read_plan.h"

namespace {

using namespace zr;

uint64_t next() {
    unsigned long long v = 0;
    long long s = 0;
    char tok[64];
    if (scanf("%63s", tok) != 1) {
        fprintf(stderr, "input ended early\n");
        exit(2);
    }
    if (tok[0] == '-') {
        s = strtoll(tok, nullptr, 0);
        return (uint64_t)s;
    }
    v = strtoull(tok, nullptr, 0);
    return v;
}

std::vector<zng_rocm_gzip_member> members(size_t n) {
    std::vector<zng_rocm_gzip_member> m(n);
    for (auto &r : m) {
        r.src_off = next();
        r.src_len = next();
        r.dst_off = next();
        r.out_len = next();
        r.crc = (uint32_t)next();
        r.bgzf = (uint32_t)next();
    }
    return m;
}

void print_member(const zng_rocm_gzip_member &r) {
    printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u\n", r.src_off, r.src_len, r.dst_off, r.out_len, r.crc, r.bgzf);
}

void print_plan(const BgzfReadPlan &plan) {
    printf("%" PRIu64 " %" PRIu64 " %zu %zu %zu\n", plan.decoded, plan.direct, plan.jobs.size(), plan.parts.size(), plan.rounds.size());
    for (uint64_t c : plan.clipped) printf("%" PRIu64 " ", c);
    printf("\n");
    for (const BgzfReadJob &j : plan.jobs) printf("J %" PRIu64 " %u %u %" PRIu64 "\n", j.member, j.slot, j.range, j.at);
    for (const BgzfReadPart &p : plan.parts) printf("P %u %u %" PRIu64 " %u %u %u\n", p.range, p.job, p.at, p.off, p.len, p.slice);
    for (const BgzfReadRound &r : plan.rounds)
        printf("R %zu %zu %zu %zu %zu %zu %u %u\n", r.range_begin, r.range_end, r.job_begin, r.job_end, r.part_begin, r.part_end, r.slots,
               r.slices);
}

int self() {
    // three members of 100, 0 and 50 bytes and the end-of-file block, as an index table with a candidate inside the first
    std::vector<BgzfIndexRow> rows = {
        {0, 60, 18, 0x11, 100, bgzf_index_flags(true, false, 0, 60, 18, 186) | kIdxNextMagic},
        {30, 30, 0, 0, 0, bgzf_index_flags(false, false, 30, 30, 0, 186)},
        {60, 88, 18, 0, 0, bgzf_index_flags(true, false, 60, 88, 18, 186) | kIdxNextMagic},
        {88, 158, 18, 0x22, 50, bgzf_index_flags(true, false, 88, 158, 18, 186) | kIdxNextMagic},
        {158, 186, 18, 0, 0, bgzf_index_flags(true, false, 158, 186, 18, 186)},
    };
    std::vector<zng_rocm_gzip_member> m(3);
    const BgzfIndexWalk w = bgzf_index_walk(rows.data(), (uint32_t)rows.size(), 186, 4096, m.data(), m.size());
    if (w.status != 0 || w.nmembers != 4 || w.plain_len != 150 || w.at != 186) return 1;
    m.resize(4);
    if (bgzf_index_walk(rows.data(), (uint32_t)rows.size(), 186, 4096, m.data(), m.size()).nmembers != 4) return 1;
    if (bgzf_index_walk(nullptr, 0, 0, 4096, nullptr, 0).status != 0 || bgzf_index_walk(nullptr, 0, 5, 4096, nullptr, 0).status != -5) return 1;
    size_t bad = 0;
    if (bgzf_read_rows_check(m.data(), m.size(), 186, &bad) != kRowsOk || bad != 4) return 1;
    if (bgzf_read_rows_check(m.data(), m.size(), 185, &bad) != kRowsOutside || bad != 3) return 1;
    std::vector<BgzfRangeIn> ranges;
    for (uint64_t u = 0; u <= 151; ++u)
        for (uint64_t len : {0ull, 1ull, 49ull, 50ull, 100ull, 151ull, ~0ull}) ranges.push_back(BgzfRangeIn{u, len});
    BgzfReadPlan plan;
    for (uint64_t slots : {2ull, 3ull, 4096ull})
        for (uint64_t round_jobs : {1ull, 5ull, 1ull << 22}) {
            bgzf_read_plan(m.data(), m.size(), ranges.data(), ranges.size(), slots, round_jobs, plan);
            uint64_t bytes = 0, want = 0;
            for (const BgzfReadPart &p : plan.parts) bytes += p.len;
            for (uint64_t c : plan.clipped) want += c;
            if (bytes != want) return 1;
            std::vector<BgzfJobVerdict> verdicts(plan.jobs.size(), BgzfJobVerdict{1, 0});
            const uint32_t res[4] = {100, 59, 1, 0};
            if (!verdicts.empty()) verdicts[0] = bgzf_job_verdict(res, m[0]);
            size_t k = 0;
            for (size_t r = 0; r < ranges.size(); ++r) {
                const size_t from = k;
                while (k < plan.parts.size() && plan.parts[k].range == r) ++k;
                const BgzfRangeOut o = bgzf_range_result(plan.parts.data() + from, k - from, verdicts.data(), plan.clipped[r]);
                if (o.status == 1 && o.out_len != plan.clipped[r]) return 1;
            }
            if (k != plan.parts.size()) return 1;
        }
    bgzf_read_plan(nullptr, 0, ranges.data(), ranges.size(), 2, 1, plan);
    if (!plan.jobs.empty() || bgzf_read_slots(0) != 4096 || bgzf_read_slots(1) != 0) return 1;
    for (uint64_t u = 0; u <= 151; ++u) {
        uint64_t v = 0, back = 0;
        const bool ok = bgzf_voffset(m.data(), m.size(), u, &v);
        if (ok != (u <= 150) || (ok && (!bgzf_uoffset(m.data(), m.size(), v, &back) || back != u))) return 1;
    }
    uint64_t v = 0;
    if (bgzf_voffset(nullptr, 0, 0, &v) || bgzf_uoffset(nullptr, 0, 0, &v) || bgzf_uoffset(m.data(), m.size(), (60ull << 16) | 1, &v)) return 1;
    printf("ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "self") return self();
    if (cmd == "flags") {
        const bool bgzf = next() != 0, cut = next() != 0;
        const uint64_t pos = next(), end = next(), header_len = next(), src_len = next();
        printf("%u\n", bgzf_index_flags(bgzf, cut, pos, end, header_len, src_len));
        return 0;
    }
    if (cmd == "walk") {
        const uint64_t src_len = next(), look = next();
        const size_t cap = (size_t)next();
        const uint32_t n = (uint32_t)next();
        std::vector<BgzfIndexRow> rows(n);
        for (auto &r : rows) {
            r.pos = next();
            r.end = next();
            r.header_len = (uint32_t)next();
            r.crc = (uint32_t)next();
            r.isize = (uint32_t)next();
            r.flags = (uint32_t)next();
        }
        std::vector<zng_rocm_gzip_member> m(cap);
        const BgzfIndexWalk w = bgzf_index_walk(rows.data(), n, src_len, look, cap ? m.data() : nullptr, cap);
        printf("%d %u %" PRIu64 " %" PRIu64 " %zu\n", w.status, w.why, w.at, w.plain_len, w.nmembers);
        for (size_t k = 0; k < cap && k < w.nmembers; ++k) print_member(m[k]);
        return 0;
    }
    if (cmd == "check") {
        const uint64_t src_len = next();
        const std::vector<zng_rocm_gzip_member> m = members((size_t)next());
        size_t bad = 0;
        const uint32_t why = bgzf_read_rows_check(m.data(), m.size(), src_len, &bad);
        printf("%u %zu\n", why, bad);
        return 0;
    }
    if (cmd == "slots") {
        printf("%" PRIu64 "\n", bgzf_read_slots(next()));
        return 0;
    }
    if (cmd == "plan") {
        const uint64_t slots = next(), round_jobs = next();
        const size_t n = (size_t)next(), nranges = (size_t)next();
        const std::vector<zng_rocm_gzip_member> m = members(n);
        std::vector<BgzfRangeIn> ranges(nranges);
        for (auto &r : ranges) {
            r.uoff = next();
            r.len = next();
        }
        BgzfReadPlan plan;
        bgzf_read_plan(m.data(), n, ranges.data(), nranges, slots, round_jobs, plan);
        print_plan(plan);
        return 0;
    }
    if (cmd == "verdict") {
        uint32_t res[4];
        for (uint32_t &w : res) w = (uint32_t)next();
        zng_rocm_gzip_member row = {0, 0, 0, 0, 0, 1};
        row.src_len = next();
        row.out_len = next();
        const BgzfJobVerdict v = bgzf_job_verdict(res, row);
        printf("%d %u\n", v.status, v.msg);
        return 0;
    }
    if (cmd == "result") {
        const uint64_t clipped = next();
        const size_t nparts = (size_t)next(), nverdicts = (size_t)next();
        std::vector<BgzfReadPart> parts(nparts);
        for (auto &p : parts) {
            p = BgzfReadPart{0, 0, 0, 0, 0, 0};
            p.job = (uint32_t)next();
            p.at = next();
        }
        std::vector<BgzfJobVerdict> verdicts(nverdicts);
        for (auto &v : verdicts) {
            v.status = (int32_t)next();
            v.msg = (uint32_t)next();
        }
        const BgzfRangeOut o = bgzf_range_result(parts.data(), nparts, verdicts.data(), clipped);
        printf("%d %" PRIu64 " %d %u\n", o.status, o.out_len, o.has_msg ? 1 : 0, o.msg);
        return 0;
    }
    if (cmd == "voff" || cmd == "uoff") {
        const size_t n = (size_t)next(), k = (size_t)next();
        const std::vector<zng_rocm_gzip_member> m = members(n);
        for (size_t i = 0; i < k; ++i) {
            uint64_t out = 0;
            const uint64_t v = next();
            const bool ok = cmd == "voff" ? bgzf_voffset(m.data(), n, v, &out) : bgzf_uoffset(m.data(), n, v, &out);
            if (ok) printf("%" PRIu64 "\n", out);
            else printf("refused\n");
        }
        return 0;
    }
    fprintf(stderr, "unknown command\n");
    return 2;
}
