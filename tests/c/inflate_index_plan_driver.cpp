// Drives zlib-ng_amd/csrc/inflate_index_plan.h on the host (tests/test_inflate_index_cpu.py; tools/sanitize_inflate_index_plan.sh
// runs "self" under ASan / UBSan).  The command is argv[1]; its numbers come from standard input, separated by white space.
//   span     SPAN_BYTES                                          "<span>" (0: refused)
//   scratch  SCRATCH_BYTES                                       "<scratch>" (0: refused)
//   select   SPAN PLAIN_LEN HEADER_LEN N, then N candidates BIT OUT_OFF
//                                                                one "in_bit out_off window_len" per point
//   plan     PLAIN_LEN SCRATCH ROUND_JOBS N NRANGES, then N points IN_BIT OUT_OFF WINDOW_LEN, then NRANGES ranges UOFF LEN
//                                                                "<decoded> <direct> <jobs> <parts> <rounds>", the clipped lengths on
//                                                                one line, then "J span slot out_cap at range" (slot -1: direct),
//                                                                "P range job at off len slice" (job -1: none),
//                                                                "R range_begin range_end job_begin job_end part_begin part_end slot_bytes slices"
//   verdict  PRODUCED CONSUMED STATUS MSG OUT_CAP                "<status> <msg>" (index_job_verdict; msg -1 mismatch)
//   result   CLIPPED NPARTS NVERDICTS, then NPARTS parts JOB AT (job -1: none), then NVERDICTS verdicts STATUS MSG
//                                                                "<status> <out_len> <msg>" (index_range_result; msg -2 too long)
//   write    FORMAT HEADER_LEN SRC_END PLAIN_LEN SPAN N, then N points
//                                                                the header and rows as bytes, one line (index_blob_write)
//   check    LEN, then LEN bytes                                 "<why>", then on 0 "format header_len src_end plain_len span", the points
//   self     a fixed run through every function, for the sanitizers; prints "ok"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "inflate_index_plan.h"

namespace {

using namespace zr;

uint64_t next() {
    char tok[64];
    if (scanf("%63s", tok) != 1) {
        fprintf(stderr, "input ended early\n");
        exit(2);
    }
    if (tok[0] == '-') return (uint64_t)strtoll(tok, nullptr, 0);
    return strtoull(tok, nullptr, 0);
}

std::vector<zng_rocm_access_point> points(size_t n) {
    std::vector<zng_rocm_access_point> p(n);
    for (auto &r : p) {
        r.in_bit = next();
        r.out_off = next();
        r.window_len = (uint32_t)next();
        r.reserved = 0;
    }
    return p;
}

void print_points(const std::vector<zng_rocm_access_point> &pts) {
    for (const auto &p : pts) printf("%" PRIu64 " %" PRIu64 " %u\n", p.in_bit, p.out_off, p.window_len);
}

void print_plan(const IndexReadPlan &plan) {
    printf("%" PRIu64 " %" PRIu64 " %zu %zu %zu\n", plan.decoded, plan.direct, plan.jobs.size(), plan.parts.size(), plan.rounds.size());
    for (uint64_t c : plan.clipped) printf("%" PRIu64 " ", c);
    printf("\n");
    for (const IndexReadJob &j : plan.jobs)
        printf("J %" PRIu64 " %" PRId64 " %" PRIu64 " %" PRIu64 " %u\n", j.span, (int64_t)j.slot, j.out_cap, j.at, j.range);
    for (const IndexReadPart &p : plan.parts)
        printf("P %u %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", p.range, (int)p.job, p.at, p.off, p.len, p.slice);
    for (const IndexReadRound &r : plan.rounds)
        printf("R %zu %zu %zu %zu %zu %zu %" PRIu64 " %u\n", r.range_begin, r.range_end, r.job_begin, r.job_end, r.part_begin, r.part_end,
               r.slot_bytes, r.slices);
}

int self() {
    // candidates of two pieces (the second begins with the first's last stop), an empty block, one at plain_len
    const std::vector<IndexCand> cands = {{80, 0}, {9000, 70000}, {9100, 70000}, {20000, 140000}, {20000, 140000}, {31000, 200000},
                                          {40000, 300000}};
    std::vector<zng_rocm_access_point> pts;
    index_select(cands.data(), cands.size(), 65536, 300000, 10, pts);
    if (pts.size() != 3 || pts[1].in_bit != 9000 || pts[2].out_off != 140000 || pts[2].window_len != 32768) return 1;
    std::vector<uint64_t> woff;
    index_window_offsets(pts.data(), pts.size(), woff);
    if (woff.back() != 65536) return 2;
    const std::vector<IndexRangeIn> ranges = {{0, 10}, {69990, 20}, {60000, 100000}, {299999, 5}, {400000, 1}, {69000, 2000}};
    IndexReadPlan plan;
    index_read_plan(pts.data(), pts.size(), 300000, ranges.data(), ranges.size(), 1u << 20, kIndexRoundJobs, plan);
    if (plan.rounds.size() != 1 || plan.direct != 1 || plan.clipped[3] != 1 || plan.clipped[4] != 0) return 3;
    index_read_plan(pts.data(), pts.size(), 300000, ranges.data(), ranges.size(), 70016, kIndexRoundJobs, plan);
    if (plan.rounds.size() < 2) return 4;
    std::vector<IndexJobVerdict> verdicts(plan.jobs.size(), IndexJobVerdict{1, 0u});
    verdicts[plan.parts[1].job] = IndexJobVerdict{-3, 1u};
    const uint32_t res[4] = {100, 7, 1, 0};
    if (index_job_verdict(res, 100).status != 1 || index_job_verdict(res, 101).msg != kIndexMsgMismatch) return 5;
    size_t k = 0;
    for (size_t r = 0; r < ranges.size(); ++r) {
        const size_t from = k;
        while (k < plan.parts.size() && plan.parts[k].range == r) ++k;
        const IndexRangeOut o = index_range_result(plan.parts.data() + from, k - from, verdicts.data(), plan.clipped[r]);
        if (r == 0 && (o.status != -3 || o.out_len != 0)) return 6;
    }
    // a span of 2 GiB and more has no job
    const std::vector<zng_rocm_access_point> big = {{0, 0, 0, 0}, {800, 1ull << 32, 32768, 0}};
    const std::vector<IndexRangeIn> br = {{100, 50}, {(1ull << 32) - 10, 20}};
    index_read_plan(big.data(), big.size(), (1ull << 32) + 1000, br.data(), br.size(), 1u << 20, kIndexRoundJobs, plan);
    if (plan.jobs.size() != 1 || plan.parts.size() != 3 || plan.parts[0].job != kIndexNoJob) return 7;
    std::vector<uint8_t> blob((size_t)index_blob_bytes(pts.data(), pts.size()), 0xa5);
    index_blob_write(IndexHead{2, 10, 5000, 300000, 65536}, pts.data(), pts.size(), blob.data());
    IndexHead head;
    std::vector<zng_rocm_access_point> back;
    if (index_blob_check(blob.data(), blob.size(), head, back) != kBlobOk || back.size() != 3 || head.src_end != 5000) return 8;
    if (index_blob_check(blob.data(), blob.size() - 1, head, back) != kBlobSize) return 9;
    blob[4] = 2;
    if (index_blob_check(blob.data(), blob.size(), head, back) != kBlobVersion) return 10;
    if (index_span_bytes(0) != kIndexSpanDefault || index_span_bytes(1) != 0 || index_scratch_bytes(0) != kIndexScratchDefault) return 11;
    printf("ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "self") return self();
    if (cmd == "span") {
        printf("%" PRIu64 "\n", index_span_bytes(next()));
    } else if (cmd == "scratch") {
        printf("%" PRIu64 "\n", index_scratch_bytes(next()));
    } else if (cmd == "select") {
        const uint64_t span = next(), plain_len = next(), header_len = next();
        std::vector<IndexCand> c((size_t)next());
        for (auto &x : c) {
            x.bit = next();
            x.out_off = next();
        }
        std::vector<zng_rocm_access_point> pts;
        index_select(c.data(), c.size(), span, plain_len, header_len, pts);
        print_points(pts);
    } else if (cmd == "plan") {
        const uint64_t plain_len = next(), scratch = next(), round_jobs = next();
        const size_t n = (size_t)next(), nranges = (size_t)next();
        const std::vector<zng_rocm_access_point> pts = points(n);
        std::vector<IndexRangeIn> ranges(nranges);
        for (auto &r : ranges) {
            r.uoff = next();
            r.len = next();
        }
        IndexReadPlan plan;
        index_read_plan(pts.data(), n, plain_len, ranges.data(), nranges, scratch, round_jobs, plan);
        print_plan(plan);
    } else if (cmd == "verdict") {
        const uint32_t res[4] = {(uint32_t)next(), (uint32_t)next(), (uint32_t)next(), (uint32_t)next()};
        const IndexJobVerdict v = index_job_verdict(res, (uint32_t)next());
        printf("%d %d\n", v.status, (int)v.msg);
    } else if (cmd == "result") {
        const uint64_t clipped = next();
        const size_t nparts = (size_t)next(), nv = (size_t)next();
        std::vector<IndexReadPart> parts(nparts);
        for (auto &p : parts) {
            p = IndexReadPart{0u, (uint32_t)next(), 0u, 0u, 0u, 0u};
            p.at = next();
        }
        std::vector<IndexJobVerdict> v(nv);
        for (auto &x : v) {
            x.status = (int32_t)next();
            x.msg = (uint32_t)next();
        }
        const IndexRangeOut o = index_range_result(parts.data(), nparts, v.data(), clipped);
        printf("%d %" PRIu64 " %d\n", o.status, o.out_len, (int)o.msg);
    } else if (cmd == "write") {
        IndexHead h;
        h.format = (uint32_t)next();
        h.header_len = next();
        h.src_end = next();
        h.plain_len = next();
        h.span_bytes = next();
        const std::vector<zng_rocm_access_point> pts = points((size_t)next());
        std::vector<uint8_t> buf(kIndexBlobHead + kIndexBlobRow * pts.size());
        index_blob_write(h, pts.data(), pts.size(), buf.data());
        for (uint8_t b : buf) printf("%u ", b);
        printf("\n");
    } else if (cmd == "check") {
        std::vector<uint8_t> buf((size_t)next());
        for (auto &b : buf) b = (uint8_t)next();
        IndexHead h;
        std::vector<zng_rocm_access_point> pts;
        const uint32_t why = index_blob_check(buf.data(), buf.size(), h, pts);
        printf("%u\n", why);
        if (!why) {
            printf("%u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", h.format, h.header_len, h.src_end, h.plain_len, h.span_bytes);
            print_points(pts);
        }
    } else {
        return 2;
    }
    return 0;
}
