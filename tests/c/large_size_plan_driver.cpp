// Drives zlib-ng_amd/csrc/inflate_large_size_plan.h on the host (tests/test_large_size_plan_cpu.py,
// tools/sanitize_inflate_large_size_plan.sh): the rules of the counting pass of the large sizing calls.  Commands (argv[1],
// numbers in argv[2..]):
//   walk PBASE NP WINDOW_LEN START0 NROWS (R0 .. R7) x NROWS   walk_size_chain over a hand-written result table of NROWS parts,
//                                      the stream's parts being [PBASE, PBASE + NP): "ok <produced> <end_bit> <parts>" or
//                                      "irregular <bad part or -1> <reason>"
//   job FORMAT HAVE_SRC SRC_LEN HAVE_WINDOW WINDOW_LEN         ls_job_ok: 0 / 1
//   round BYTES                                                ls_round_ok: 0 / 1
//   tail FORMAT AT SRC_LEN                                     ls_member_tail: "<status> <in_used>"
//   row W0 W1 W2 W3 W4                                         ls_stream_row: "<out_len> <used> <status> <msg>"
//   self                                                       all of the above over many values, for the sanitizers
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string_view>
#include <vector>

#include "inflate_large_size_plan.h"

namespace {

uint64_t num(char **argv, int i) { return strtoull(argv[i], nullptr, 0); }

void walk_print(const std::vector<uint32_t> &res, size_t pbase, size_t np, uint32_t window_len, unsigned long long start0) {
    std::vector<unsigned long long> starts(np ? np : 1, start0);
    zr::SizeChain c;
    if (zr::walk_size_chain(res.data(), pbase, np, starts.data(), window_len, c))
        printf("ok %llu %llu %zu\n", (unsigned long long)c.produced, c.end_bit, c.parts);
    else
        printf("irregular %ld %s\n", c.bad_part == ~(size_t)0 ? -1L : (long)c.bad_part, c.reason);
}

// a chain of n parts, each ending on the next, the last on the BFINAL block; counts of `each` bytes
std::vector<uint32_t> clean_chain(size_t n, uint64_t each) {
    std::vector<uint32_t> res(8 * n, 0u);
    for (size_t i = 0; i < n; ++i) {
        uint32_t *r = &res[8 * i];
        r[0] = (uint32_t)each;
        r[7] = (uint32_t)(each >> 32);
        r[1] = (uint32_t)(1000 * (i + 1));
        r[3] = i + 1 == n ? 1u : 0u;
        r[6] = i + 1 == n ? 0xffffffffu : (uint32_t)(i + 1);
    }
    return res;
}

int self() {
    using namespace zr;
    static uint8_t some[4];
    uint64_t checked = 0;
    for (int format = -1; format <= 3; ++format)
        for (uint64_t len : {0ull, 1ull, 1ull << 17, (1ull << 31) - 1, 1ull << 31, 1ull << 40})
            for (uint32_t wl : {0u, 1u, 32768u, 32769u, 0xffffffffu})
                for (int have = 0; have < 4; ++have) checked += ls_job_ok(format, have & 1 ? some : nullptr, len, have & 2 ? some : nullptr, wl);
    for (size_t b : {(size_t)0, (size_t)1, kRoundMin - 1, kRoundMin, kRoundEnd - 1, kRoundEnd, ~(size_t)0}) checked += ls_round_ok(b);
    for (int format = 0; format <= 2; ++format)
        for (uint64_t at : {0ull, 5ull, 100ull, (1ull << 31)})
            for (uint64_t len : {0ull, 5ull, 104ull, 108ull, (1ull << 31) + 8}) {
                int status = 0;
                uint64_t used = 0;
                ls_member_tail(format, at, len, &status, &used);
                if (used > len && status != 1) return 2;
                checked += status == 1;
            }
    // chains: clean ones of many sizes and counts up to the wrap, every word of one part damaged in turn
    for (size_t n : {1u, 2u, 7u, 500u})
        for (uint64_t each : {0ull, 1ull, 0xffffffffull, 0x100000000ull, ~0ull / 500, ~0ull / 2 + 1}) {
            std::vector<uint32_t> res = clean_chain(n, each);
            std::vector<unsigned long long> starts(n, 0);
            SizeChain c;
            const bool ok = walk_size_chain(res.data(), 0, n, starts.data(), 0, c);
            const bool wraps = n > 1 && each > ~0ull / n;
            if (ok == wraps) return 3;
            if (ok && (c.produced != each * n || c.parts != n)) return 4;
            for (size_t k = 0; k < 8 * n && n <= 7; ++k)
                for (uint32_t v : {0u, 1u, 5u, 0x7fffffffu, 0xffffffffu}) {
                    std::vector<uint32_t> bad = res;
                    bad[k] = v;
                    SizeChain d;
                    checked += walk_size_chain(bad.data(), 0, n, starts.data(), 32768, d);
                    if (d.parts > n) return 5;            // (a bad link never sends the walk round in a circle)
                }
        }
    const uint32_t w[5] = {0xfffffffeu, 0x3u, 77u, (uint32_t)-5, 12u};
    const LsRow r = ls_stream_row(w);
    if (r.out_len != 0x3fffffffeull || r.used != 77u || (int32_t)r.status != -5 || r.msg != 12u) return 6;
    printf("self ok (%llu accepted)\n", (unsigned long long)checked);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    using namespace zr;
    if (argc < 2) return 64;
    const std::string_view cmd = argv[1];
    if (cmd == "self") return self();
    if (cmd == "walk" && argc >= 7) {
        const size_t pbase = num(argv, 2), np = num(argv, 3), nrows = num(argv, 6);
        if (argc != 7 + 8 * (int)nrows || pbase + np > nrows || !np) return 64;
        std::vector<uint32_t> res(8 * nrows);
        for (size_t i = 0; i < 8 * nrows; ++i) res[i] = (uint32_t)num(argv, 7 + (int)i);
        walk_print(res, pbase, np, (uint32_t)num(argv, 4), num(argv, 5));
        return 0;
    }
    if (cmd == "job" && argc == 7) {
        static uint8_t some[4];
        printf("%d\n", ls_job_ok((int)strtol(argv[2], nullptr, 0), num(argv, 3) ? some : nullptr, num(argv, 4), num(argv, 5) ? some : nullptr,
                                 (uint32_t)num(argv, 6)) ? 1 : 0);
        return 0;
    }
    if (cmd == "round" && argc == 3) {
        printf("%d\n", ls_round_ok((size_t)num(argv, 2)) ? 1 : 0);
        return 0;
    }
    if (cmd == "tail" && argc == 5) {
        int status = 0;
        uint64_t used = 0;
        ls_member_tail((int)num(argv, 2), num(argv, 3), num(argv, 4), &status, &used);
        printf("%d %llu\n", status, (unsigned long long)used);
        return 0;
    }
    if (cmd == "row" && argc == 7) {
        const uint32_t w[5] = {(uint32_t)num(argv, 2), (uint32_t)num(argv, 3), (uint32_t)num(argv, 4), (uint32_t)num(argv, 5), (uint32_t)num(argv, 6)};
        const LsRow r = ls_stream_row(w);
        printf("%llu %u %d %u\n", (unsigned long long)r.out_len, r.used, (int)(int32_t)r.status, r.msg);
        return 0;
    }
    return 64;
}
