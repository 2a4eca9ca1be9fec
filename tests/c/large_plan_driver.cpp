// Drives walk_chain and group_segments of zlib-ng_amd/csrc/inflate_large_plan.h with tables read from stdin
// (tests/test_large_plan_cpu.py writes them by hand).  Input, whitespace-separated integers:
//   rows pbase np window_len src_len sub blocks
//   np starts, np keys, rows x 8 result words, rows x 8 side words, rows x 4 marks
// Output: "ok" or "fail <bad part or -1> <reason>", then
//   produced end_bit final subparts
//   copies: one "part dst n" per copy (part = row of the tables whose slot it reads)
//   segs: the first copy of every segment, and the number of copies behind them
#include <cstdio>
#include <iostream>
#include <vector>

#include "inflate_large_plan.h"

int main() {
    size_t rows, pbase, np;
    uint32_t window_len;
    uint64_t src_len;
    int sub, blocks;
    if (!(std::cin >> rows >> pbase >> np >> window_len >> src_len >> sub >> blocks)) return 2;
    std::vector<unsigned long long> starts(np), keys(np);
    std::vector<uint32_t> res(8 * rows), side(8 * rows), marks(4 * rows);
    for (auto &x : starts) std::cin >> x;
    for (auto &x : keys) std::cin >> x;
    for (auto &x : res) std::cin >> x;
    for (auto &x : side) std::cin >> x;
    for (auto &x : marks) std::cin >> x;
    if (!std::cin) return 2;
    std::vector<uint16_t> slots(rows);
    std::vector<uint16_t *> slot_ptr(rows);
    for (size_t g = 0; g < rows; ++g) slot_ptr[g] = &slots[g];
    zr::Chain c;
    const bool ok = zr::walk_chain(res.data(), side.data(), marks.data(), slot_ptr.data(), pbase, np, starts.data(), keys.data(),
                                   window_len, src_len, sub != 0, blocks != 0, nullptr, c);
    if (ok) printf("ok\n");
    else printf("fail %ld %s\n", c.bad_part == ~(size_t)0 ? -1l : (long)c.bad_part, c.reason);
    printf("%llu %llu %d %zu\ncopies:", (unsigned long long)c.produced, c.end_bit, c.final ? 1 : 0, c.subparts);
    for (const zr::PartCopy &p : c.copies) printf(" %ld %llu %u", (long)(p.src - slots.data()), (unsigned long long)p.dst, p.n);
    printf("\nsegs:");
    if (ok)
        for (size_t f : zr::group_segments(c.copies, c.produced)) printf(" %zu", f);
    printf("\n");
    return 0;
}
