// Drives walk_chain (zlib-ng_amd/csrc/inflate_large_plan.h) twice over the same tables, without and with Chain::record, for
// tests/test_inflate_index_cpu.py.  Input, whitespace-separated integers:
//   np window_len src_len sub
//   np starts, np keys, np x 8 result words, np x 8 side words
// Output: per walk "ok|fail produced end_bit final copies", then "cands:" and one "bit out_off" pair per candidate recorded.
#include <cstdio>
#include <iostream>
#include <vector>

#include "inflate_large_plan.h"

int main() {
    size_t np;
    uint32_t window_len;
    uint64_t src_len;
    int sub;
    if (!(std::cin >> np >> window_len >> src_len >> sub)) return 2;
    std::vector<unsigned long long> starts(np), keys(np);
    std::vector<uint32_t> res(np * 8), side(np * 8), marks(np * 4, 0);
    for (auto &v : starts) std::cin >> v;
    for (auto &v : keys) std::cin >> v;
    for (auto &v : res) std::cin >> v;
    for (auto &v : side) std::cin >> v;
    if (!std::cin) return 2;
    std::vector<uint16_t> slots(np);
    std::vector<uint16_t *> slot_ptr(np);
    for (size_t g = 0; g < np; ++g) slot_ptr[g] = &slots[g];
    for (int record = 0; record < 2; ++record) {
        zr::Chain c;
        c.record = record != 0;
        const bool ok = zr::walk_chain(res.data(), side.data(), marks.data(), slot_ptr.data(), 0, np, starts.data(), keys.data(), window_len,
                                       src_len, sub != 0, false, nullptr, c);
        printf("%s %llu %llu %d", ok ? "ok" : "fail", (unsigned long long)c.produced, c.end_bit, c.final ? 1 : 0);
        for (const zr::PartCopy &p : c.copies) printf(" %ld:%llu:%u", (long)(p.src - slots.data()), (unsigned long long)p.dst, p.n);
        printf("\n");
        if (record) {
            printf("cands:");
            for (const auto &k : c.cands) printf(" %llu %llu", k.first, (unsigned long long)k.second);
            printf("\n");
        }
    }
    return 0;
}
