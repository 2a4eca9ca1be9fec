// Drives the rules of zlib-ng_amd/csrc/inflate_large_plan.h with tables read from stdin (tests/test_large_plan_cpu.py
// writes them by hand).  Without an argument: walk_chain and group_segments.  Input, whitespace-separated integers:
//   rows pbase np window_len src_len sub blocks
//   np starts, np keys, rows x 8 result words, rows x 8 side words, rows x 4 marks
// Output: "ok" or "fail <bad part or -1> <reason>", then
//   produced end_bit final subparts
//   copies: one "part dst n" per copy (part = row of the tables whose slot it reads)
//   segs: the first copy of every segment, and the number of copies behind them
// With an argument, another rule:
//   layout  in: np sub blocks slot_symbols
//           out: jobs starts keys res extra slots up_bytes res_words mirror_bytes device_bytes (part_tables)
//   retry   in: limit_bytes nstreams, nstreams x (first n), rows, rows part_bytes, rows messages (result word 4)
//           out: "again:" rows, "off:", "cap:", "total:" one number, "over:" streams (plan_retry)
//   chainfull  in: i0 i1 rows, rows x (message, "ended on BFINAL", link) -- result words 4, 3, 6
//           out: the row of the first full part on the chain from row i0, "end" (the chain ends without one) or "broken"
//           (first_full_on_chain)
//   segs    in: nstreams, per stream: produced dst ncopies, ncopies x (dst n); a copy's slot is its number over all streams
//           out: "v:" per stream, "copies:" one "slot dst gstart n first" per copy, "segs:" the middle word of every triple,
//                "seg_dst:", "seg_end:", "v_end:" one number (symbol_tables)
//   finder  in: ns, ns scanned lengths, nsurvivors, the survivors (64-bit words as the kernels write them: bit position, tag
//               in bits 40-61, marks in bits 62 and 63)
//           out: "plan:" item_bytes cap1 cap2 first nitems share, "items:" one "stream lo hi" per item (find_plan),
//                "patterns_first:" per stream (patterns_first of its length), then one "list:" per stream with its survivors,
//                sorted (find_demux; the first half of the survivors is given as the run that came back with the counts, the
//                second as the rest)
#include <cstdio>
#include <cstring>
#include <iostream>
#include <vector>

#include "inflate_large_plan.h"

static void line(const char *name, const std::vector<uint64_t> &v) {
    printf("%s", name);
    for (uint64_t x : v) printf(" %llu", (unsigned long long)x);
    printf("\n");
}

static int layout() {
    size_t np;
    int sub, blocks;
    uint64_t slot_symbols;
    if (!(std::cin >> np >> sub >> blocks >> slot_symbols)) return 2;
    const zr::PartTables t = zr::part_tables(np, sub != 0, blocks != 0, slot_symbols);
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", t.jobs, t.starts, t.keys, t.res, t.extra, t.slots, t.up_bytes, t.res_words,
           t.mirror_bytes, t.device_bytes);
    return 0;
}

static int retry() {
    uint64_t limit;
    size_t ns, rows;
    if (!(std::cin >> limit >> ns)) return 2;
    std::vector<std::pair<size_t, size_t>> spans(ns);
    for (auto &sp : spans) std::cin >> sp.first >> sp.second;
    if (!(std::cin >> rows)) return 2;
    std::vector<uint64_t> part_bytes(rows);
    std::vector<uint32_t> res(8 * rows, 0);
    for (auto &x : part_bytes) std::cin >> x;
    for (size_t i = 0; i < rows; ++i) std::cin >> res[8 * i + 4];
    if (!std::cin) return 2;
    const zr::RetryPlan r = zr::plan_retry(res.data(), spans, part_bytes.data(), limit);
    line("again:", std::vector<uint64_t>(r.again.begin(), r.again.end()));
    line("off:", r.off);
    line("cap:", r.cap);
    line("total:", {r.total});
    line("over:", std::vector<uint64_t>(r.over.begin(), r.over.end()));
    return 0;
}

static int chainfull() {
    size_t i0, i1, rows;
    if (!(std::cin >> i0 >> i1 >> rows)) return 2;
    std::vector<uint32_t> res(8 * rows, 0);
    for (size_t i = 0; i < rows; ++i) std::cin >> res[8 * i + 4] >> res[8 * i + 3] >> res[8 * i + 6];
    if (!std::cin || i0 >= i1 || i1 > rows) return 2;
    const size_t at = zr::first_full_on_chain(res.data(), i0, i1);
    if (at == i1) printf("end\n");
    else if (at > i1) printf("broken\n");
    else printf("%zu\n", at);
    return 0;
}

static int segs() {
    size_t ns;
    if (!(std::cin >> ns)) return 2;
    std::vector<std::vector<zr::PartCopy>> copies(ns);
    std::vector<zr::SymStream> streams;
    static uint16_t slots[1];
    size_t slot = 0;
    for (size_t k = 0; k < ns; ++k) {
        uint64_t produced, dst;
        size_t nc;
        if (!(std::cin >> produced >> dst >> nc)) return 2;
        for (size_t c = 0; c < nc; ++c) {
            uint64_t d;
            uint32_t n;
            if (!(std::cin >> d >> n)) return 2;
            copies[k].push_back(zr::PartCopy{slots + slot++, d, 0, n, 0u});
        }
        streams.push_back(zr::SymStream{&copies[k], produced, dst});
    }
    const zr::SymTables t = zr::symbol_tables(streams);
    std::vector<uint64_t> v, mid;
    for (const zr::SymStream &s : streams) v.push_back(s.v);
    for (size_t i = 1; i < t.segs.size(); i += 3) mid.push_back(t.segs[i]);
    line("v:", v);
    printf("copies:");
    for (const zr::PartCopy &p : t.copies)
        printf(" %ld %llu %llu %u %u", (long)(p.src - slots), (unsigned long long)p.dst, (unsigned long long)p.gstart, p.n, p.first);
    printf("\n");
    line("segs:", mid);
    line("seg_dst:", t.seg_dst);
    line("seg_end:", t.seg_end);
    line("v_end:", {t.v_end});
    return 0;
}

static int finder() {
    size_t ns, n;
    if (!(std::cin >> ns)) return 2;
    std::vector<uint64_t> lens(ns);
    for (auto &x : lens) std::cin >> x;
    if (!(std::cin >> n)) return 2;
    std::vector<unsigned long long> got(n);
    for (auto &x : got) std::cin >> x;
    if (!std::cin) return 2;
    const zr::FindPlan p = zr::find_plan(lens.data(), ns);
    std::vector<zr::FindItemDev> items(p.nitems + 1, zr::FindItemDev{~0ull, ~0ull, ~0u, ~0u});      // (one more: nothing is written there)
    zr::find_items(lens.data(), ns, p.share, items.data());
    if (items.back().stream != ~0u) return 3;
    items.pop_back();
    printf("plan: %llu %u %u %u %zu %llu\nitems:", (unsigned long long)p.item_bytes, p.cap1, p.cap2, p.first, p.nitems, (unsigned long long)p.share);
    for (const zr::FindItemDev &it : items) printf(" %u %llu %llu", it.stream, it.lo, it.hi);
    printf("\npatterns_first:");
    for (uint64_t len : lens) printf(" %u", zr::patterns_first((size_t)len));
    printf("\n");
    for (const auto &list : zr::find_demux(got.data(), n / 2, got.data() + n / 2, n - n / 2, ns))
        line("list:", std::vector<uint64_t>(list.begin(), list.end()));
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1)
        return !strcmp(argv[1], "layout") ? layout() : !strcmp(argv[1], "retry") ? retry() : !strcmp(argv[1], "chainfull") ? chainfull()
               : !strcmp(argv[1], "segs") ? segs() : !strcmp(argv[1], "finder") ? finder() : 2;
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
