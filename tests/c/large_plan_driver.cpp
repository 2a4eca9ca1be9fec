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
//   pieces  the rules of the pieces loop; in: an operation and its numbers, a state being "bit key fin produced abit aout p"
//           next     state src_len piece_bytes
//                    out: "next:" any end base start_bit scan_lo key0 fin0 last q (piece_next)
//           pass     state src_len piece_bytes, then what the pass over that next piece said: stopped next_bit next_key next_fin
//                    (PiecePass's out fields, the pass's own positions) out used
//                    out: "step:" done in_used anchored, "state:" the state behind it (piece_after_pass)
//           halve    p   out: "halve:" allowed, the p behind it (piece_halve)
//           history  pos window_len   out: "history:" len where (0 output, 1 the window, 2 spliced) dst_off window_off
//                    from_window from_dst (piece_history)
//           seq      state src_len n, n x (status, end bit): the sequential decoder's answers in turn
//                    out: "seq:" a0 sb span len (seq_input), per answer "turn:" more span len stream_form (seq_wants_more,
//                    seq_stream_form)
//           blocks   state eb produced piece_bytes   out: "state:" (piece_after_blocks, from seq_input of the state)
//   self    no input: steps the pieces state machine over synthetic pass outcomes for a sweep of src_len, piece_bytes and
//           keys, and checks what must hold at every step (tools/sanitize_inflate_large_plan.sh runs it under ASan + UBSan)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
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

static bool read_state(zr::PiecesState &s) { return (bool)(std::cin >> s.bit >> s.key >> s.fin >> s.produced >> s.abit >> s.aout >> s.p); }
static void print_state(const zr::PiecesState &s) {
    printf("state: %llu %llu %d %llu %llu %llu %llu\n", (unsigned long long)s.bit, (unsigned long long)s.key, s.fin,
           (unsigned long long)s.produced, (unsigned long long)s.abit, (unsigned long long)s.aout, (unsigned long long)s.p);
}

static int pieces() {
    std::string op;
    zr::PiecesState s;
    uint64_t src_len, piece_bytes;
    if (!(std::cin >> op)) return 2;
    if (op == "next" || op == "pass") {
        if (!read_state(s) || !(std::cin >> src_len >> piece_bytes)) return 2;
        zr::NextPiece n = zr::piece_next(s, src_len, piece_bytes);
        if (op == "next") {
            line("next:", {n.any, n.end, n.base, n.start_bit, n.pp.scan_lo, n.pp.key0});
            printf("fin0: %d\n", n.pp.fin0);
            line("last:", {n.pp.last, n.pp.q});
            return 0;
        }
        int stopped;
        uint64_t out, used;
        if (!(std::cin >> stopped >> n.pp.next_bit >> n.pp.next_key >> n.pp.next_fin >> out >> used) || !n.any) return 2;
        n.pp.stopped = stopped != 0;
        const zr::PieceStep r = zr::piece_after_pass(s, n, out, used, piece_bytes);
        line("step:", {r.done, r.in_used, r.anchored});
        print_state(s);
        return 0;
    }
    if (op == "halve") {
        if (!(std::cin >> s.p)) return 2;
        const bool ok = zr::piece_halve(s);
        line("halve:", {ok, s.p});
        return 0;
    }
    if (op == "history") {
        uint64_t pos;
        uint32_t window_len;
        if (!(std::cin >> pos >> window_len)) return 2;
        const zr::PieceHistory h = zr::piece_history(pos, window_len);
        line("history:", {h.len, (uint64_t)h.where, h.dst_off, h.window_off, h.from_window, h.from_dst});
        return 0;
    }
    if (op == "seq") {
        size_t turns;
        if (!read_state(s) || !(std::cin >> src_len >> turns)) return 2;
        zr::SeqInput in = zr::seq_input(s);
        line("seq:", {in.a0, in.sb, in.span, in.len(src_len)});
        for (size_t t = 0; t < turns; ++t) {
            int status;
            uint64_t eb;
            if (!(std::cin >> status >> eb)) return 2;
            const bool more = zr::seq_wants_more(in, src_len, status, eb);
            line("turn:", {more, in.span, in.len(src_len), zr::seq_stream_form(status, eb, in.sb)});
        }
        return 0;
    }
    if (op == "blocks") {
        uint64_t eb, produced;
        if (!read_state(s) || !(std::cin >> eb >> produced >> piece_bytes)) return 2;
        zr::piece_after_blocks(s, zr::seq_input(s), eb, produced, piece_bytes);
        print_state(s);
        return 0;
    }
    return 2;
}

// ---- self: the pieces state machine over synthetic outcomes ----------------------------------------------------------------
#define CHECK(x)                                                              \
    do {                                                                      \
        if (!(x)) {                                                           \
            fprintf(stderr, "self: %s does not hold (line %d)\n", #x, __LINE__); \
            abort();                                                          \
        }                                                                     \
    } while (0)

// One call: passes whose outcome `rnd` draws -- stopped at a start inside the piece with a key of 0, 1 or H + 2 (H in front of
// the start: in the piece, or up to 70000 bytes in front of it), asked to halve, left to the sequential decoder, or the end.
static uint64_t self_call(uint64_t src_len, uint64_t piece_bytes, uint32_t window_len, uint64_t seed) {
    auto rnd = [&]() {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        return seed >> 33;
    };
    zr::PiecesState s = zr::pieces_begin(piece_bytes);
    uint64_t turns = 0;
    for (;; ++turns) {
        CHECK(turns < 100000);
        CHECK(s.abit <= s.bit && s.aout <= s.produced && s.p >= zr::kPieceMin && s.p <= piece_bytes);
        const uint64_t sbyte = s.bit >> 3;
        zr::NextPiece n = zr::piece_next(s, src_len, piece_bytes);
        CHECK(n.any == (sbyte < src_len));
        bool to_host = !n.any;
        if (n.any) {
            CHECK(n.base % 256 == 0 && n.base <= sbyte && sbyte < n.end && n.end <= src_len && n.end - sbyte <= s.p);
            CHECK(n.pp.scan_lo + n.base == sbyte && (n.start_bit >> 3) == n.pp.scan_lo && n.start_bit + 8 * n.base == s.bit);
            CHECK(n.pp.last == (n.end == src_len) && (n.pp.last || src_len - n.end >= s.p / 4) && n.pp.q == piece_bytes);
            if (s.key >= 2) CHECK(n.pp.key0 >= 2 && n.pp.key0 + 8 * n.base == s.key && ((n.pp.key0 - 2) >> 3) <= n.pp.scan_lo);
            else CHECK(n.pp.key0 == s.key);
            const zr::PieceHistory h = zr::piece_history(s.produced, window_len);
            CHECK(h.len == std::min<uint64_t>(32768, s.produced + window_len));
            if (h.where == zr::PieceHistory::kInDst) CHECK(h.dst_off + h.len == s.produced);
            if (h.where == zr::PieceHistory::kWindow) CHECK(s.produced == 0 && h.len == window_len);
            if (h.where == zr::PieceHistory::kSpliced)
                CHECK(h.from_dst == s.produced && h.from_window + h.from_dst == h.len && h.window_off + h.from_window == window_len);
            const unsigned what = (unsigned)(rnd() % 16);
            if (what == 0) {                               // asked to halve
                const uint64_t p0 = s.p;
                n.pp.halve = true;
                if (zr::piece_halve(s)) {
                    CHECK(s.p == p0 / 2 && s.p >= zr::kPieceMin);
                    continue;
                }
                CHECK(s.p == p0 && p0 / 2 < zr::kPieceMin);
                to_host = true;
            } else if (what == 1) {
                to_host = true;
            } else {
                const uint64_t bits = 8 * (n.end - sbyte) - (s.bit & 7), out = rnd() % 100000;
                zr::PiecesState t = s;
                if (n.pp.last && what < 6) {               // the stream ends in the piece
                    const uint64_t used = n.len() - rnd() % std::min<uint64_t>(n.len() - n.pp.scan_lo, 9);
                    const zr::PieceStep r = zr::piece_after_pass(t, n, out, used, piece_bytes);
                    CHECK(r.done && r.in_used == n.base + used && r.in_used <= src_len && r.in_used > sbyte && t.produced == s.produced + out);
                    return turns;
                }
                if (bits < 2) {
                    to_host = true;
                } else {
                    // stopped at a later start of the piece; the same start and key once, to see them come back as they went in
                    const bool same = what == 15 && turns % 2 == 0;
                    n.pp.stopped = true;
                    n.pp.next_bit = same ? n.start_bit : n.start_bit + 1 + rnd() % (bits - 1);
                    const uint64_t hmax = std::min<uint64_t>(n.pp.next_bit, 8 * 70000);
                    const unsigned kind = (unsigned)(rnd() % 3);
                    n.pp.next_key = same ? n.pp.key0 : kind < 2 ? kind : n.pp.next_bit - rnd() % (hmax + 1) + 2;
                    n.pp.next_fin = (int)(rnd() % 3) - 1;
                    const zr::PieceStep r = zr::piece_after_pass(t, n, out, 0, piece_bytes);
                    CHECK(!r.done && t.bit == n.pp.next_bit + 8 * n.base && t.fin == n.pp.next_fin && t.p == piece_bytes);
                    CHECK(same ? t.bit == s.bit && t.key == s.key : t.bit > s.bit);
                    CHECK(t.key < 2 ? t.key == n.pp.next_key : t.key == n.pp.next_key + 8 * n.base && t.key - 2 <= t.bit);
                    CHECK(r.anchored == (t.key == 0) && t.produced == s.produced + out);
                    if (r.anchored) CHECK(t.abit == t.bit && t.aout == t.produced);
                    else CHECK(t.abit == s.abit && t.aout == s.aout);
                    s = t;
                    if (same) s.p = piece_bytes, to_host = true;      // (no progress twice would be the device's bug, not the rules')
                    else continue;
                }
            }
        }
        CHECK(to_host);
        zr::SeqInput in = zr::seq_input(s);
        CHECK(8 * in.a0 + in.sb == s.abit && in.sb < 8 && in.a0 <= src_len);
        CHECK(in.span >= 2 * s.p && in.a0 + in.span >= std::min(sbyte, src_len) + s.p);
        const zr::PieceHistory h = zr::piece_history(s.aout, window_len);
        CHECK(h.len == std::min<uint64_t>(32768, s.aout + window_len));
        uint64_t eb = in.sb;
        int status = 0;
        for (;;) {
            const uint64_t len = in.len(src_len);
            CHECK(in.a0 + len <= src_len && (len == in.span || in.a0 + len == src_len));
            const unsigned what = (unsigned)(rnd() % 8);
            status = what == 0 ? -3 : what == 1 && in.a0 + len == src_len ? 1 : 0;
            if (8 * len <= in.sb) status = -3, eb = in.sb;       // (no input: nothing can complete)
            else eb = what >= 5 || status == 1 ? in.sb + 1 + rnd() % (8 * len - in.sb) : in.sb;
            const uint64_t span0 = in.span;
            if (!zr::seq_wants_more(in, src_len, status, eb)) {
                CHECK(in.span == span0);
                break;
            }
            CHECK(status == 0 && eb == in.sb && len < src_len - in.a0 && in.span == 2 * span0);
        }
        if (zr::seq_stream_form(status, eb, in.sb)) {
            CHECK(status < 0 || (status == 0 && eb == in.sb));
            return turns;                                  // the stream form's answer ends the call
        }
        CHECK(status == 1 || (status == 0 && eb != in.sb));
        if (status == 1) return turns;
        zr::PiecesState t = s;
        const uint64_t total = s.aout + rnd() % 100000;
        zr::piece_after_blocks(t, in, eb, total, piece_bytes);
        CHECK(t.bit == 8 * in.a0 + eb && t.bit > s.abit && t.key == 0 && t.fin == -1 && t.abit == t.bit);
        CHECK(t.produced == total && t.aout == total && t.p == piece_bytes);
        CHECK(in.a0 + zr::seq_blocks_bytes(eb) <= src_len && 8 * zr::seq_blocks_bytes(eb) >= eb);
        s = t;
    }
}

static int self() {
    const uint64_t M = 1u << 20;
    const uint64_t pieces[] = {zr::kPieceMin, zr::kPieceMin + 12345, 2 * zr::kPieceMin, 5 * M + 12345, 64 * M, zr::kPieceMax};
    const uint64_t lens[] = {0, 1, 255, 256, 300000, zr::kPieceMin - 1, zr::kPieceMin, 5 * M - 1, 9 * M + 77, 40 * M + 3, 130 * M,
                             (1ull << 31) + 64 * M, (5ull << 30) + 1};
    uint64_t calls = 0, turns = 0;
    for (uint64_t q : pieces)
        for (uint64_t n : lens)
            for (uint64_t extra : {(uint64_t)0, q / 4, q / 4 - 1, q + q / 4 - 1})
                for (uint32_t w : {0u, 1u, 32768u})
                    for (uint64_t seed = 1; seed <= 12; ++seed, ++calls) turns += self_call(n + extra, q, w, seed * 0x9e3779b97f4a7c15ull + n + q);
    printf("self ok: %llu calls, %llu turns\n", (unsigned long long)calls, (unsigned long long)turns);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1)
        return !strcmp(argv[1], "layout") ? layout() : !strcmp(argv[1], "retry") ? retry() : !strcmp(argv[1], "chainfull") ? chainfull()
               : !strcmp(argv[1], "segs") ? segs() : !strcmp(argv[1], "finder") ? finder() : !strcmp(argv[1], "pieces") ? pieces()
               : !strcmp(argv[1], "self") ? self() : 2;
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
