// Stand-alone driver of zlib-ng_amd/csrc/gzip_header_plan.h (the gzip header fields of the device members: render, lengths,
// refusals, the field walk, the gather layout) for tests/test_gzip_header_plan_cpu.py and tools/sanitize_gzip_header_plan.sh.
// No GPU, no library: the plan header alone.
//   run FILE   one command per line of FILE, one answer line each:
//     R level strategy time os text hcrc reserved extra_len EXTRA NAME COMMENT
//                     a header; EXTRA / NAME / COMMENT are "-" (a null pointer) or "=" followed by the bytes in hex (NAME and
//                     COMMENT without their terminator); extra_len is given on its own so that it can disagree with EXTRA
//                     -> "refused", or "<gh_bytes> <hex of the rendered header>"
//     N level strategy   the null header -> as R
//     P HEX           gh_parse_host over the bytes -> status msg header_len flg time xflags os extra_len name_len comment_len
//                     extra_off name_off comment_off
//     G k  then k lines "status extra_len has_name name_len has_comment comment_len"   -> "need off0 off1 ..."
//   self       render, walk every truncation of every rendered header against wrapper_parse_rules, lay out a table
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "gzip_header_plan.h"

using namespace zr;

static std::vector<uint8_t> unhex(const std::string &s) {
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return out;
}

static void print_hex(const std::vector<uint8_t> &b) {
    static const char digit[] = "0123456789abcdef";
    std::string s(2 * b.size(), '0');
    for (size_t i = 0; i < b.size(); ++i) {
        s[2 * i] = digit[b[i] >> 4];
        s[2 * i + 1] = digit[b[i] & 15];
    }
    fputs(s.c_str(), stdout);
}

// "refused" or the rendered header; the length must be what gh_bytes said before a byte was written
static bool render(const zng_rocm_gzip_header *h, int level, int strategy, std::vector<uint8_t> *out) {
    GhLens lens;
    if (gh_check(h, &lens)) return false;
    const uint32_t n = gh_bytes(h, lens);
    out->assign((size_t)n + 8, 0xa5);                    // guard bytes behind the header
    gh_render(h, lens, level, strategy, out->data());
    for (size_t k = n; k < out->size(); ++k)
        if ((*out)[k] != 0xa5) {
            fprintf(stderr, "gh_render wrote behind gh_bytes\n");
            exit(2);
        }
    out->resize(n);
    return n <= kGhMaxBytes;
}

static void print_row(const GhRow &r) {
    printf("%d %u %llu %u %u %u %u %u %u %u %llu %llu %llu\n", r.status, r.msg, (unsigned long long)r.header_len, r.flg, r.time, r.xflags,
           r.os, r.extra_len, r.name_len, r.comment_len, (unsigned long long)r.extra_off, (unsigned long long)r.name_off,
           (unsigned long long)r.comment_off);
}

static int run(const char *path) {
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "R" || cmd == "N") {
            int level, strategy;
            in >> level >> strategy;
            zng_rocm_gzip_header h;
            memset(&h, 0, sizeof h);
            std::vector<uint8_t> extra, name, comment, out;
            if (cmd == "R") {
                std::string e, n, c;
                in >> h.time >> h.os >> h.text >> h.hcrc >> h.reserved >> h.extra_len >> e >> n >> c;
                extra = unhex(e.substr(1));
                name = unhex(n.substr(1));
                comment = unhex(c.substr(1));
                extra.push_back(0);                      // (so that data() is a pointer for an empty field)
                name.push_back(0);
                comment.push_back(0);
                if (e[0] == '=') h.extra = extra.data();
                if (n[0] == '=') h.name = (const char *)name.data();
                if (c[0] == '=') h.comment = (const char *)comment.data();
            }
            if (!render(cmd == "R" ? &h : nullptr, level, strategy, &out)) {
                puts("refused");
                continue;
            }
            printf("%zu ", out.size());
            print_hex(out);
            putchar('\n');
        } else if (cmd == "P") {
            std::string hex;
            in >> hex;
            const std::vector<uint8_t> b = unhex(hex);
            std::vector<uint8_t> exact(b);               // a heap block of exactly these bytes: a read behind them is seen
            print_row(gh_parse_host(exact.data(), exact.size()));
        } else if (cmd == "G") {
            size_t k = 0;
            in >> k;
            std::vector<GhRow> rows(k, gh_row_refused(0, kWrapNone));
            for (size_t i = 0; i < k && std::getline(f, line); ++i) {
                std::istringstream row(line);
                int has_name, has_comment;
                row >> rows[i].status >> rows[i].extra_len >> has_name >> rows[i].name_len >> has_comment >> rows[i].comment_len;
                rows[i].name_off = has_name ? 1 : 0;
                rows[i].comment_off = has_comment ? 1 : 0;
            }
            printf("%llu", (unsigned long long)gh_gather_layout(rows.data(), k));
            for (size_t i = 0; i < k; ++i) printf(" %llu", (unsigned long long)rows[i].text_off);
            putchar('\n');
        } else if (!cmd.empty()) {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}

#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "self: %s (line %d)\n", #cond, __LINE__);  \
            return 1;                                                  \
        }                                                              \
    } while (0)

// every cut of a rendered header: status, message and header_len are the rules' own, the fields those that were set
static int self_walk(const std::vector<uint8_t> &head, const zng_rocm_gzip_header &h, const GhLens &lens) {
    for (size_t cut = 0; cut <= head.size(); ++cut) {
        std::vector<uint8_t> exact(head.begin(), head.begin() + (long)cut);
        const GhRow r = gh_parse_host(exact.data(), cut);
        const WrapperHead w = wrapper_parse_rules(2, HostBytes{exact.data()}, cut);
        EXPECT(r.status == w.status && r.msg == w.msg && r.header_len == (w.status == 0 ? w.header_len : 0u));
        EXPECT((r.status == 0) == (cut == head.size()));
    }
    const GhRow r = gh_parse_host(head.data(), head.size());
    EXPECT(r.flg == gh_flg(&h) && r.time == h.time && r.os == (h.os & 0xffu));
    EXPECT(r.extra_len == lens.extra && r.name_len == lens.name && r.comment_len == lens.comment);
    EXPECT((r.extra_off != 0) == (h.extra != nullptr) && (r.name_off != 0) == (h.name != nullptr) && (r.comment_off != 0) == (h.comment != nullptr));
    if (h.extra) EXPECT(!memcmp(head.data() + r.extra_off, h.extra, lens.extra));
    if (h.name) EXPECT(!memcmp(head.data() + r.name_off, h.name, (size_t)lens.name + 1));
    if (h.comment) EXPECT(!memcmp(head.data() + r.comment_off, h.comment, (size_t)lens.comment + 1));
    if (h.hcrc) {                                        // a flipped FHCRC byte
        std::vector<uint8_t> bad(head);
        bad[bad.size() - 1] ^= 0x40;
        const GhRow b = gh_parse_host(bad.data(), bad.size());
        EXPECT(b.status == -3 && b.msg == kWrapHeaderCrc && b.header_len == 0 && gh_gather_len(b) == 0);
    }
    return 0;
}

static int self() {
    const std::string big(kGhFieldMax, 'n');
    const std::vector<uint8_t> extra(kGhFieldMax, 0xee);
    const uint8_t sub[6] = {66, 67, 2, 0, 0x34, 0x12};
    std::vector<GhRow> table;
    for (uint32_t flg = 0; flg < 32; ++flg)
        for (int size = 0; size < 3; ++size) {
            zng_rocm_gzip_header h;
            memset(&h, 0, sizeof h);
            h.time = 0x01020304u * (flg + 1u);
            h.os = flg == 5 ? 0x1ffu : flg;
            h.text = flg & 1u;
            h.hcrc = flg & 2u;
            if (flg & 4u) {
                h.extra = size == 2 ? extra.data() : sub;
                h.extra_len = size == 0 ? 0u : size == 1 ? 6u : kGhFieldMax;
            }
            if (flg & 8u) h.name = size == 0 ? "" : size == 1 ? "a.txt" : big.c_str();
            if (flg & 16u) h.comment = size == 0 ? "" : size == 1 ? "c" : big.c_str();
            GhLens lens;
            std::vector<uint8_t> head;
            EXPECT(gh_check(&h, &lens) == 0 && render(&h, flg % 10, flg & 2 ? 2 : 0, &head));
            EXPECT(head.size() == gh_bytes(&h, lens));
            if (size < 2 && self_walk(head, h, lens)) return 1;
            if (size == 2 && flg == 31) EXPECT(head.size() == kGhMaxBytes);
            table.push_back(gh_parse_host(head.data(), head.size()));
            EXPECT(table.back().status == 0);
            zng_rocm_gzip_header bad = h;                // the refusals
            bad.reserved = 1;
            EXPECT(gh_check(&bad, nullptr) == ZNG_ROCM_EINVAL);
            bad = h;
            bad.extra_len = kGhFieldMax + 1u;
            EXPECT(gh_check(&bad, nullptr) == ZNG_ROCM_EINVAL);
        }
    const std::string over(kGhFieldMax + 1u, 'x');
    zng_rocm_gzip_header h;
    memset(&h, 0, sizeof h);
    h.name = over.c_str();
    EXPECT(gh_check(&h, nullptr) == ZNG_ROCM_EINVAL);
    h.name = nullptr;
    h.comment = over.c_str();
    EXPECT(gh_check(&h, nullptr) == ZNG_ROCM_EINVAL);
    h.comment = nullptr;
    h.extra_len = 1;
    EXPECT(gh_check(&h, nullptr) == ZNG_ROCM_EINVAL);
    GhLens none;
    EXPECT(gh_check(nullptr, &none) == 0 && gh_bytes(nullptr, none) == 10u);
    // the layout: refused and cut members put nothing into the text and move nobody
    table[3] = gh_row_refused(-3, kWrapFlags);
    table[4] = gh_row_refused(-5, kWrapNone);
    uint64_t want = 0;
    const uint64_t need = gh_gather_layout(table.data(), table.size());
    for (size_t i = 0; i < table.size(); ++i) {
        EXPECT(table[i].text_off == want);
        want += gh_gather_len(table[i]);
        if (i == 3 || i == 4) EXPECT(gh_gather_len(table[i]) == 0);
    }
    EXPECT(need == want && need > 0);
    puts("self ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "run")) return run(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "self")) return self();
    fprintf(stderr, "usage: %s run FILE | self\n", argv[0]);
    return 2;
}
