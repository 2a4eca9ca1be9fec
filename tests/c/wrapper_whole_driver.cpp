// Drives wrapper_parse_whole and wrapper_trailer_verdict (zlib-ng_amd/csrc/framing_parse.h) on the host, for
// tests/test_wrapper_whole_cpu.py and tools/sanitize_wrapper_whole.sh (plain host C++, no HIP).  Commands (argv[1]):
//   parse <file>     one case per line, "<format> <hex bytes or ->": prints "<header_len> <msg> <wrap msg> <fdict> <dictid>",
//                    once through HostBytes (memchr) and once through LaneBytes (the byte walk of the kernels); the two must agree
//   trailer <file>   one case per line, "<format> <hex trailer> <adler> <crc> <out_len>": prints the verdict
//   self             every prefix and every mutation of the first four bytes of built-in members, for the sanitizer run
// Every member is parsed in a heap block of exactly its length, so a read behind the bytes that exist is an error under ASan.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "framing_parse.h"

using namespace zr;

static uint32_t g_tab[256];

static void make_table() {
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
        g_tab[i] = c;
    }
}

static const char *msg_name(uint32_t msg) {
    switch (msg) {
    case kMsgNone: return "none";
    case kMsgStarved: return "starved";
    case kMsgHeaderCheck: return "header";
    case kMsgMethod: return "method";
    case kMsgWindow: return "window";
    case kMsgHeaderCrc: return "hcrc";
    case kMsgNeedDict: return "needdict";
    case kMsgDataCheck: return "data";
    case kMsgLengthCheck: return "length";
    default: return "other";
    }
}

static const char *wrap_name(uint32_t msg) {
    static const char *const names[kWrapMsgCount] = {"none", "header", "method", "window", "flags", "hcrc", "data", "length"};
    return msg < kWrapMsgCount ? names[msg] : "other";
}

static std::vector<uint8_t> unhex(const std::string &hex) {
    std::vector<uint8_t> out;
    if (hex == "-") return out;
    for (size_t i = 0; i + 1 < hex.size(); i += 2) out.push_back((uint8_t)strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

static bool same(const WholeHead &a, const WholeHead &b) {
    return a.header_len == b.header_len && a.msg == b.msg && a.wrap_msg == b.wrap_msg && a.fdict == b.fdict && a.dictid == b.dictid;
}

// both ways of reaching the bytes, in a block of exactly n bytes
static bool parse_exact(int format, const uint8_t *bytes, size_t n, WholeHead *out) {
    uint8_t *block = (uint8_t *)malloc(n ? n : 1);
    if (!block) return false;
    if (n) memcpy(block, bytes, n);
    const WholeHead a = wrapper_parse_whole(format, HostBytes{block}, n, g_tab);
    const WholeHead b = wrapper_parse_whole(format, LaneBytes{block}, n, g_tab);
    free(block);
    *out = a;
    return same(a, b);
}

static int self_test() {
    std::vector<std::vector<uint8_t>> members;
    for (int fdict = 0; fdict < 2; ++fdict)
        for (uint32_t flevel = 0; flevel < 4; ++flevel) {
            uint32_t header = (0x78u << 8) | (flevel << 6) | (fdict ? 0x20u : 0u);
            header += 31u - header % 31u;
            std::vector<uint8_t> m = {(uint8_t)(header >> 8), (uint8_t)header};
            if (fdict) m.insert(m.end(), {0x11, 0x22, 0x33, 0x44});
            m.insert(m.end(), {0x03, 0x00, 0x00, 0x00, 0x00, 0x01});
            members.push_back(m);
        }
    const size_t nzlib = members.size();
    std::vector<uint8_t> g = {0x1f, 0x8b, 8, 4 | 8 | 16 | 2, 1, 2, 3, 4, 0, 3, 5, 0, 'e', 'x', 't', 'r', 'a'};
    for (const char *s : {"file name.txt", "a comment"}) g.insert(g.end(), (const uint8_t *)s, (const uint8_t *)s + strlen(s) + 1);
    uint32_t c = 0xffffffffu;
    for (uint8_t b : g) c = g_tab[(c ^ b) & 0xffu] ^ (c >> 8);
    g.push_back((uint8_t)~c);
    g.push_back((uint8_t)(~c >> 8));
    const size_t ghead = g.size();
    g.insert(g.end(), {0x03, 0x00, 0, 0, 0, 0, 0, 0, 0, 0});
    members.push_back(g);
    members.push_back({0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3, 0x03, 0x00, 0, 0, 0, 0, 0, 0, 0, 0});
    WholeHead h;
    for (size_t m = 0; m < members.size(); ++m) {
        const int format = m < nzlib ? 1 : 2;
        const std::vector<uint8_t> &full = members[m];
        if (!parse_exact(format, full.data(), full.size(), &h)) return 1;
        const bool fdict = format == 1 && (full[1] & 0x20u);
        if (h.msg != (fdict ? (uint32_t)kMsgNeedDict : (uint32_t)kMsgNone)) return 2;
        if (format == 2 && h.header_len != (m + 1 == members.size() ? 10u : ghead)) return 3;
        if (fdict && (h.dictid != 0x11223344u || h.fdict != 1u)) return 4;
        for (size_t n = 0; n <= full.size(); ++n)
            if (!parse_exact(format, full.data(), n, &h)) return 5;
        for (size_t at = 0; at < 4; ++at)
            for (uint32_t v = 0; v < 256; ++v) {
                if (v == full[at]) continue;
                std::vector<uint8_t> mut = full;
                mut[at] = (uint8_t)v;
                if (!parse_exact(format, mut.data(), mut.size(), &h)) return 6;
                for (size_t n = 2; n <= 9 && n <= mut.size(); ++n)
                    if (!parse_exact(format, mut.data(), n, &h)) return 7;
            }
    }
    g[ghead - 1] ^= 0x01u;                                // the stored FHCRC off by one bit
    if (!parse_exact(2, g.data(), g.size(), &h) || h.msg != kMsgHeaderCrc || h.wrap_msg != kWrapHeaderCrc) return 8;
    // the trailer: the compare order and the low 32 bits of the length
    const uint8_t zt[4] = {0x01, 0x02, 0x03, 0x04}, gt[8] = {0x04, 0x03, 0x02, 0x01, 0x05, 0, 0, 0};
    if (wrapper_trailer_verdict(1, zt, 0x01020304u, 0, 7) != kWrapNone || wrapper_trailer_verdict(1, zt, 0x01020305u, 0, 7) != kWrapDataCheck) return 9;
    if (wrapper_trailer_verdict(2, gt, 0, 0x01020304u, (1ull << 32) + 5) != kWrapNone) return 10;
    if (wrapper_trailer_verdict(2, gt, 0, 0x01020304u, 6) != kWrapLengthCheck || wrapper_trailer_verdict(2, gt, 0, 1u, 6) != kWrapDataCheck) return 11;
    if (wrapper_trailer_verdict(0, gt, 0, 0, 0) != kWrapNone) return 12;
    for (int format = 1; format <= 2; ++format)           // what the writer writes, the reader accepts
        for (int level = 0; level <= 9; ++level) {
            uint8_t w[10];
            for (uint32_t k = 0; k < wrapper_head_bytes(format); ++k) w[k] = wrapper_header_byte(format, level, 0, k);
            if (!parse_exact(format, w, wrapper_head_bytes(format), &h) || h.msg != kMsgNone || h.header_len != wrapper_head_bytes(format)) return 13;
            uint8_t t[8];
            for (uint32_t k = 0; k < wrapper_tail_bytes(format); ++k) t[k] = wrapper_trailer_byte(format, k, 0xa1b2c3d4u, 0x00010203u);
            if (wrapper_trailer_verdict(format, t, 0xa1b2c3d4u, 0xa1b2c3d4u, 0x00010203u) != kWrapNone) return 14;
        }
    printf("self ok\n");
    return 0;
}

int main(int argc, char **argv) {
    make_table();
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "self") return self_test();
    if (argc < 3) return 2;
    std::ifstream in(argv[2]);
    if (!in) return 3;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream f(line);
        int format = 0;
        std::string hex;
        f >> format >> hex;
        const std::vector<uint8_t> bytes = unhex(hex);
        if (cmd == "parse") {
            WholeHead h;
            if (!parse_exact(format, bytes.data(), bytes.size(), &h)) return 4;
            printf("%llu %s %s %u %u\n", (unsigned long long)h.header_len, msg_name(h.msg), wrap_name(h.wrap_msg), h.fdict, h.dictid);
        } else if (cmd == "trailer") {
            unsigned long long adler = 0, crc = 0, out_len = 0;
            f >> adler >> crc >> out_len;
            const uint32_t v = wrapper_trailer_verdict(format, bytes.data(), (uint32_t)adler, (uint32_t)crc, out_len);
            printf("%s %s\n", wrap_name(v), msg_name(wrapper_inflate_msg(v)));
        } else {
            return 2;
        }
    }
    return 0;
}
