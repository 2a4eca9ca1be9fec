// dict_plan_driver.cpp -- the rules of zlib-ng_amd/csrc/dict_plan.h on the command line, for tests/test_dict_plan_cpu.py
// (plain host C++, no HIP):
//   header <dictid>            the 16 bytes of the wrapper's head and the 4 of a trailer with Adler-32 <dictid>, hex
//   parse <hex bytes> <dictid> what a reader holding dictionary <dictid> makes of the first bytes of a zlib member:
//                              <bytes consumed> <verdict> <history>
//   table <file>               the file as a dictionary: "<W> <first byte of the window> <entered positions>", then the
//                              head table, one line
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dict_plan.h"

using namespace zr;

static const char *verdict(uint32_t msg) {
    switch (msg) {
    case kMsgNone: return "none";
    case kMsgStarved: return "starved";
    case kMsgHeaderCheck: return "header";
    case kMsgMethod: return "method";
    case kMsgWindow: return "window";
    case kDictMismatch: return "mismatch";
    default: return "other";
    }
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string cmd = argv[1];
    if (cmd == "header") {
        const uint32_t id = (uint32_t)strtoul(argv[2], nullptr, 0);
        uint8_t h[kDictWrapHead];
        dict_put_header(h, id);
        for (uint32_t k = 0; k < kDictWrapHead; ++k) printf("%02x", h[k]);
        printf("\n");
        for (uint32_t k = 0; k < 4; ++k) printf("%02x", dict_trailer_byte(k, id));
        printf("\n");
        return 0;
    }
    if (cmd == "parse" && argc >= 4) {
        std::vector<uint8_t> in;
        const char *hex = argv[2];
        for (size_t i = 0; hex[i] && hex[i + 1] && hex[0] != '-'; i += 2) {
            const char b[3] = {hex[i], hex[i + 1], 0};
            in.push_back((uint8_t)strtoul(b, nullptr, 16));
        }
        in.push_back(0);                                  // never read: the rule stays inside n
        const DictHeader h = dict_parse_header(in.data(), in.size() - 1, (uint32_t)strtoul(argv[3], nullptr, 0));
        printf("%u %s %u\n", h.pos, verdict(h.msg), h.history);
        return 0;
    }
    if (cmd == "table") {
        FILE *f = fopen(argv[2], "rb");
        if (!f) return 3;
        std::vector<uint8_t> d;
        uint8_t buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + n);
        fclose(f);
        const uint32_t W = dict_window(d.size());
        printf("%u %llu %u\n", W, (unsigned long long)dict_window_start(d.size()), dict_positions(W));
        std::vector<uint32_t> head(kDictHeadSlots);
        dict_head_table(d.data() + dict_window_start(d.size()), W, head.data());
        for (uint32_t h = 0; h < kDictHeadSlots; ++h) printf("%u ", head[h]);
        printf("\n");
        return 0;
    }
    return 2;
}
