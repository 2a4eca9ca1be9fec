// Drives zlib-ng_amd/csrc/deflate_window_plan.h on the host (tests/test_window_plan_cpu.py).  Commands (argv[1], numbers in
// argv[2..]):
//   verdict FORMAT WINDOW_BITS            "<status of win_check> <effective window, 0 = refused>"
//   table                                 one line per window 9..15: "<w> <size> <cap> <prime> <window form 0/1>"
//   prime SEG_START W                     the first position a segment at SEG_START enters into the rows
//   header FORMAT LEVEL STRATEGY WINDOW_BITS   hex of the header bytes at the effective window ("refused" if there is none)
//   self                                  every rule over a sweep of its arguments against its own invariants (the sanitizer run)
#include <cstdio>
#include <cstdlib>
#include <string>

#include "deflate_window_plan.h"

namespace {

void hex(const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
    printf("\n");
}

}  // namespace

int main(int argc, char **argv) {
    using namespace zr;
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "verdict" && argc == 4) {
        printf("%d %d\n", win_check(atoi(argv[2]), atoi(argv[3])), win_effective(atoi(argv[2]), atoi(argv[3])));
        return 0;
    }
    if (cmd == "table") {
        for (int w = kWinBitsMin; w <= kWinBitsMax; ++w)
            printf("%d %u %u %u %d\n", w, win_size(w), win_dist(w), win_prime(w), win_form(w) ? 1 : 0);
        return 0;
    }
    if (cmd == "prime" && argc == 4) {
        printf("%u\n", win_prime_start((uint32_t)strtoul(argv[2], nullptr, 0), atoi(argv[3])));
        return 0;
    }
    if (cmd == "header" && argc == 6) {
        const int format = atoi(argv[2]), level = atoi(argv[3]), strategy = atoi(argv[4]);
        const int w = win_effective(format, atoi(argv[5]));
        if (!w) {
            printf("refused\n");
            return 0;
        }
        uint8_t h[16];
        const uint32_t n = wrapper_head_bytes(format);
        for (uint32_t k = 0; k < n; ++k) h[k] = win_header_byte(format, level, strategy, w, k);
        hex(h, n);
        return 0;
    }
    if (cmd == "self") {
        for (int format = -1; format <= 3; ++format)
            for (int wb = -16; wb <= 32; ++wb) {
                const int w = win_effective(format, wb);
                if ((w == 0) != (win_check(format, wb) == ZNG_ROCM_EINVAL)) return 1;
                if (w && (w < kWinBitsMin || w > kWinBitsMax)) return 1;
                if (w && w != wb && !(wb == 8 && format == 1 && w == 9)) return 1;
            }
        for (int w = kWinBitsMin; w <= kWinBitsMax; ++w) {
            if (win_dist(w) + kWinMinLookahead != win_size(w) || win_prime(w) > kWinPrimeMax || win_prime(w) < win_dist(w)) return 1;
            const uint32_t starts[] = {0u, 1u, 250u, 1023u, 1024u, 32768u, 131072u, 131073u, 0xfff00000u};
            for (uint32_t s : starts) {
                const uint32_t p0 = win_prime_start(s, w);
                // a batch border, at or in front of every source within the cap, never more than the prime and a batch back
                if (p0 % kWinBatch || p0 > s || (s >= win_dist(w) && p0 > s - win_dist(w)) || s - p0 >= win_prime(w) + kWinBatch) return 1;
            }
            for (int level = 0; level <= 9; ++level)
                for (int strategy = 0; strategy <= 4; ++strategy) {
                    const unsigned cmf = win_header_byte(1, level, strategy, w, 0), flg = win_header_byte(1, level, strategy, w, 1);
                    if (cmf != 8u + ((unsigned)(w - 8) << 4) || ((cmf << 8) | flg) % 31u || (flg & 0x20u) ||
                        (flg >> 6) != wrapper_zlib_flevel(level, strategy))
                        return 1;
                    if (w == kWinBitsMax && (cmf != wrapper_header_byte(1, level, strategy, 0) || flg != wrapper_header_byte(1, level, strategy, 1)))
                        return 1;
                    for (uint32_t k = 0; k < 10; ++k)                  // gzip has no window field
                        if (win_header_byte(2, level, strategy, w, k) != wrapper_header_byte(2, level, strategy, k)) return 1;
                }
        }
        printf("self ok\n");
        return 0;
    }
    fprintf(stderr, "unknown command\n");
    return 2;
}
