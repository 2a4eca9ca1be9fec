// Drives the host inflaters -- zng_rocm_inflate_tokens_decode_window (one thread) and zng_rocm_inflate_tokens_decode_threads
// (eight) of zlib-ng_amd/csrc/inflate_host.cpp + inflate_threads.cpp -- with the decoy streams of tests/decoy_cases.py, which
// tools/sanitize_inflate_decoys.sh writes to files and builds this program for (ASan + UBSan; nothing here needs a device).
// Arguments: the files.  Output, one line per file and thread count:
//   <file> <threads> <status> <out_len> <in_used> <parts> <tokens> <literals>
// The joined token stream is replayed here (literal runs and copies) so that every token and literal is read.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "zng_rocm.h"

static uint64_t replay(const zng_rocm_inflate_tokens &t) {
    std::vector<uint8_t> out;
    out.reserve((size_t)t.out_len);
    size_t lp = 0;
    for (size_t i = 0; i < t.ntokens; ++i) {
        const uint32_t tok = t.tokens[i];
        if (tok >> 31) {
            const size_t len = ((tok >> 16) & 0xffu) + 3u, dist = (tok & 0xffffu) + 1u;
            if (dist > out.size()) return ~0ull;
            for (size_t k = 0; k < len; ++k) out.push_back(out[out.size() - dist]);
        } else {
            if (lp + tok > t.nliterals) return ~0ull;
            out.insert(out.end(), t.literals + lp, t.literals + lp + tok);
            lp += tok;
        }
    }
    uint64_t sum = 0;
    for (uint8_t b : out) sum = sum * 31u + b;
    return out.size() == t.out_len && lp == t.nliterals ? sum : ~0ull;
}

int main(int argc, char **argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        std::ifstream f(argv[a], std::ios::binary);
        const std::vector<uint8_t> src((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        uint64_t sums[2] = {0, 0};
        int k = 0;
        for (int threads : {1, 8}) {
            zng_rocm_inflate_tokens t = {};
            const int st = threads == 1 ? zng_rocm_inflate_tokens_decode_window(src.data(), src.size(), 0, &t)
                                        : zng_rocm_inflate_tokens_decode_threads(src.data(), src.size(), 0, threads, &t);
            sums[k++] = st == 1 ? replay(t) : ~0ull;
            printf("%s %d %d %llu %zu %d %zu %zu\n", argv[a], threads, st, (unsigned long long)t.out_len, t.in_used,
                   threads == 1 ? 0 : zng_rocm_inflate_threads_last_parts(), t.ntokens, t.nliterals);
            zng_rocm_inflate_tokens_free(&t);
        }
        if (sums[0] == ~0ull || sums[0] != sums[1]) {
            printf("%s: the two decodes do not replay to the same bytes\n", argv[a]);
            bad = 1;
        }
    }
    return bad;
}
