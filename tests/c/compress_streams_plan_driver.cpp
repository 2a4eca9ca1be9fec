// Drives zlib-ng_amd/csrc/compress_streams_plan.h on the host (tests/test_compress_streams_plan_cpu.py).  Commands (argv[1],
// numbers in argv[2..]):
//   header FORMAT LEVEL STRATEGY          "<level 0..9> <FLEVEL> <XFL>", then the hex of the header bytes (an empty line for raw)
//   trailer FORMAT CHECK N                hex of the trailer bytes
//   stored N FLAGS                        "<blocks> <bytes> <marker>", then per block "<length> <hex of its 5 header bytes>"
//   rounds ROUND_BYTES LEN...             "<rounds>", then one line per round "<first job> <jobs>"
//   call FORMAT LEVEL STRATEGY HAVE_JOBS NJOBS HAVE_RESULTS     the status of cs_call_check
//   file HAVE_DST DST_CAP                 the status of cs_file_check
//   job FORMAT PER_JOB_OUT HAVE_IN IN_LEN HAVE_OUT OUT_CAP DICT_LEN FLAGS      the status of cs_job_check
//   jobs FORMAT PER_JOB_OUT OUT_CAP LEN...   cs_jobs_check over jobs of these lengths, all with that out_cap: "<status> <bad job>"
//   bound N FORMAT                        "<deflate bound> <bound>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "compress_streams_plan.h"

namespace {

void hex(const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
    printf("\n");
}

uint64_t num(char **argv, int i) { return strtoull(argv[i], nullptr, 0); }

}  // namespace

int main(int argc, char **argv) {
    using namespace zr;
    static uint8_t some[4];
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "header" && argc == 5) {
        const int format = atoi(argv[2]), level = cs_level(atoi(argv[3])), strategy = atoi(argv[4]);
        if (level == kCsLevelRefused) {
            printf("refused\n");
            return 0;
        }
        uint8_t h[16];
        const uint32_t n = cs_head_bytes(format);
        for (uint32_t k = 0; k < n; ++k) h[k] = cs_header_byte(format, level, strategy, k);
        printf("%d %u %u\n", level, cs_zlib_flevel(level, strategy), cs_gzip_xfl(level, strategy));
        hex(h, n);
        return 0;
    }
    if (cmd == "trailer" && argc == 5) {
        const int format = atoi(argv[2]);
        uint8_t t[16];
        const uint32_t n = cs_tail_bytes(format);
        for (uint32_t k = 0; k < n; ++k) t[k] = cs_trailer_byte(format, k, (uint32_t)num(argv, 3), (uint32_t)num(argv, 4));
        hex(t, n);
        return 0;
    }
    if (cmd == "stored" && argc == 4) {
        const uint64_t n = num(argv, 2);
        const uint32_t flags = (uint32_t)num(argv, 3);
        const uint64_t nb = cs_stored_blocks(n);
        printf("%llu %llu %d\n", (unsigned long long)nb, (unsigned long long)cs_stored_bytes(n, flags), cs_stored_marker(flags) ? 1 : 0);
        for (uint64_t b = 0; b < nb; ++b) {
            const uint32_t len = cs_stored_block_len(n, b);
            uint8_t h[kCsStoredHead];
            for (uint32_t k = 0; k < kCsStoredHead; ++k) h[k] = cs_stored_byte(k, len, b + 1 == nb && !(flags & ZNG_ROCM_BLOCK_NOT_FINAL));
            printf("%u ", len);
            hex(h, sizeof h);
        }
        return 0;
    }
    if (cmd == "rounds" && argc >= 3) {
        std::vector<zng_rocm_stream_job> jobs((size_t)argc - 3);
        for (size_t i = 0; i < jobs.size(); ++i) {
            memset(&jobs[i], 0, sizeof jobs[i]);
            jobs[i].in_len = (uint32_t)num(argv, 3 + (int)i);
        }
        const uint64_t round_bytes = num(argv, 2);
        printf("%llu\n", (unsigned long long)cs_rounds(jobs.data(), jobs.size(), round_bytes));
        for (uint64_t first = 0; first < jobs.size();) {
            const uint64_t last = cs_round_end(jobs.data(), jobs.size(), first, round_bytes);
            printf("%llu %llu\n", (unsigned long long)first, (unsigned long long)(last - first));
            first = last;
        }
        return 0;
    }
    if (cmd == "call" && argc == 8) {
        printf("%d\n", cs_call_check(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), num(argv, 5) ? some : nullptr, num(argv, 6),
                                     num(argv, 7) ? some : nullptr));
        return 0;
    }
    if (cmd == "file" && argc == 4) {
        printf("%d\n", cs_file_check(num(argv, 2) ? some : nullptr, num(argv, 3)));
        return 0;
    }
    if (cmd == "job" && argc == 10) {
        zng_rocm_stream_job j;
        j.in = num(argv, 4) ? some : nullptr;
        j.in_len = (uint32_t)num(argv, 5);
        j.out = num(argv, 6) ? some : nullptr;
        j.out_cap = (uint32_t)num(argv, 7);
        j.dict_len = (uint32_t)num(argv, 8);
        j.flags = (uint32_t)num(argv, 9);
        printf("%d\n", cs_job_check(atoi(argv[2]), j, num(argv, 3) != 0));
        return 0;
    }
    if (cmd == "jobs" && argc >= 5) {
        std::vector<zng_rocm_stream_job> jobs((size_t)argc - 5);
        for (size_t i = 0; i < jobs.size(); ++i) {
            jobs[i].in = jobs[i].out = some;
            jobs[i].in_len = (uint32_t)num(argv, 5 + (int)i);
            jobs[i].out_cap = (uint32_t)num(argv, 4);
            jobs[i].dict_len = jobs[i].flags = 0;
        }
        uint64_t bad = ~0ull;
        const int rc = cs_jobs_check(atoi(argv[2]), jobs.data(), jobs.size(), num(argv, 3) != 0, &bad);
        printf("%d %lld\n", rc, (long long)bad);
        return 0;
    }
    if (cmd == "bound" && argc == 4) {
        const uint64_t n = num(argv, 2);
        printf("%llu %llu\n", (unsigned long long)cs_deflate_bound(n), (unsigned long long)cs_bound(n, atoi(argv[3])));
        return 0;
    }
    if (cmd == "self") {
        // every rule over a sweep of its arguments, each checked against its own invariants: what the sanitizer build runs
        for (int format = 0; format <= 2; ++format)
            for (int level = -1; level <= 9; ++level)
                for (int strategy = 0; strategy <= 4; ++strategy) {
                    uint8_t h[16], t[16];
                    for (uint32_t k = 0; k < cs_head_bytes(format); ++k) h[k] = cs_header_byte(format, cs_level(level), strategy, k);
                    for (uint32_t k = 0; k < cs_tail_bytes(format); ++k) t[k] = cs_trailer_byte(format, k, 0x01020304u, 0xfffffffeu);
                    if (format == 1 && (((unsigned)h[0] << 8 | h[1]) % 31u || t[0] != 1 || t[3] != 4)) return 1;
                    if (format == 2 && (h[0] != 0x1f || h[9] != 3 || t[0] != 4 || t[4] != 0xfe)) return 1;
                }
        const uint64_t sizes[] = {0, 1, 65534, 65535, 65536, 131070, 131071, 0xffffffffull};
        for (uint64_t n : sizes)
            for (uint32_t flags = 0; flags < 4; ++flags) {
                uint64_t sum = 0;
                for (uint64_t b = 0; b < cs_stored_blocks(n); ++b) sum += cs_stored_block_len(n, b) + kCsStoredHead;
                if (sum + (cs_stored_marker(flags) ? 5u : 0u) != cs_stored_bytes(n, flags)) return 1;
                for (int format = 0; format <= 2; ++format)
                    if (cs_stored_bytes(n, flags) + cs_head_bytes(format) + cs_tail_bytes(format) > cs_bound(n, format)) return 1;
            }
        std::vector<zng_rocm_stream_job> jobs(9);
        const uint32_t lens[9] = {0, 1, 0xffffffffu, 7, 0, 0, 262144, 262145, 3};
        for (size_t i = 0; i < jobs.size(); ++i) {
            jobs[i].in = jobs[i].out = some;
            jobs[i].in_len = lens[i];
            jobs[i].out_cap = 0xffffffffu;
            jobs[i].dict_len = jobs[i].flags = 0;
        }
        const uint64_t rbs[] = {0, 1, 8, 262144, 262145, 1ull << 32, ~0ull};
        for (uint64_t rb : rbs) {
            uint64_t rounds = 0, first = 0;
            while (first < jobs.size()) {
                const uint64_t last = cs_round_end(jobs.data(), jobs.size(), first, rb);
                if (last <= first || last > jobs.size()) return 1;
                first = last;
                ++rounds;
            }
            if (rounds != cs_rounds(jobs.data(), jobs.size(), rb)) return 1;
        }
        uint64_t bad = 0;
        if (cs_jobs_check(0, jobs.data(), jobs.size(), true, &bad) != ZNG_ROCM_EINVAL || bad != 2) return 1;
        if (cs_jobs_check(0, jobs.data(), 2, true, &bad) != ZNG_ROCM_OK || cs_jobs_check(0, nullptr, 0, true, nullptr)) return 1;
        printf("self ok\n");
        return 0;
    }
    fprintf(stderr, "unknown command\n");
    return 2;
}
