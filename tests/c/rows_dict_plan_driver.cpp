// Drives the rules of the shared preset dictionary at every level on the host (tests/test_rows_dict_plan_cpu.py): dict_plan.h
// (the primed positions of the rows engine), framing_parse.h (the zlib header with FDICT) and compress_streams_plan.h (the cs_dict_*
// checks and the bound).  Commands (argv[1], numbers in argv[2..]):
//   primed W...                            dict_rows_primed of every W, one per line; then "<batch> <table bytes>"
//   header LEVEL STRATEGY DICTID           "<head bytes of format 0> <of format 1> <of format 2>", then the hex of the 6 header bytes
//   bound N FORMAT                         cs_dict_bound
//   call FORMAT LEVEL STRATEGY HAVE_DICT HAVE_JOBS NJOBS HAVE_RESULTS     the status of cs_dict_call_check
//   job FORMAT PER_JOB_OUT HAVE_IN IN_LEN HAVE_OUT OUT_CAP DICT_LEN FLAGS   the status of cs_dict_job_check
//   jobs FORMAT PER_JOB_OUT OUT_CAP LEN...   cs_dict_jobs_check over jobs of these lengths, all with that out_cap: "<status> <bad job>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "compress_streams_plan.h"
#include "dict_plan.h"

namespace {

uint64_t num(char **argv, int i) { return strtoull(argv[i], nullptr, 0); }

}  // namespace

int main(int argc, char **argv) {
    using namespace zr;
    static uint8_t some[4];
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "primed") {
        for (int i = 2; i < argc; ++i) printf("%u\n", dict_rows_primed((uint32_t)num(argv, i)));
        printf("%u %u\n", kDictRowBatch, kDictRowsBytes);
        return 0;
    }
    if (cmd == "header" && argc == 5) {
        const int level = cs_level(atoi(argv[2])), strategy = atoi(argv[3]);
        if (level == kCsLevelRefused) {
            printf("refused\n");
            return 0;
        }
        printf("%u %u %u\n", cs_dict_head_bytes(0), cs_dict_head_bytes(1), cs_dict_head_bytes(2));
        for (uint32_t k = 0; k < cs_dict_head_bytes(1); ++k) printf("%02x", cs_dict_header_byte(level, strategy, (uint32_t)num(argv, 4), k));
        printf("\n");
        return 0;
    }
    if (cmd == "bound" && argc == 4) {
        printf("%llu\n", (unsigned long long)cs_dict_bound(num(argv, 2), atoi(argv[3])));
        return 0;
    }
    if (cmd == "call" && argc == 9) {
        printf("%d\n", cs_dict_call_check(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), num(argv, 5) ? some : nullptr,
                                          num(argv, 6) ? some : nullptr, num(argv, 7), num(argv, 8) ? some : nullptr));
        return 0;
    }
    if (cmd == "job" && argc == 10) {
        zng_rocm_stream_job j;
        memset(&j, 0, sizeof j);
        j.in = num(argv, 4) ? some : nullptr;
        j.in_len = (uint32_t)num(argv, 5);
        j.out = num(argv, 6) ? some : nullptr;
        j.out_cap = (uint32_t)num(argv, 7);
        j.dict_len = (uint32_t)num(argv, 8);
        j.flags = (uint32_t)num(argv, 9);
        printf("%d\n", cs_dict_job_check(atoi(argv[2]), j, num(argv, 3) != 0));
        return 0;
    }
    if (cmd == "jobs" && argc >= 5) {
        std::vector<zng_rocm_stream_job> jobs;
        for (int i = 5; i < argc; ++i) {
            zng_rocm_stream_job j;
            memset(&j, 0, sizeof j);
            j.in = some;
            j.in_len = (uint32_t)num(argv, i);
            j.out = some;
            j.out_cap = (uint32_t)num(argv, 4);
            jobs.push_back(j);
        }
        uint64_t bad = ~0ull;
        const int rc = cs_dict_jobs_check(atoi(argv[2]), jobs.data(), jobs.size(), num(argv, 3) != 0, &bad);
        printf("%d %lld\n", rc, rc ? (long long)bad : -1ll);
        return 0;
    }
    return 2;
}
