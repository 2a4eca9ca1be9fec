// Drives zlib-ng_amd/csrc/inflate_sizes_plan.h on the host (tests/test_inflate_sizes_plan_cpu.py,
// tools/sanitize_inflate_sizes_plan.sh).  Commands (argv[1], numbers in argv[2..]):
//   call FORMAT HAS_DICT HAVE_JOBS NJOBS HAVE_RESULTS                      the status of is_call_check
//   packed FORMAT HAS_DICT HAVE_JOBS NJOBS HAVE_DST DST_CAP ALIGN HAVE_OFFSETS HAVE_RESULTS   the status of is_packed_call_check
//   job FORMAT HAS_DICT PACKED HAVE_IN IN_LEN DICT_LEN FLAGS               the status of is_job_check
//   jobs FORMAT HAS_DICT PACKED BAD_AT NJOBS                               is_jobs_check over NJOBS jobs, every job from BAD_AT on
//                                                                          with flags set: "<status> <bad job>"
//   add COUNT N                                                            is_count_add: "<saturated 0/1> <count>"
//   sizing FORMAT HDR HMSG IN_LEN OUT_LEN USED STATUS MSG                  is_sizing_row: "<out_len> <used> <status> <msg>"
//   places ALIGN DST_CAP (STATUS SIZE)...                                  per job "<offset> <room> <fits 0/1>", then "<need>"; the
//                                                                          prefix-sum form the scan kernel adds up is held against
//                                                                          the running rule (exit 3 where they differ)
//   final S_OUT S_USED S_STATUS S_MSG FITS D_OUT D_USED D_STATUS D_MSG     is_final_row: "<out_len> <used> <status> <msg>"
//   self                                                                   all of the above over many values, for the sanitizers
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "inflate_sizes_plan.h"

namespace {

uint64_t num(char **argv, int i) { return strtoull(argv[i], nullptr, 0); }

void row(const zr::IsRow &r) { printf("%u %u %d %u\n", r.out_len, r.used, (int)r.status, r.msg); }

// the places of a batch both ways: false where the prefix sums of the padded rooms are not the running rule's offsets
bool places(const std::vector<zr::IsRow> &sizing, uint32_t align, uint64_t dst_cap, bool print) {
    using namespace zr;
    const uint64_t n = sizing.size();
    std::vector<uint64_t> want(n + 1);
    is_places(sizing.data(), n, align, want.data());
    uint64_t sum = 0, need = 0;
    bool same = true;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t room = is_room(sizing[i]);
        same = same && sum == want[i];
        if (i + 1 == n) need = is_need(sum, room);
        if (print)
            printf("%llu %llu %d\n", (unsigned long long)sum, (unsigned long long)room,
                   (int32_t)sizing[i].status == 1 && is_fits(sum, room, dst_cap) ? 1 : 0);
        sum += is_padded(room, align);
    }
    same = same && need == want[n];
    if (print) printf("%llu\n", (unsigned long long)need);
    return same;
}

int self() {
    using namespace zr;
    static uint8_t some[4];
    uint64_t checked = 0;
    for (int format = -1; format <= 3; ++format)
        for (int has_dict = 0; has_dict <= 1; ++has_dict) {
            for (uint64_t njobs : {0ull, 1ull, 5ull, 0x7fffffffull, 0x80000000ull}) {
                checked += is_call_check(format, has_dict != 0, some, njobs, some) == ZNG_ROCM_OK;
                checked += is_call_check(format, has_dict != 0, nullptr, njobs, nullptr) == ZNG_ROCM_OK;
                for (uint32_t align : {0u, 1u, 2u, 3u, 64u, 4096u, 8192u, 0x80000000u})
                    checked += is_packed_call_check(format, has_dict != 0, some, njobs, nullptr, njobs & 1u, align, some, some) == ZNG_ROCM_OK;
            }
            for (int packed = 0; packed <= 1; ++packed)
                for (uint64_t in_len : {0ull, 1ull, 0x7fffffffull, 0x80000000ull, ~0ull})
                    for (uint32_t dict_len : {0u, 1u, 32768u, 32769u, ~0u}) {
                        zng_rocm_inflate_dev_job j;
                        memset(&j, 0, sizeof j);
                        j.in = some;
                        j.in_len = in_len;
                        j.dict_len = dict_len;
                        checked += is_job_check(format, has_dict != 0, j, packed != 0) == ZNG_ROCM_OK;
                        uint64_t bad = 0;
                        checked += is_jobs_check(format, has_dict != 0, &j, 1, packed != 0, &bad) == ZNG_ROCM_OK;
                    }
        }
    for (uint32_t count : {0u, 1u, 258u, kIsCountMax - 258u, kIsCountMax - 1u, kIsCountMax})
        for (uint32_t n : {0u, 1u, 258u, 65535u, kIsCountMax, ~0u}) {
            uint32_t c = count;
            const bool full = is_count_add(&c, n);
            if (c > kIsCountMax || full != ((uint64_t)count + n > kIsCountMax)) return 4;
            ++checked;
        }
    const uint32_t sizes[] = {0u, 1u, 63u, 64u, 65u, 4095u, 4096u, 4097u, 70000u, kIsCountMax};
    for (uint32_t align : {0u, 1u, 2u, 64u, 4096u})
        for (int shape = 0; shape < 8; ++shape) {
            std::vector<IsRow> s;
            for (int i = 0; i < 40; ++i) {
                const uint32_t size = sizes[(i * 7 + shape) % 10];
                const uint32_t status = (i + shape) % 5 == 0 ? kIsDataError : (i + shape) % 7 == 0 ? kIsBufError : 1u;
                s.push_back(IsRow{size, size / 2u, status, status == 1u ? (uint32_t)kMsgNone : (uint32_t)kMsgBlockType});
            }
            if (!places(s, align, 1ull << 33, false)) return 3;
            for (const IsRow &r : s) {
                const IsRow f0 = is_final_row(r, false, IsRow{r.out_len, r.used, 1u, kMsgNone});
                const IsRow f1 = is_final_row(r, true, IsRow{r.out_len, r.used, kIsDataError, kMsgDataCheck});
                checked += f0.status + f1.status;
                for (int format = 0; format <= 2; ++format)
                    for (uint32_t hmsg : {(uint32_t)kMsgNone, (uint32_t)kMsgStarved, (uint32_t)kMsgHeaderCheck, kDictMismatch})
                        checked += is_sizing_row(format, 10u, hmsg, (uint64_t)r.used + 14u, r).status;
            }
        }
    printf("self ok %llu\n", (unsigned long long)checked);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    using namespace zr;
    static uint8_t some[4];
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "call" && argc == 7) {
        printf("%d\n", is_call_check(atoi(argv[2]), num(argv, 3) != 0, num(argv, 4) ? some : nullptr, num(argv, 5),
                                     num(argv, 6) ? some : nullptr));
        return 0;
    }
    if (cmd == "packed" && argc == 11) {
        printf("%d\n", is_packed_call_check(atoi(argv[2]), num(argv, 3) != 0, num(argv, 4) ? some : nullptr, num(argv, 5),
                                            num(argv, 6) ? some : nullptr, num(argv, 7), (uint32_t)num(argv, 8),
                                            num(argv, 9) ? some : nullptr, num(argv, 10) ? some : nullptr));
        return 0;
    }
    if (cmd == "job" && argc == 9) {
        zng_rocm_inflate_dev_job j;
        memset(&j, 0, sizeof j);
        j.in = num(argv, 5) ? some : nullptr;
        j.in_len = num(argv, 6);
        j.dict_len = (uint32_t)num(argv, 7);
        j.flags = (uint32_t)num(argv, 8);
        printf("%d\n", is_job_check(atoi(argv[2]), num(argv, 3) != 0, j, num(argv, 4) != 0));
        return 0;
    }
    if (cmd == "jobs" && argc == 7) {
        const uint64_t bad_at = num(argv, 5), n = num(argv, 6);
        std::vector<zng_rocm_inflate_dev_job> jobs(n ? n : 1);
        memset(jobs.data(), 0, jobs.size() * sizeof jobs[0]);
        for (uint64_t i = 0; i < n; ++i) {
            jobs[i].in = some;
            jobs[i].in_len = 4;
            jobs[i].flags = i >= bad_at ? 1u : 0u;
        }
        uint64_t bad = ~0ull;
        const int rc = is_jobs_check(atoi(argv[2]), num(argv, 3) != 0, jobs.data(), n, num(argv, 4) != 0, &bad);
        printf("%d %lld\n", rc, (long long)bad);
        return 0;
    }
    if (cmd == "add" && argc == 4) {
        uint32_t c = (uint32_t)num(argv, 2);
        const bool full = is_count_add(&c, (uint32_t)num(argv, 3));
        printf("%d %u\n", full ? 1 : 0, c);
        return 0;
    }
    if (cmd == "sizing" && argc == 10) {
        row(is_sizing_row(atoi(argv[2]), (uint32_t)num(argv, 3), (uint32_t)num(argv, 4), num(argv, 5),
                          IsRow{(uint32_t)num(argv, 6), (uint32_t)num(argv, 7), (uint32_t)strtoll(argv[8], nullptr, 0), (uint32_t)num(argv, 9)}));
        return 0;
    }
    if (cmd == "places" && argc >= 4 && argc % 2 == 0) {
        std::vector<IsRow> s;
        for (int i = 4; i + 1 < argc; i += 2)
            s.push_back(IsRow{(uint32_t)num(argv, i + 1), 0u, (uint32_t)strtoll(argv[i], nullptr, 0), 0u});
        return places(s, (uint32_t)num(argv, 2), num(argv, 3), true) ? 0 : 3;
    }
    if (cmd == "final" && argc == 11) {
        const IsRow s = {(uint32_t)num(argv, 2), (uint32_t)num(argv, 3), (uint32_t)strtoll(argv[4], nullptr, 0), (uint32_t)num(argv, 5)};
        const IsRow d = {(uint32_t)num(argv, 7), (uint32_t)num(argv, 8), (uint32_t)strtoll(argv[9], nullptr, 0), (uint32_t)num(argv, 10)};
        row(is_final_row(s, num(argv, 6) != 0, d));
        return 0;
    }
    if (cmd == "self" && argc == 2) return self();
    return 2;
}
