// Drives zlib-ng_amd/csrc/deflate_rows_plan.h on the host (tests/test_deflate_rows_plan_cpu.py).  Commands (argv[1], numbers in
// argv[2..]; a JOB is six numbers: in out in_len out_cap dict_len flags, the pointers as integers):
//   consts                                "kSegBytes kSegBytesMin kPrime kHistWords kSubBatches kSubBytes kMaxSub kRowsBatch
//                                          sizeof(SegJob) sizeof(BlkJob)"
//   segbytes IN_LEN CUS                   segment_bytes
//   bound N                               "<rows_deflate_bound> <cs_deflate_bound>"
//   sizes BYTES                           "<seg_bm_words> <seg_d16_entries> <seg_slot_bytes>"
//   plan SEG_BYTES SHARED RULE CAP_ONE JOB...
//                                         "counts" and its eight numbers, "totals" and its four, then one "seg" line per segment
//                                         (in bm_off d16_off seg_start seg_end, then the OR of the fields no kernel reads) and one
//                                         "blk" line per block (the fields of BlkJob in the order of the struct); RULE 0 job, 1 one,
//                                         2 keep
//   one ENTRY LEVEL STRATEGY WBITS NULL_ARGS IN OUT IN_LEN DICT_LEN FLAGS OUT_CAP
//                                         status of a one-stream call (ENTRY 0 block, 1 async)
//   streams LEVEL STRATEGY WBITS NULL_JOBS NULL_OUT_LENS JOB...
//                                         "<status> <first refused job, or the number of jobs>"
//   round COUNT_DICT ROOM FIRST JOB...    rows_round_end, and cs_round_end for the same list when COUNT_DICT is 0
//   sweep                                 the block cut over dict_len mod 1024 = 0..1023 and every in_len around a block border up
//                                         to 3 * kSubBytes + 2: "<cases> <blocks> <blocks without positions in a stream that has some>"
//   self                                  the planner over a mix of job lists against its own invariants (the sanitizer run)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "compress_streams_plan.h"
#include "deflate_rows_plan.h"

namespace {

using namespace zr;

unsigned long long num(const char *s) { return strtoull(s, nullptr, 0); }

std::vector<zng_rocm_stream_job> jobs_from(int argc, char **argv, int at) {
    std::vector<zng_rocm_stream_job> v;
    for (; at + 6 <= argc; at += 6) {
        zng_rocm_stream_job j;
        j.in = (const uint8_t *)(uintptr_t)num(argv[at]);
        j.out = (uint8_t *)(uintptr_t)num(argv[at + 1]);
        j.in_len = (uint32_t)num(argv[at + 2]);
        j.out_cap = (uint32_t)num(argv[at + 3]);
        j.dict_len = (uint32_t)num(argv[at + 4]);
        j.flags = (uint32_t)num(argv[at + 5]);
        v.push_back(j);
    }
    return v;
}

struct Planned {
    RowsCounts           c;
    RowsTotals           t;
    std::vector<SegJob>  seg;
    std::vector<BlkJob>  blk;
};

Planned run_plan(const RowsPlan &p) {
    Planned r;
    r.c = rows_plan_count(p);
    r.seg.resize(r.c.nseg);            // exactly what the counting pass says: the sanitizer sees an overrun
    r.blk.resize(r.c.max_blk);
    r.t = rows_plan_fill(p, r.seg.data(), r.blk.data());
    return r;
}

// the condition under which the block cut once left a block out, over one stream: blocks, and those it would have skipped
void cut_census(uint32_t dict, uint32_t in_len, uint32_t seg_bytes, unsigned long long *blocks, unsigned long long *empty) {
    zng_rocm_stream_job j = rows_one_job((const uint8_t *)(uintptr_t)(1u << 20), (uint8_t *)(uintptr_t)(1u << 30), in_len, dict, 0);
    const RowsPlan p = {&j, 1, seg_bytes, 0, kRowsCapKeep, 0};
    const Planned r = run_plan(p);
    for (size_t i = 0; i < r.t.nb; ++i) {
        ++*blocks;
        if (r.blk[i].blo >= r.blk[i].bhi && in_len != 0) ++*empty;
    }
}

bool self_check() {
    const uint32_t lens[] = {0, 1, 1023, 1024, 1025, 61439, 61440, 61441, 131071, 131072, 131073, 2 * 131072 + 5, 600000};
    const uint32_t dicts[] = {0, 1, 1000, 1024, 32768};
    for (uint32_t seg_bytes : {kSegBytesMin, kSegBytes})
        for (uint32_t shared : {0u, 1u, 32768u})
            for (int rule = 0; rule < 3; ++rule) {
                std::vector<zng_rocm_stream_job> jobs;
                uintptr_t at = 1u << 20;
                for (uint32_t n : lens)
                    for (uint32_t d : dicts) {
                        zng_rocm_stream_job j = rows_one_job((const uint8_t *)at, (uint8_t *)(at + (1ull << 40)), n, shared ? 0 : d,
                                                             (n + d) % 3 == 0 ? ZNG_ROCM_BLOCK_NOT_FINAL : 0);
                        j.out_cap = (uint32_t)rows_deflate_bound(n);
                        jobs.push_back(j);
                        at += n + 64;
                    }
                const RowsPlan p = {jobs.data(), jobs.size(), seg_bytes, shared, (RowsCapRule)rule, 1ull << 33};
                const Planned r = run_plan(p);
                if (r.t.nb > r.c.max_blk || r.t.nb < r.c.nseg) return false;
                size_t k = 0, b = 0, slots = 0;
                for (size_t s = 0; s < jobs.size(); ++s) {
                    const uint32_t dict = shared ? shared : jobs[s].dict_len;
                    uint32_t pos = dict;
                    const size_t b0 = b;
                    for (bool more = true; more; ++k) {
                        const SegJob &g = r.seg[k];
                        if (g.seg_start != pos || g.seg_end < pos || g.seg_end - pos > seg_bytes || (const uint8_t *)((uintptr_t)jobs[s].in - dict) != g.in)
                            return false;
                        uint32_t at_pos = g.seg_start;
                        for (; b < r.t.nb && r.blk[b].hist_idx / kMaxSub == k; ++b) {
                            const BlkJob &q = r.blk[b];
                            if (q.blo != at_pos || q.bhi < q.blo || (q.bhi == q.blo && jobs[s].in_len) || q.first_seg != b0 ||
                                (q.stream & ~kRowsLastBlock) != s || (size_t)q.out != slots || q.out_cap % 4 ||
                                q.bm_off != g.bm_off || q.d16_off != g.d16_off)
                                return false;
                            at_pos = q.bhi;
                            slots += q.out_cap;
                        }
                        if (at_pos != g.seg_end) return false;
                        pos = g.seg_end;
                        more = pos < dict + jobs[s].in_len;
                    }
                    if (!(r.blk[b - 1].stream & kRowsLastBlock) || r.blk[b - 1].is_last != ((jobs[s].flags & ZNG_ROCM_BLOCK_NOT_FINAL) ? 0u : 1u))
                        return false;
                }
                if (k != r.c.nseg || b != r.t.nb || slots != r.t.slot_total) return false;
            }
    unsigned long long blocks = 0, empty = 0;
    for (uint32_t d = 0; d < 1024; d += 37)
        for (uint32_t n = 0; n <= 3 * kSubBytes + 2; n += 1021) cut_census(d, n, kSegBytes, &blocks, &empty);
    return empty == 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "consts") {
        printf("%u %u %u %d %u %u %u %u %zu %zu\n", kSegBytes, kSegBytesMin, kPrime, kHistWords, kSubBatches, kSubBytes, kMaxSub, kRowsBatch,
               sizeof(SegJob), sizeof(BlkJob));
        return 0;
    }
    if (cmd == "segbytes" && argc == 4) {
        printf("%u\n", segment_bytes((size_t)num(argv[2]), atoi(argv[3])));
        return 0;
    }
    if (cmd == "bound" && argc == 3) {
        printf("%llu %llu\n", (unsigned long long)rows_deflate_bound(num(argv[2])), (unsigned long long)cs_deflate_bound(num(argv[2])));
        return 0;
    }
    if (cmd == "sizes" && argc == 3) {
        const uint32_t n = (uint32_t)num(argv[2]);
        printf("%zu %zu %zu\n", seg_bm_words(n), seg_d16_entries(n), seg_slot_bytes(n));
        return 0;
    }
    if (cmd == "plan" && argc >= 6) {
        const std::vector<zng_rocm_stream_job> jobs = jobs_from(argc, argv, 6);
        const RowsPlan p = {jobs.data(), jobs.size(), (uint32_t)num(argv[2]), (uint32_t)num(argv[3]), (RowsCapRule)atoi(argv[4]), num(argv[5])};
        const Planned r = run_plan(p);
        printf("counts %zu %zu %zu %zu %zu %zu %zu %zu\n", r.c.nseg, r.c.max_blk, r.c.seg_tab, r.c.table_bytes, r.c.sizes_bytes, r.c.hist_word,
               r.c.len_hist_bytes, r.c.scan_bytes);
        printf("totals %zu %zu %zu %zu\n", r.t.nb, r.t.slot_total, r.t.bm_total, r.t.d16_total);
        for (const SegJob &g : r.seg)
            printf("seg %llu %llu %llu %u %u %llu\n", (unsigned long long)(uintptr_t)g.in, (unsigned long long)g.bm_off,
                   (unsigned long long)g.d16_off, g.seg_start, g.seg_end,
                   (unsigned long long)((uintptr_t)g.out | (uintptr_t)g.dst | g.dst_cap | g.out_cap | g.is_last | g.first_seg | g.stream));
        for (size_t i = 0; i < r.t.nb; ++i) {
            const BlkJob &q = r.blk[i];
            printf("blk %llu %llu %llu %llu %llu %llu %u %u %u %u %u %u %u %u %u %u\n", (unsigned long long)(uintptr_t)q.in,
                   (unsigned long long)(uintptr_t)q.out, (unsigned long long)(uintptr_t)q.dst, (unsigned long long)q.dst_cap,
                   (unsigned long long)q.bm_off, (unsigned long long)q.d16_off, q.seg_start, q.seg_end, q.blo, q.bhi, q.hist_idx, q.hist_prev,
                   q.out_cap, q.is_last, q.first_seg, q.stream);
        }
        return 0;
    }
    if (cmd == "one" && argc == 13) {
        const RowsRefusal r = rows_one_check((RowsEntry)atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]) != 0,
                                             (const void *)(uintptr_t)num(argv[7]), (const void *)(uintptr_t)num(argv[8]), num(argv[9]),
                                             (uint32_t)num(argv[10]), (uint32_t)num(argv[11]), num(argv[12]));
        printf("%d\n", rows_status(r));
        return 0;
    }
    if (cmd == "streams" && argc >= 7) {
        const std::vector<zng_rocm_stream_job> jobs = jobs_from(argc, argv, 7);
        uint64_t bad = jobs.size();
        const RowsRefusal r = rows_streams_check(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]) ? nullptr : jobs.data(),
                                                 jobs.size(), atoi(argv[6]) != 0, &bad);
        printf("%d %llu\n", rows_status(r), (unsigned long long)bad);
        return 0;
    }
    if (cmd == "round" && argc >= 5) {
        const std::vector<zng_rocm_stream_job> jobs = jobs_from(argc, argv, 5);
        const bool count_dict = atoi(argv[2]) != 0;
        printf("%llu", (unsigned long long)rows_round_end(jobs.data(), jobs.size(), num(argv[4]), num(argv[3]), count_dict));
        if (!count_dict) printf(" %llu", (unsigned long long)cs_round_end(jobs.data(), jobs.size(), num(argv[4]), num(argv[3])));
        printf("\n");
        return 0;
    }
    if (cmd == "sweep") {
        unsigned long long cases = 0, blocks = 0, empty = 0;
        for (uint32_t d = 0; d < 1024; ++d) {
            std::vector<uint32_t> lens = {0, 1, 2, 3 * kSubBytes + 2};
            for (uint32_t k = 1; k <= 3; ++k)
                for (int e = -1; e <= 1; ++e) {
                    lens.push_back(k * kSubBytes + e);              // a border counted from the plaintext
                    lens.push_back(k * kSubBytes - d + e);          // ... and from the batch that holds its first byte
                    lens.push_back(k * kSubBytes - d - kRowsBatch + e);
                }
            for (uint32_t n : lens)
                for (uint32_t seg_bytes : {kSegBytesMin, kSegBytes})
                    for (uint32_t dict : {d, d + 31u * 1024u}) {
                        cut_census(dict, n, seg_bytes, &blocks, &empty);
                        ++cases;
                    }
        }
        printf("%llu %llu %llu\n", cases, blocks, empty);
        return 0;
    }
    if (cmd == "self") {
        if (!self_check()) return 1;
        printf("self ok\n");
        return 0;
    }
    fprintf(stderr, "unknown command\n");
    return 2;
}
