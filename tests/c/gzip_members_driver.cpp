// Drives zlib-ng_amd/csrc/gzip_members_plan.h and the BSIZE walk of framing_parse.h on the host
// (tests/test_gzip_members_cpu.py).  Commands (argv[1]):
//   scan FILE     the candidates of the file's bytes, one line of positions (scan_candidates)
//   bsize FILE    "<status> <header_len> <bsize or -1>": wrapper_parse_rules(2) and gzip_bgzf_bsize on the file's bytes
//   table FILE    the candidate table of the file as the link kernel builds it (the kernel's steps restated with the shared
//                 rules: header verdict, BSIZE, member_next, the eight bytes in front of the guessed end), one row per line:
//                 pos header_len next status msg flags crc isize
//                 a candidate's header is shown member_header_look bytes, as the scatter kernel cuts its job
//   cost FILE     "<candidates> <bytes examined>": the table built as above with every byte the header rules and the BSIZE walk
//                 look at counted (a zero search counts the bytes up to and with the zero, or all of them), plus the bytes an
//                 FHCRC pass covers
//   plan          stdin: n src_len start dst_off dst_cap, n rows as above, then nres and nres x "status out_len in_used".
//                 Output: one line per planned member "cand engine src_off span dst_off out_guess crc bgzf to_end", then
//                 "alone <cand> guess|must" (guess: the plan could tell the guess was wrong) or "end", then "dst_end <bytes>", then "unverified <index>" when nres == the members planned
//   after         stdin: at src_len b0 b1 -> "done" or "member" (after_member)
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "framing_parse.h"
#include "gzip_members_plan.h"

namespace {

struct HostBytes {
    const uint8_t *src;
    uint32_t byte(uint64_t pos) const { return src[pos]; }
    uint64_t find_zero(uint64_t from, uint64_t n) const {
        const void *z = from < n ? memchr(src + from, 0, (size_t)(n - from)) : nullptr;
        return z ? (uint64_t)((const uint8_t *)z - src) : n;
    }
};

struct CountedBytes {                                    // HostBytes that counts what is looked at
    const uint8_t *src;
    uint64_t *examined;
    uint32_t byte(uint64_t pos) const {
        ++*examined;
        return src[pos];
    }
    uint64_t find_zero(uint64_t from, uint64_t n) const {
        const uint64_t z = HostBytes{src}.find_zero(from, n);
        *examined += (z < n ? z + 1 : n) - (from < n ? from : n);
        return z;
    }
};

bool slurp(const char *path, std::vector<uint8_t> &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return true;
}

void print_row(const zr::CandRow &r) {
    printf("%llu %llu %u %d %u %u %u %u\n", (unsigned long long)r.pos, (unsigned long long)r.header_len, r.next, r.status, r.msg, r.flags,
           r.crc, r.isize);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "scan" || cmd == "bsize" || cmd == "table" || cmd == "cost") {
        std::vector<uint8_t> data;
        if (argc < 3 || !slurp(argv[2], data)) return 2;
        const uint8_t *src = data.data();
        const uint64_t n = data.size();
        if (cmd == "bsize") {
            const zr::WrapperHead h = zr::wrapper_parse_rules(2, HostBytes{src}, n);
            uint32_t bsize = 0;
            const bool has = h.status == 0 && zr::gzip_bgzf_bsize(HostBytes{src}, n, &bsize);
            printf("%d %llu %ld\n", h.status, (unsigned long long)h.header_len, has ? (long)bsize : -1l);
            return 0;
        }
        std::vector<uint64_t> pos;
        zr::scan_candidates(src, n, pos);
        if (cmd == "scan") {
            for (uint64_t p : pos) printf("%llu ", (unsigned long long)p);
            printf("\n");
            return 0;
        }
        const uint32_t nc = (uint32_t)pos.size();
        if (cmd == "cost") {
            uint64_t examined = 0;
            for (uint32_t i = 0; i < nc; ++i) {
                const uint64_t p = pos[i];
                const CountedBytes in{src + p, &examined};
                const zr::WrapperHead h = zr::wrapper_parse_rules(2, in, zr::member_header_look(n, p));
                uint32_t bsize = 0;
                if (h.status == 0) zr::gzip_bgzf_bsize(in, n - p, &bsize);
                if (h.status == 0 && h.hcrc) examined += h.header_len - 2;
            }
            printf("%u %llu\n", nc, (unsigned long long)examined);
            return 0;
        }
        for (uint32_t i = 0; i < nc; ++i) {
            const uint64_t p = pos[i];
            const zr::WrapperHead h = zr::wrapper_parse_rules(2, HostBytes{src + p}, zr::member_header_look(n, p));
            zr::CandRow r = {p, h.header_len, 0u, h.status, h.msg, 0u, 0u, 0u};
            uint32_t bsize = 0;
            const bool bgzf = h.status == 0 && zr::gzip_bgzf_bsize(HostBytes{src + p}, n - p, &bsize);
            if (bgzf) r.flags |= zr::kCandBgzf;
            r.next = zr::member_next(pos.data(), nc, i, bgzf, bsize, n);
            const uint64_t end = r.next < nc ? pos[r.next] : n;
            if (h.status == 0 && end >= p + h.header_len + 8) {
                const uint8_t *t = src + end - 8;
                r.crc = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
                r.isize = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
                r.flags |= zr::kCandTrailer;
            }
            print_row(r);
        }
        return 0;
    }
    if (cmd == "plan") {
        uint32_t n, start;
        uint64_t src_len, dst_off, dst_cap;
        if (!(std::cin >> n >> src_len >> start >> dst_off >> dst_cap)) return 2;
        std::vector<zr::CandRow> rows(n);
        for (auto &r : rows) std::cin >> r.pos >> r.header_len >> r.next >> r.status >> r.msg >> r.flags >> r.crc >> r.isize;
        size_t nres;
        std::cin >> nres;
        std::vector<zr::MemberResult> res(nres);
        for (auto &r : res) std::cin >> r.status >> r.out_len >> r.in_used;
        if (!std::cin) return 2;
        zr::MembersPlan plan;
        zr::plan_members(rows.data(), n, src_len, start, dst_off, dst_cap, plan);
        for (const zr::PlannedMember &m : plan.items)
            printf("%u %u %llu %llu %llu %llu %u %u %d\n", m.cand, m.engine, (unsigned long long)m.src_off, (unsigned long long)m.span,
                   (unsigned long long)m.dst_off, (unsigned long long)m.out_guess, m.crc, m.bgzf, m.to_end ? 1 : 0);
        if (plan.alone) printf("alone %u %s\n", plan.solo, plan.bad_guess ? "guess" : "must");
        else printf("end\n");
        printf("dst_end %llu\n", (unsigned long long)plan.dst_end);
        if (nres == plan.items.size()) printf("unverified %zu\n", zr::first_unverified(plan, res.data()));
        return 0;
    }
    if (cmd == "after") {
        uint64_t at, src_len;
        uint32_t b0, b1;
        if (!(std::cin >> at >> src_len >> b0 >> b1)) return 2;
        printf("%s\n", zr::after_member(at, src_len, b0, b1) == zr::kAfterMember ? "member" : "done");
        return 0;
    }
    return 2;
}
