// Drives zlib-ng_amd/csrc/bgzf_plan.h on the host (tests/test_bgzf_plan_cpu.py).  Commands (argv[1], numbers in argv[2..]):
//   cut SRC_LEN BLOCK_BYTES ROUND_BYTES   "<piece> <pieces> <pieces per round> <rounds> <bound>", then one line per round
//                                         "<first piece> <pieces> <first byte> <bytes>" and one line with every piece's length;
//                                         "refused 0" for a block_bytes the call refuses (the 0 is the bound)
//   member N CLEN                         "<payload> <stored> <member bytes>" (bgzf_member)
//   frame PAYLOAD CRC N                   hex of the 18 header bytes, the 8 trailer bytes and the 5 bytes of the stored block
//                                         header around N bytes, one line each
//   eof                                   hex of the end-of-file block: the table, then bgzf_eof_byte
//   args LEVEL HAVE_SRC SRC_LEN BLOCK_BYTES HAVE_DST DST_CAP HAVE_OUT HAVE_MEMBERS MEMBERS_CAP HAVE_N FLAGS
//                                         "ok <level 0..9>" or "refused"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "bgzf_plan.h"

namespace {

void hex(const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
    printf("\n");
}

uint64_t num(char **argv, int i) { return strtoull(argv[i], nullptr, 0); }

}  // namespace

int main(int argc, char **argv) {
    using namespace zr;
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "cut" && argc == 5) {
        const uint64_t src_len = num(argv, 2), round_bytes = num(argv, 4);
        const uint32_t block = (uint32_t)num(argv, 3), piece = bgzf_piece_bytes(block);
        if (!piece) {
            printf("refused %llu\n", (unsigned long long)bgzf_bound(src_len, block));
            return 0;
        }
        const uint64_t np = bgzf_pieces(src_len, piece), per = bgzf_round_pieces(round_bytes, piece);
        printf("%u %llu %llu %llu %llu\n", piece, (unsigned long long)np, (unsigned long long)per,
               (unsigned long long)bgzf_rounds(src_len, piece, round_bytes), (unsigned long long)bgzf_bound(src_len, block));
        for (uint64_t first = 0; first < np; first += per) {
            const uint64_t n = np - first < per ? np - first : per;
            uint64_t bytes = 0;
            for (uint64_t g = first; g < first + n; ++g) bytes += bgzf_piece_len(src_len, piece, g);
            printf("%llu %llu %llu %llu\n", (unsigned long long)first, (unsigned long long)n, (unsigned long long)(first * piece),
                   (unsigned long long)bytes);
        }
        for (uint64_t g = 0; g < np; ++g) printf("%u ", bgzf_piece_len(src_len, piece, g));
        printf("\n");
        return 0;
    }
    if (cmd == "member" && argc == 4) {
        const BgzfMember m = bgzf_member((uint32_t)num(argv, 2), (uint32_t)num(argv, 3));
        printf("%u %u %u\n", m.payload, m.stored, bgzf_member_bytes(m));
        return 0;
    }
    if (cmd == "frame" && argc == 5) {
        const uint32_t payload = (uint32_t)num(argv, 2), crc = (uint32_t)num(argv, 3), n = (uint32_t)num(argv, 4);
        uint8_t head[kBgzfHead], tail[kBgzfTail], stored[kBgzfStoredHead];
        bgzf_put_header(head, kBgzfHead + payload + kBgzfTail);
        bgzf_put_trailer(tail, crc, n);
        for (uint32_t k = 0; k < kBgzfStoredHead; ++k) stored[k] = bgzf_stored_byte(k, n);
        hex(head, sizeof head);
        hex(tail, sizeof tail);
        hex(stored, sizeof stored);
        return 0;
    }
    if (cmd == "eof") {
        uint8_t b[kBgzfEofBytes];
        for (uint32_t k = 0; k < kBgzfEofBytes; ++k) b[k] = bgzf_eof_byte(k);
        hex(kBgzfEof, sizeof kBgzfEof);
        hex(b, sizeof b);
        return 0;
    }
    if (cmd == "args" && argc == 13) {
        static const char some = 0;
        auto ptr = [&](int i) -> const void * { return num(argv, i) ? &some : nullptr; };
        const int level = atoi(argv[2]);
        const bool ok = bgzf_args_ok(level, ptr(3), num(argv, 4), (uint32_t)num(argv, 5), ptr(6), num(argv, 7), ptr(8), ptr(9),
                                     num(argv, 10), ptr(11), (uint32_t)num(argv, 12));
        if (ok) printf("ok %d\n", bgzf_level(level));
        else printf("refused\n");
        return 0;
    }
    fprintf(stderr, "unknown command\n");
    return 2;
}
