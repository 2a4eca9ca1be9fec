#!/bin/sh
# Sanitizer run of the host inflaters over the decoy streams of tests/decoy_cases.py: valid streams whose stored payload
# imitates block starts by the thousand (00 00 ff ff, stored headers that chain to each other and onto genuine starts, dynamic
# headers at every bit offset, FINAL blocks of other text behind a marker).  The generator writes every stream to a
# temporary directory; a stand-alone program, tests/c/inflate_decoys_driver.cpp, is built with ASan + UBSan from
# inflate_host.cpp + inflate_threads.cpp, decodes each file on one thread and on eight, replays both token streams and prints
# status / lengths / parts, which are compared here with the lengths the generator expects.  CPU only; nothing is loaded
# into python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -pthread -I "$ROOT/include" "$ROOT/tests/c/inflate_decoys_driver.cpp" "$ROOT/zlib-ng_amd/csrc/inflate_host.cpp" \
    "$ROOT/zlib-ng_amd/csrc/inflate_threads.cpp" -o "$OUT/inflate_decoys_driver"
(cd "$ROOT/tests" && python3 - "$OUT" <<'PY'
import sys
import decoy_cases
with open(sys.argv[1] + "/expect.txt", "w") as f:
    for k, name in enumerate(decoy_cases.ALL):
        s = decoy_cases.get(name)
        with open("%s/%02d.deflate" % (sys.argv[1], k), "wb") as g:
            g.write(s.comp)
        for threads in (1, 8):
            f.write("%s/%02d.deflate %d 1 %d %d\n" % (sys.argv[1], k, threads, len(s.plain), len(s.comp)))
PY
)
ASAN_OPTIONS=detect_leaks=1 "$OUT/inflate_decoys_driver" "$OUT"/*.deflate > "$OUT/got.txt"
cut -d' ' -f1-5 "$OUT/got.txt" | cmp - "$OUT/expect.txt"
sed "s|$OUT/||" "$OUT/got.txt"
