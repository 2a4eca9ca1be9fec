#!/bin/sh
# Sanitizer run of the rules that hold one stream of the level-1 class kernels to its 32-bit contract
# (zlib-ng_amd/csrc/deflate_quick_plan.h: the bound and the largest in_len, the flush rule of the bit ring under a cursor that
# wraps at 2^32 bits, the Adler-32 fold, the job check).  A stand-alone program, tests/c/deflate_quick_plan_driver.cpp, is built
# with ASan + UBSan and runs its "self" command: walks of 20000 batches from the start of a stream, across every wrap of the
# cursor and up to the last bit of the largest stream, each beside true 64-bit counters; the fold with every lane at its largest;
# the job check at and above the largest in_len.  CPU only; nothing is loaded into python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -I "$ROOT/zlib-ng_amd/csrc" "$ROOT/tests/c/deflate_quick_plan_driver.cpp" -o "$OUT/deflate_quick_plan_driver"
"$OUT/deflate_quick_plan_driver" self
