#!/bin/sh
# Sanitizer run of the host rules of the large inflater's pieces loop (zlib-ng_amd/csrc/inflate_large_plan.h: the next piece,
# the pass's buffer and re-basing, the steps behind a pass and behind the sequential decoder, halving, the history).  A
# stand-alone program, tests/c/large_plan_driver.cpp, is built with ASan + UBSan and runs its "self" command: the state
# machine stepped over synthetic pass outcomes for a sweep of stream lengths, piece sizes and keys.  CPU only; nothing is
# loaded into python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -I "$ROOT/zlib-ng_amd/csrc" "$ROOT/tests/c/large_plan_driver.cpp" -o "$OUT/large_plan_driver"
"$OUT/large_plan_driver" self
