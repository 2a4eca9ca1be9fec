#!/bin/sh
# Sanitizer run of the host rules of BGZF random access (zlib-ng_amd/csrc/bgzf_read_plan.h: chain walk, row check, plan,
# results, virtual offsets).  A stand-alone program, tests/c/bgzf_read_plan_driver.cpp, is built with ASan + UBSan and runs its
# "self" command: every range (uoff, len) over a small members table, at several slot counts and round sizes.  CPU only;
# nothing is loaded into python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -I "$ROOT/zlib-ng_amd/csrc" "$ROOT/tests/c/bgzf_read_plan_driver.cpp" -o "$OUT/bgzf_read_plan_driver"
"$OUT/bgzf_read_plan_driver" self
