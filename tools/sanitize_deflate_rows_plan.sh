#!/bin/sh
# Sanitizer run of the host rules of the rows deflate engine (zlib-ng_amd/csrc/deflate_rows_plan.h: the sizes, the argument
# checks, the round cut, and the planner that cuts streams into segments and segments into blocks).  A stand-alone program,
# tests/c/deflate_rows_plan_driver.cpp, is built with ASan + UBSan and runs its "self" command -- the planner over job lists of
# every border length, own and shared histories and the three dst_cap rules, into tables of exactly the size its counting pass
# gives, against its own invariants -- and its "sweep" command, the block cut over every dict_len mod 1024.  CPU only; nothing
# is loaded into python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -I "$ROOT/zlib-ng_amd/csrc" "$ROOT/tests/c/deflate_rows_plan_driver.cpp" -o "$OUT/deflate_rows_plan_driver"
"$OUT/deflate_rows_plan_driver" self
"$OUT/deflate_rows_plan_driver" sweep
