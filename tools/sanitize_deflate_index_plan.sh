#!/bin/sh
# Sanitizer run of the host rules of zng_rocm_compress2_index_dev (zlib-ng_amd/csrc/deflate_index_plan.h: the refusal order, the
# level-0 block starts in closed form, the block rows of the rows engine turned into candidates, the span bound).  A stand-alone
# program, tests/c/deflate_index_plan_driver.cpp, is built with ASan + UBSan and runs its "self" command -- every function over
# every border length, the candidates through index_select at five spans, against the bound.  CPU only; nothing is loaded into
# python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -I "$ROOT/zlib-ng_amd/csrc" "$ROOT/tests/c/deflate_index_plan_driver.cpp" -o "$OUT/deflate_index_plan_driver"
"$OUT/deflate_index_plan_driver" self
