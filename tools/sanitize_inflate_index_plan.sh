#!/bin/sh
# Sanitizer run of the host rules of the inflate index (zlib-ng_amd/csrc/inflate_index_plan.h: selection, window offsets, the
# read plan, results, the saved form and its check).  A stand-alone program, tests/c/inflate_index_plan_driver.cpp, is built
# with ASan + UBSan and runs its "self" command: candidates of two pieces, ranges over three points at two scratch sizes, a
# span of 4 GiB, a blob written, checked, cut and changed.  CPU only; nothing is loaded into python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -I "$ROOT/zlib-ng_amd/csrc" "$ROOT/tests/c/inflate_index_plan_driver.cpp" -o "$OUT/inflate_index_plan_driver"
"$OUT/inflate_index_plan_driver" self
