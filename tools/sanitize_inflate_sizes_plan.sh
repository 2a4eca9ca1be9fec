#!/bin/sh
# Sanitizer run of the host rules of zng_rocm_inflate_sizes_dev / zng_rocm_uncompress_packed_dev
# (zlib-ng_amd/csrc/inflate_sizes_plan.h: argument checks, the saturation of a stream's count, the sizing row of a wrapped member,
# places, the fit against dst_cap, final rows).  A stand-alone program, tests/c/inflate_sizes_plan_driver.cpp, is built with
# ASan + UBSan and runs its "self" command -- every format with and without a dictionary, counts around 0x7fffffff, batches of
# sizes around every alignment with jobs that take no room, the prefix-sum form of the places against the running rule -- and a
# batch whose offsets pass 2^32.  CPU only; nothing is loaded into python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -I "$ROOT/zlib-ng_amd/csrc" "$ROOT/tests/c/inflate_sizes_plan_driver.cpp" -o "$OUT/inflate_sizes_plan_driver"
"$OUT/inflate_sizes_plan_driver" self
"$OUT/inflate_sizes_plan_driver" places 4096 0x300000000 1 0x7fffffff 1 0x7fffffff -3 5 1 0x7fffffff 1 1 > /dev/null
