#!/bin/sh
# Sanitizer run of the host rules of zng_rocm_compress_streams2_dev / zng_rocm_compress_members_dev
# (zlib-ng_amd/csrc/compress_streams_plan.h: argument checks, rounds, header and trailer bytes, stored sizes, bounds).  A
# stand-alone program, tests/c/compress_streams_plan_driver.cpp, is built with ASan + UBSan and runs its "self" command: every
# format, level and strategy, the stored sizes around the 65535-byte cut, and the rounds of a job list at several round sizes.
# CPU only; nothing is loaded into python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -I "$ROOT/zlib-ng_amd/csrc" "$ROOT/tests/c/compress_streams_plan_driver.cpp" -o "$OUT/compress_streams_plan_driver"
"$OUT/compress_streams_plan_driver" self
