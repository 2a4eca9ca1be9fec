#!/bin/sh
# Sanitizer run of the host rules of the zng_rocm_*_window_* calls (zlib-ng_amd/csrc/deflate_window_plan.h: which windowBits are
# taken, the distance cap and the priming length they mean, the zlib header they write).  A stand-alone program,
# tests/c/window_plan_driver.cpp, is built with ASan + UBSan and runs its "self" command: every format and windowBits from -16
# to 32, the cap and priming tables, segment starts around the batch and segment borders, and the header bytes of every window,
# level and strategy.  CPU only; nothing is loaded into python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -I "$ROOT/zlib-ng_amd/csrc" "$ROOT/tests/c/window_plan_driver.cpp" -o "$OUT/window_plan_driver"
"$OUT/window_plan_driver" self
