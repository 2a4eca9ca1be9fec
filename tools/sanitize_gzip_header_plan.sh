#!/bin/sh
# Sanitizer run of the host rules of the gzip header fields (zlib-ng_amd/csrc/gzip_header_plan.h: what
# zng_rocm_compress_members_header_dev renders and zng_rocm_gzip_headers_dev / zng_rocm_gzip_header_parse read).  A stand-alone
# program, tests/c/gzip_header_plan_driver.cpp, is built with ASan + UBSan and runs its "self" command: all 32 flag combinations
# with empty, small and 65535-byte fields, every truncation of the rendered headers against wrapper_parse_rules from heap blocks
# of exactly the cut's length, a flipped FHCRC, every refusal, and the gather layout of a table with refused members.
# CPU only; nothing is loaded into python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -I "$ROOT/zlib-ng_amd/csrc" "$ROOT/tests/c/gzip_header_plan_driver.cpp" -o "$OUT/gzip_header_plan_driver"
"$OUT/gzip_header_plan_driver" self
