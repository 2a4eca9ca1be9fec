#!/bin/sh
# Sanitizer run of the wrapper rules that the callers holding a whole member share (zlib-ng_amd/csrc/framing_parse.h:
# wrapper_parse_whole over wrapper_parse_rules, wrapper_trailer_verdict, the canonical writer).  A stand-alone program,
# tests/c/wrapper_whole_driver.cpp, is built with ASan + UBSan and runs its "self" command: every prefix of zlib and gzip
# members and every mutation of their first four bytes, each parsed in a heap block of exactly its length, through both ways of
# reaching the bytes.  CPU only; nothing is loaded into python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -I "$ROOT/zlib-ng_amd/csrc" "$ROOT/tests/c/wrapper_whole_driver.cpp" -o "$OUT/wrapper_whole_driver"
"$OUT/wrapper_whole_driver" self
