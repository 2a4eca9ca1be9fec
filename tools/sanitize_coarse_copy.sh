#!/bin/sh
# Sanitizer run of deflateCopy / inflateCopy through the arch/rocm adapters (integration/arch/rocm/rocm_deflate.c
# archrocm_deflate_copy, rocm_inflate.c archrocm_inflate_copy) and of the adapters' gather / drain / carry state machines,
# none of which run where no GPU is.  One stand-alone program: tests/c/coarse_copy_driver.c, the adapters,
# tests/c/hook_stub.cpp (the zng_rocm_hook_* calls on the CPU: stored blocks out, every hook's history and every decode's
# plaintext a heap block of its own) and the project's host decoder zlib-ng_amd/csrc/inflate_host.cpp, built with ASan + UBSan.
# It runs the cases of tests/test_coarse_copy_cpu.py: every copy point, both orders of ending, every failing allocation
# inside a copy, a refused clone, a diverging copy; the leak check is on.  Outputs are compared with what went in by
# python's zlib, which only reads the files the program wrote.  CPU only; nothing is loaded into python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
ARCH="$ROOT/integration/arch/rocm"
SAN="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined"
INC="-I $ROOT/include -I $ROOT/tests/c -I $ARCH"
for f in "$ROOT/tests/c/coarse_copy_driver.c" "$ARCH/rocm_deflate.c" "$ARCH/rocm_inflate.c" "$ARCH/rocm_slots.c" "$ARCH/rocm_features.c"; do
    gcc -std=c11 -pedantic -Wall -Wextra -Werror $SAN -DZNG_ROCM_STANDALONE_CHECK -DROCM_MIN_BYTES=1024 -DROCM_INFLATE_MIN_BYTES=1 \
        -DROCM_DEFLATE_BLOCK_BYTES=1048576 $INC -c "$f" -o "$OUT/$(basename "$f").o"
done
g++ -std=c++17 -Wall -Wextra -Werror $SAN $INC -c "$ROOT/tests/c/hook_stub.cpp" -o "$OUT/hook_stub.o"
g++ -std=c++17 $SAN $INC -c "$ROOT/zlib-ng_amd/csrc/inflate_host.cpp" -o "$OUT/inflate_host.o"
g++ $SAN -pthread "$OUT"/*.o -o "$OUT/coarse_copy_driver"
export ASAN_OPTIONS=detect_leaks=1
python3 - "$OUT" "$ROOT" <<'EOF'
import sys
work, root = sys.argv[1], sys.argv[2]
sys.path.insert(0, root + "/tests")
import pathlib
import coarse_copy_util as cu
exe, tmp = work + "/coarse_copy_driver", pathlib.Path(work)
p, a, b = cu.inputs()
runs = 0
for point in ("first", "gather", "sync", "drain", "finish", "copy2"):
    for order in (0, 1):
        for kw in (dict(), dict(level=0), dict(w_bits=10), dict(strategy=3), dict(wrap=0)):
            res, src, cpy = cu.deflate_copy(exe, tmp, point, order, **kw)
            cu.check_deflate_round_trip(res, src, cpy, point, wrap=kw.get("wrap", 1))
            runs += 1
for point in ("gather", "sync", "drain"):
    res, src, cpy = cu.deflate_copy(exe, tmp, point, 0, env={"HOOK_STUB_FAIL_CLONE": "1"})
    assert res["failed"] is None and cu.inflate_zlib(src, 1) == p + a, res
    for k in (1, 2, 3):
        res, src, cpy = cu.deflate_copy(exe, tmp, point, 1, env={"COPY_DRIVER_FAIL_ALLOC": str(k)})
        assert cu.inflate_zlib(src, 1) == p + a, res
        runs += 1
n = len(cu.zstream())
for point, (at, last_out) in cu.inflate_points(n).items():
    for order in (0, 1):
        res, src, cpy = cu.inflate_copy(exe, tmp, at, last_out, order)
        assert res["failed"] is None and src == p and cpy == p, res
        bad, expected = cu.flipped(cu.zstream(), at)
        res, src, cpy = cu.inflate_copy(exe, tmp, at, last_out, order, alt=bad)
        assert src == p and res["copy"][len("data error: "):] in expected, res
        runs += 2
    for env in ({"COPY_DRIVER_FAIL_ALLOC": "1"}, {"COPY_DRIVER_FAIL_ALLOC": "2"}, {"COPY_DRIVER_FAIL_ALLOC": "3"},
                {"HOOK_STUB_FAIL_CLONE": "1"}):
        res, src, cpy = cu.inflate_copy(exe, tmp, at, last_out, 0, env=env)
        assert src == p, res
        runs += 1
res, src, cpy = cu.inflate_copy(exe, tmp, 0, wbits=14)
assert res["src"].split()[0] == "fallback" and res["copy"].split()[0] == "fallback", res
print("sanitize_coarse_copy: %d runs clean" % (runs + 1))
EOF
