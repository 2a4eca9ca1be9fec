"""What a copy of a device-held stream costs: microseconds per zng_rocm_hook_clone for a hook with a full 32 KiB history,
against the only route a caller had without it -- zng_rocm_hook_get_history to the host, zng_rocm_hook_create,
zng_rocm_hook_set_history.  Both are timed as one call sequence including the destroy of what they made (wall clock around
synchronous calls: every one of them waits for its own stream), --rounds times after --warmup untimed rounds; the
figures are the median and the fastest round.  Both routes are checked once: the new hook's history is the source's.
A third row times zng_rocm_hook_create + zng_rocm_hook_destroy alone: what either route spends before a byte of history moves.
No threshold: the figures are what DESIGN.md quotes.  Not part of bench.py.
    python tools/hook_clone_rate.py [--rounds 200] [--warmup 20] [--out FILE]"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def history(lib, h, buf):
    n = C.c_uint32(0)
    assert lib.zng_rocm_hook_get_history(h, C.addressof(buf), C.byref(n)) == 0
    return buf.raw[:n.value]


def by_clone(lib, src, keep=False):
    out = C.c_void_p()
    assert lib.zng_rocm_hook_clone(src, C.byref(out)) == 0
    if keep:
        return out
    lib.zng_rocm_hook_destroy(out)


def by_host(lib, src, buf, keep=False):
    n = C.c_uint32(0)
    assert lib.zng_rocm_hook_get_history(src, C.addressof(buf), C.byref(n)) == 0
    out = C.c_void_p()
    assert lib.zng_rocm_hook_create(C.byref(out), 1 << 20) == 0
    assert lib.zng_rocm_hook_set_history(out, C.addressof(buf), n.value) == 0
    if keep:
        return out
    lib.zng_rocm_hook_destroy(out)


def create_destroy(lib):
    out = C.c_void_p()
    assert lib.zng_rocm_hook_create(C.byref(out), 1 << 20) == 0
    lib.zng_rocm_hook_destroy(out)


def timed(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import synth
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    lib = zr.lib()
    data = synth.silesia_like(32768, seed=2029).tobytes()
    src = C.c_void_p()
    assert lib.zng_rocm_hook_create(C.byref(src), 1 << 20) == 0
    buf, probe = C.create_string_buffer(32768), C.create_string_buffer(32768)
    try:
        assert lib.zng_rocm_hook_set_history(src, data, len(data)) == 0
        for make in (lambda: by_clone(lib, src, keep=True), lambda: by_host(lib, src, buf, keep=True)):
            h = make()
            assert history(lib, h, probe) == data
            lib.zng_rocm_hook_destroy(h)
        res = {"history_bytes": len(data), "rounds": args.rounds, "warmup": args.warmup,
               "includes": "the destroy of the new hook",
               "zng_rocm_hook_clone": timed(lambda: by_clone(lib, src), args.rounds, args.warmup),
               "get_history_create_set_history": timed(lambda: by_host(lib, src, buf), args.rounds, args.warmup),
               "hook_create_destroy_alone": timed(lambda: create_destroy(lib), args.rounds, args.warmup)}
        assert history(lib, src, probe) == data
    finally:
        lib.zng_rocm_hook_destroy(src)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
