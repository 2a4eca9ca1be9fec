"""Output rate of the streaming inflate hook THROUGH THE ADAPTER: tests/c/coarse_stream_driver.c (inflate()'s control flow
around INFLATE_TYPEDO_HOOK, integration/arch/rocm/rocm_inflate.c linked in) on one 256 MiB CPython level-6 zlib stream,
fed in pieces of 64 KiB, 1 MiB, 16 MiB and in one piece.  Each figure is the best of the driver's timed passes after the
first (COARSE_STREAM_PASSES: the whole feed again, the hook reset in between, so start-up and first allocations stay in
pass 1).  The adapter's carry copies, its drain into next_out and the trailer check are inside the figures.
Baseline: zng_rocm_hook_inflate, the whole-stream hook, on the same deflate data in one piece through ctypes (best of
--passes - 1 after one warm-up call); and zng_rocm_hook_inflate_blocks in one piece the same way, for the hook alone.
GB/s of plaintext.  Not part of bench.py.
    python tools/hook_stream_rate.py [--mib 256] [--passes 4] [--out FILE]"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build_driver(zr, d):
    """the coarse_stream_driver, built as tests/test_gpu_hook_stream.py builds it (ROCM_INFLATE_MIN_BYTES=1: the adapter
    as shipped leaves a stream whose first call brings less than 1 MiB to software, and the 64 KiB row would measure
    nothing of the device)"""
    libdir = os.path.dirname(zr.lib_path())
    exe = os.path.join(d, "coarse_stream_driver")
    arch = os.path.join(ROOT, "integration", "arch", "rocm")
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-DZNG_ROCM_STANDALONE_CHECK", "-DROCM_INFLATE_MIN_BYTES=1", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "c"), "-I" + arch,
                           os.path.join(ROOT, "tests", "c", "coarse_stream_driver.c")] +
                          [os.path.join(arch, f) for f in ("rocm_deflate.c", "rocm_inflate.c", "rocm_slots.c", "rocm_features.c")] +
                          ["-o", exe, "-L" + libdir, "-lzng_rocm", "-Wl,-rpath," + libdir])
    return exe


def through_adapter(exe, d, comp, plain_len, piece, passes):
    cuts = os.path.join(d, "cuts.txt")
    with open(cuts, "w") as f:
        f.write("\n".join(str(c) for c in range(piece, len(comp), piece)) + "\n")
    p = subprocess.run([exe, "1", str(16 << 20), os.path.join(d, "in.z"), cuts, os.path.join(d, "out.bin")],
                       capture_output=True, text=True, timeout=1200, env=dict(os.environ, COARSE_STREAM_PASSES=str(passes)))
    assert p.returncode == 0, (p.returncode, p.stdout[-1000:], p.stderr[-1000:])
    lines = p.stdout.splitlines()
    assert "end %d 0 %d" % (len(comp), plain_len) in lines, lines[-4:]          # Z_STREAM_END, trailer checked
    secs = [float(ln.split()[1]) for ln in lines if ln.startswith("seconds ")]
    assert len(secs) == passes
    return round(plain_len / min(secs[1:]) / 1e9, 3), [round(s, 4) for s in secs]


def hook_call(lib, h, buf, n, blocks):
    cv = C.c_uint32(1)
    out, out_len, used, end_bit, msg = C.c_void_p(), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0), C.c_char_p()
    if blocks:
        st = lib.zng_rocm_hook_inflate_blocks(h, C.addressof(buf), n, 0, 1, C.byref(cv), C.byref(out), C.byref(out_len),
                                              C.byref(end_bit), C.byref(msg))
    else:
        st = lib.zng_rocm_hook_inflate(h, C.addressof(buf), n, 1, C.byref(cv), C.byref(out), C.byref(out_len),
                                       C.byref(used), C.byref(msg))
    assert st == 1, st
    return out_len.value, cv.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import synth
    zr = importlib.import_module("zlib-ng_amd")
    inf = importlib.import_module("zlib-ng_amd.inflate")
    plain = synth.silesia_like(args.mib << 20, seed=2028).tobytes()
    comp = zlib.compress(plain, 6)
    raw = comp[2:-4]
    want = zlib.adler32(plain)
    rows, spans = {}, {}
    zr.init(0)
    hook = inf.InflateHook()
    try:
        buf = C.create_string_buffer(raw, len(raw))
        for name, blocks in (("baseline_hook_inflate_one_piece", False), ("hook_inflate_blocks_one_piece", True)):
            hook_call(hook.lib, hook.h, buf, len(raw), blocks)                      # warm-up
            best = None
            for _ in range(args.passes - 1):
                hook.set_history(b"")
                t0 = time.perf_counter()
                n, cv = hook_call(hook.lib, hook.h, buf, len(raw), blocks)
                dt = time.perf_counter() - t0
                assert (n, cv) == (len(plain), want)
                best = dt if best is None else min(best, dt)
            rows[name] = round(len(plain) / best / 1e9, 3)
    finally:
        hook.close()
    with tempfile.TemporaryDirectory(prefix="hook_stream_rate_") as d:
        exe = build_driver(zr, d)
        with open(os.path.join(d, "in.z"), "wb") as f:
            f.write(comp)
        for name, piece in (("adapter_64KiB", 64 << 10), ("adapter_1MiB", 1 << 20), ("adapter_16MiB", 16 << 20),
                            ("adapter_one_piece", len(comp))):
            rows[name], spans[name] = through_adapter(exe, d, comp, len(plain), piece, args.passes)
    res = {"plain_bytes": len(plain), "compressed_bytes": len(comp), "GBps_output": rows, "pass_seconds": spans}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
