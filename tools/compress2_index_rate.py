"""What an index written while compressing costs beside compressing alone, and beside compressing and then decoding the whole
stream again to build one.

One stream, device-resident: --mib (256) MiB of synth.silesia_like, gzip (format 2), level --level (6), span --span-kib (1024).
Three ways over it, alternating inside one process, one untimed warm-up each, then --reps (5) timings each; a figure is the
MEDIAN host time around a call that ends in a synchronise, with min and max beside it:

  compress          zng_rocm_compress2_dev alone: the parent's path, untouched by the index call
  compress_index    zng_rocm_compress2_index_dev (index created and destroyed inside the timing)
  compress_build    zng_rocm_compress2_dev, then zng_rocm_inflate_index_build_dev on what it wrote: the only way to an index
                    before, with its plaintext-sized destination (index created and destroyed inside the timing)

Recorded, not gated: the three times, index / compress and build-way / compress, the points and the exported bytes of both
indexes, the longest span of each.  Checked: both calls write the same stream; the new index's spans are below span + 65536;
64 ranges read through it equal the plaintext.

    python tools/compress2_index_rate.py [--mib 256] [--reps 5] [--out FILE.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KiB, MiB = 1 << 10, 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--span-kib", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compress2_index_rate_v1.json"))
    a = ap.parse_args()
    assert a.reps >= 1 and a.mib >= 1
    import torch
    import synth
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    rocm = zr.rocm
    lib = rocm.lib()
    inf = importlib.import_module("zlib-ng_amd.inflate")
    one = importlib.import_module("zlib-ng_amd.oneshot")
    st = torch.cuda.Stream()
    sp = C.c_void_p(st.cuda_stream)
    fmt, span, n = 2, a.span_kib * KiB, a.mib * MiB

    plain = synth.silesia_like(n, seed=0xC21D)
    src = torch.from_numpy(plain).cuda()
    cap = one.compress_bound(n, fmt)
    dst_a = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    dst_b = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    back = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    out_len, in_used = C.c_uint64(0), C.c_size_t(0)
    clen = {}

    def compress(keep=None):
        dlen = C.c_size_t(cap)
        assert lib.zng_rocm_compress2_dev(rocm._dev_ptr(dst_a), C.byref(dlen), rocm._dev_ptr(src), n, a.level, fmt, sp) == 0
        clen["compress"] = dlen.value

    def compress_index(keep=None):
        dlen, h = C.c_size_t(cap), C.c_void_p(None)
        assert lib.zng_rocm_compress2_index_dev(rocm._dev_ptr(dst_b), C.byref(dlen), rocm._dev_ptr(src), n, a.level, fmt, span, C.byref(h), sp) == 0
        clen["compress_index"] = dlen.value
        if keep is not None:
            keep["compress_index"] = h.value
        else:
            lib.zng_rocm_inflate_index_destroy(h)

    def compress_build(keep=None):
        compress()
        h = C.c_void_p(None)
        assert lib.zng_rocm_inflate_index_build_dev(fmt, rocm._dev_ptr(dst_a), clen["compress"], rocm._dev_ptr(back), n, C.byref(out_len),
                                                    C.byref(in_used), span, 0, 0, C.byref(h), sp) == 1
        if keep is not None:
            keep["compress_build"] = h.value
        else:
            lib.zng_rocm_inflate_index_destroy(h)

    ways = {"compress": compress, "compress_index": compress_index, "compress_build": compress_build}
    kept = {}
    per = {k: [] for k in ways}
    with torch.cuda.stream(st):
        for fn in ways.values():                          # warm-up: allocates the scratch; keeps one index of each kind
            fn(kept)
        st.synchronize()
        for _ in range(a.reps):
            for k, fn in ways.items():
                st.synchronize()
                t0 = time.perf_counter()
                fn()
                st.synchronize()
                per[k].append(time.perf_counter() - t0)
        assert clen["compress"] == clen["compress_index"] and torch.equal(dst_a[:clen["compress"]], dst_b[:clen["compress"]])
        assert (out_len.value, in_used.value) == (n, clen["compress"]) and torch.equal(back[:n], src)

        def figure(v):
            med = statistics.median(v)
            return dict(ms=round(med * 1e3, 4), min_ms=round(min(v) * 1e3, 4), max_ms=round(max(v) * 1e3, 4), gbps=round(n / med / 1e9, 3))

        out = {"tool": "tools/compress2_index_rate.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
               "figure": "median of reps, host clock around a call that ends in a synchronise; GB/s of plaintext",
               "plain_bytes": n, "file_bytes": clen["compress"], "level": a.level, "format": fmt, "span_bytes": span}
        for k in ways:
            out[k] = figure(per[k])
        out["compress_index_over_compress"] = round(out["compress_index"]["ms"] / out["compress"]["ms"], 4)
        out["compress_build_over_compress"] = round(out["compress_build"]["ms"] / out["compress"]["ms"], 4)
        for k, h in kept.items():
            idx = inf.InflateIndex(h)
            pts = idx.points()
            ends = [p[1] for p in pts[1:]] + [n]
            out[k].update(points=len(pts), index_bytes=len(idx.save(stream=st)), longest_span=max(e - p[1] for p, e in zip(pts, ends)))
            if k == "compress_index":
                assert out[k]["longest_span"] < span + 65536
                rng = np.random.default_rng(0xC21E)
                ranges = [(int(u), 100000, torch.zeros(100000, dtype=torch.uint8, device="cuda")) for u in rng.integers(0, n - 100000, size=64)]
                rc, res, _ = idx.read(dst_b[:clen["compress"]], ranges, stream=st)
                st.synchronize()
                assert rc == 0 and all(r == (1, 100000, None) for r in res)
                assert all(torch.equal(d, src[u:u + 100000]) for u, _, d in ranges)
            idx.close()
    lib.zng_rocm_stream_release(sp)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
