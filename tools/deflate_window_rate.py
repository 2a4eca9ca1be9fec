"""Rate and size of device deflate at deflateInit2's windowBits (zng_rocm_deflate_window_block_dev) against the call without a
window: the 256 MiB level-6 input of bench.py's deflate_lvl6 leg (synth.silesia_like, seed 0x5EED0003), device resident,
compressed at windowBits 9, 12, 14, at 15 through the new call and at 15 through the old call (zng_rocm_deflate_block_dev).
The five variants alternate in one process after a warm-up call each, --repeats rounds; a time is a host clock around a
synchronous call (it ends in a device synchronise).  Per variant: every time, the median and best GB/s of input, the compressed
size; `spread_old` is (slowest - fastest) / median over the repeats of the OLD call, the yardstick every difference is held
against.  For the first --cpu-mib MiB: device size / CPython zlib size at level 6 and the same wbits, whole and per class of
synth.segment (256 KiB each, the classes of tests/test_gpu_deflate_window.py).  Not part of bench.py.
    python tools/deflate_window_rate.py [--mib 256] [--repeats 5] [--cpu-mib 16] [--out profiles/deflate_window_rate_v1.json]"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VARIANTS = [("w9", 9), ("w12", 12), ("w14", 14), ("w15_new", 15), ("w15_old", None)]
LEVEL = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-mib", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import synth
    import window_cases as wc
    zr = importlib.import_module("zlib-ng_amd")
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    rocm = importlib.import_module("zlib-ng_amd.rocm")
    zr.init()
    lib = rocm.lib()
    n = a.mib << 20
    plain = synth.silesia_like(n, seed=0x5EED0003)
    src = torch.from_numpy(np.concatenate([plain, np.zeros(16, np.uint8)])).cuda()
    cap = dfl.deflate_bound(n)
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call(w, length=n):
        """one synchronous call -> compressed length.  w None: the call without a window"""
        out_len = C.c_size_t(0)
        st = rocm._stream_ptr(None)
        if w is None:
            rc = lib.zng_rocm_deflate_block_dev(LEVEL, rocm._dev_ptr(src), length, 0, 0, rocm._dev_ptr(dst), cap, C.byref(out_len), st)
        else:
            rc = lib.zng_rocm_deflate_window_block_dev(LEVEL, 0, w, rocm._dev_ptr(src), length, 0, 0, rocm._dev_ptr(dst), cap,
                                                       C.byref(out_len), st)
        assert rc == 0, (w, rc)
        return int(out_len.value)

    res = {"what": __doc__.split("\n")[0], "input": "synth.silesia_like(%d MiB, seed=0x5EED0003), level %d" % (a.mib, LEVEL),
           "repeats": a.repeats, "rows": {}}
    sizes, digests = {}, {}
    for name, w in VARIANTS:                                     # warm-up, the size, and a reader's verdict on the head of it
        sizes[name] = call(w)
        comp = dst[:sizes[name]].cpu().numpy()
        digests[name] = zlib.crc32(comp.tobytes())
        d = zlib.decompressobj(-(w or 15))
        assert d.decompress(comp[:2 << 20].tobytes(), 2 << 20) == plain[:2 << 20].tobytes(), name
    assert sizes["w15_new"] == sizes["w15_old"] and digests["w15_new"] == digests["w15_old"], "15 must give the old call's bytes"
    times = {name: [] for name, _ in VARIANTS}
    for _ in range(a.repeats):                                   # alternating: every round takes each variant once
        for name, w in VARIANTS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            clen = call(w)
            times[name].append(time.perf_counter() - t0)
            assert clen == sizes[name]
    for name, w in VARIANTS:
        ts = times[name]
        med = statistics.median(ts)
        res["rows"][name] = {"window_bits": w or 15, "call": "zng_rocm_deflate_block_dev" if w is None else "zng_rocm_deflate_window_block_dev",
                             "bytes": sizes[name], "ratio": round(sizes[name] / n, 4), "seconds_all": [round(t, 5) for t in ts],
                             "GBps_median": round(n / med / 1e9, 3), "GBps_best": round(n / min(ts) / 1e9, 3),
                             "spread": round((max(ts) - min(ts)) / med, 4)}
        print(name, res["rows"][name], flush=True)
    old = res["rows"]["w15_old"]
    res["spread_old"] = old["spread"]
    for name, _ in VARIANTS:
        res["rows"][name]["median_vs_old"] = round(res["rows"][name]["GBps_median"] / old["GBps_median"], 4)

    # size against CPython at the same window: the first --cpu-mib MiB, whole and per class
    m = min(a.cpu_mib << 20, n)
    head = plain[:m].tobytes()
    res["cpython"] = {"zlib_version": zlib.ZLIB_RUNTIME_VERSION, "bytes_in": m, "level": LEVEL, "rows": {}}
    for name, w in VARIANTS[:4]:
        z = zlib.compressobj(LEVEL, zlib.DEFLATED, -w)
        ref = len(z.compress(head) + z.flush())
        got = call(w, m)
        assert wc.reader(-w, dst[:got].cpu().numpy().tobytes(), chunk=1 << 16) == (head, True, b""), name
        res["cpython"]["rows"][name] = {"device_bytes": got, "cpython_bytes": ref, "device_over_cpython": round(got / ref, 4)}
        print("cpython", name, res["cpython"]["rows"][name], flush=True)
    per_class = {}
    for k, kind in enumerate(synth.CLASSES):
        part = synth.segment(kind, 256 << 10, np.random.default_rng([0x5123, k]))
        data = np.concatenate([part, np.zeros((256 << 10) - part.size, dtype=np.uint8)])
        csrc = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).cuda()
        per_class[kind] = {}
        for name, w in VARIANTS[:4]:
            cdst, clen = dfl.deflate_dev(csrc, level=LEVEL, length=data.size, window_bits=w)
            z = zlib.compressobj(LEVEL, zlib.DEFLATED, -w)
            per_class[kind][name] = round(clen / len(z.compress(data.tobytes()) + z.flush()), 4)
    res["cpython"]["per_class_device_over_cpython"] = per_class
    res["cpython"]["classes_worse_than_15_by_more_than_0.05"] = sorted(
        "%s/%s" % (kind, name) for kind, row in per_class.items() for name in ("w9", "w12", "w14") if row[name] > row["w15_new"] + 0.05)
    print("per class", per_class, flush=True)
    line = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(json.dumps({k: v["GBps_median"] for k, v in res["rows"].items()}))


if __name__ == "__main__":
    main()
