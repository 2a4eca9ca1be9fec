"""Rate and ratio of zlib's strategies on the device (zng_rocm_deflate_strategy_block_dev) against CPython's zlib with the
same strategies on the same bytes: one stream of `--mib` MiB of synth.silesia_like, device resident, compressed at level 6
(default strategy), Z_FIXED at level 6, Z_RLE and Z_HUFFMAN_ONLY.  Device figures: the best of --passes synchronous calls
after one warm-up call (host clock around a call that ends in a device synchronise).  CPython: one call each.  GB/s of
input; ratio = compressed / input.  Not part of bench.py.
    python tools/deflate_strategy_rate.py [--mib 256] [--passes 5] [--cpu-mib 256] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROWS = [("level6", 6, 0), ("fixed_level6", 6, 4), ("rle", 6, 3), ("huffman_only", 6, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--cpu-mib", type=int, default=None, help="CPython on the first N MiB only (default: all)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import synth
    zr = importlib.import_module("zlib-ng_amd")
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    zr.init()
    n = a.mib << 20
    plain = synth.silesia_like(n, seed=0x5EED0006)
    src = torch.from_numpy(np.concatenate([plain, np.zeros(16, np.uint8)])).cuda()
    torch.cuda.synchronize()
    res = {"what": __doc__.split("\n")[0], "input": "synth.silesia_like(%d MiB, seed=0x5EED0006)" % a.mib,
           "passes": a.passes, "rows": {}}
    for name, level, strategy in ROWS:
        dst, clen = dfl.deflate_dev(src, level=level, length=n, strategy=strategy)          # warm-up, and the output
        comp = dst[:clen].cpu().numpy().tobytes()
        assert zlib.decompress(comp, -15) == plain.tobytes(), name
        del dst
        times = []
        for _ in range(a.passes):
            t0 = time.perf_counter()
            dst, clen2 = dfl.deflate_dev(src, level=level, length=n, strategy=strategy)
            times.append(time.perf_counter() - t0)
            assert clen2 == clen
            del dst
        best = min(times)
        res["rows"][name] = {"level": level, "strategy": strategy, "bytes": clen, "ratio": round(clen / n, 4),
                             "seconds_best": round(best, 5), "seconds_all": [round(t, 5) for t in times],
                             "GBps": round(n / best / 1e9, 3)}
        print(name, res["rows"][name], flush=True)
    base = res["rows"]["level6"]["seconds_best"]
    for name in ("fixed_level6", "rle", "huffman_only"):
        res["rows"][name]["time_vs_level6"] = round(res["rows"][name]["seconds_best"] / base, 3)
    m = (a.cpu_mib or a.mib) << 20
    data = plain[:m].tobytes()
    res["cpython"] = {"zlib_version": zlib.ZLIB_RUNTIME_VERSION, "bytes_in": m, "rows": {}}
    for name, level, strategy in ROWS:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        t0 = time.perf_counter()
        out = c.compress(data) + c.flush()
        dt = time.perf_counter() - t0
        res["cpython"]["rows"][name] = {"bytes": len(out), "ratio": round(len(out) / m, 4), "seconds": round(dt, 3),
                                        "GBps": round(m / dt / 1e9, 4)}
        print("cpython", name, res["cpython"]["rows"][name], flush=True)
    line = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(json.dumps({k: v["GBps"] for k, v in res["rows"].items()}))


if __name__ == "__main__":
    main()
