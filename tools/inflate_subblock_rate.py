"""Rates of ONE large raw stream inflated on the device with and without ZNG_ROCM_INFLATE_SUBBLOCK
(zng_rocm_inflate_large_ex_dev): 256 MiB of synth.silesia_like, the compressed bytes in HBM, one host thread,
the flags-0 and SUBBLOCK calls alternating, best of 5 after a warm-up of each.  Streams: CPython Z_FIXED level 6, CPython
level 6, this library's own level-6 stream (the bench's inflate leg).  Every timed call is checked byte for byte.

    python tools/inflate_subblock_rate.py [--mib 256] [--reps 5] [--out FILE.json]
"""
import argparse
import importlib
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import synth
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    inf = importlib.import_module("zlib-ng_amd.inflate")
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    plain = synth.silesia_like(a.mib << 20, seed=2026)
    want = torch.from_numpy(plain).cuda()
    streams = {}
    for name, strategy in (("cpython_fixed_l6", zlib.Z_FIXED), ("cpython_l6", zlib.Z_DEFAULT_STRATEGY)):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strategy)
        comp = c.compress(plain.tobytes()) + c.flush()
        streams[name] = torch.from_numpy(np.frombuffer(comp, dtype=np.uint8).copy()).cuda()
    comp, clen = dfl.deflate_dev(want, level=6)
    streams["own_l6"] = comp[:clen].contiguous()
    dst = torch.empty(plain.size + 64, dtype=torch.uint8, device="cuda")
    rows = {}
    for name, src in streams.items():
        best = {False: float("inf"), True: float("inf")}
        info = {}
        for rep in range(a.reps + 1):
            for sub in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st, n, used, parts = inf.inflate_large_dev(src, dst, subblock=sub)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                subparts = inf.inflate_large_last_subparts()
                placed = inf.inflate_large_last_substarts() if sub else 0
                assert (st, n, used) == (1, plain.size, int(src.numel())), (name, sub, st, n, used)
                assert torch.equal(dst[:n], want), (name, sub)
                if rep:
                    best[sub] = min(best[sub], dt)
                info[sub] = {"parts": parts, "subparts": subparts}
                if parts == 0:                                   # the sequential decoder did it: say why
                    info[sub]["fallback"] = zr.rocm.lib().zng_rocm_last_error().decode()
                if sub:
                    # sub-starts the dry parse placed, and the share a genuine decode landed on (parts on the chain)
                    info[sub].update({"substarts_placed": placed, "landed_share": round(subparts / placed, 4) if placed else None})
        rows[name] = {
            "compressed_bytes": int(src.numel()),
            "flags0": {"ms": round(best[False] * 1e3, 3), "GBps_out": round(plain.size / best[False] / 1e9, 2), **info[False]},
            "subblock": {"ms": round(best[True] * 1e3, 3), "GBps_out": round(plain.size / best[True] / 1e9, 2), **info[True]},
            "speedup": round(best[False] / best[True], 3),
        }
        print(name, json.dumps(rows[name]), flush=True)
    res = {"what": "zng_rocm_inflate_large_ex_dev, flags 0 vs ZNG_ROCM_INFLATE_SUBBLOCK", "plaintext_bytes": int(plain.size),
           "host_threads": 1, "timing": "best of %d after a warm-up, calls alternating" % a.reps, "streams": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
