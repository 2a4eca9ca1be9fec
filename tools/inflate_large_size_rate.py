"""Time and scratch of the sizing call for large device-resident streams (zng_rocm_uncompress_large_size_dev) beside the
decode of the same streams in the same run (zng_rocm_inflate_large_dev): 256 MiB of the synthetic mix as a CPython level-6
raw stream and as this library's own level-6 stream.  Per stream and call:
  wall_ms      --repeats synchronous calls after one warm-up call, each timed on the host from a synchronised device
  kernel_ms    the launches the library's trace sees in one more call (zng_rocm_trace_begin / _end): for the sizing call the
               counting part kernel alone, for the decode its part kernel (a second entry: the rerun of parts above 64 : 1)
  grown_bytes  what zng_rocm_workspace_bytes of a fresh HIP stream grew by over the first call
The decode's spread (max - min of its repeats) is what the sizing call's time is held against: it does strictly less, so it
must not take longer beyond that spread.  Not part of bench.py.
    python tools/inflate_large_size_rate.py [--mib 256] [--repeats 5] [--out FILE]"""
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


def timed(torch, call, repeats):
    call()                                                # warm-up: first allocations stay out of the figures
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        out.append(round((time.perf_counter() - t0) * 1e3, 3))
    return out


def traced(zr, call):
    zr.rocm.trace_begin(16)
    call()
    return [round(ms, 3) for ms in zr.rocm.trace_end(16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import synth
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    inf = importlib.import_module("zlib-ng_amd.inflate")
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    zr.init(0)
    plain = synth.silesia_like(args.mib << 20, seed=2028)
    plain_dev = torch.from_numpy(plain).cuda()
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    cpython = c.compress(plain.tobytes()) + c.flush()
    own, n = dfl.deflate_dev(plain_dev, level=6)
    streams = {"cpython6": torch.from_numpy(np.frombuffer(cpython, dtype=np.uint8).copy()).cuda(), "own6": own[:n].clone()}
    del own
    dst = torch.zeros(plain.size, dtype=torch.uint8, device="cuda")
    res = {"plain_bytes": int(plain.size), "repeats": args.repeats, "streams": {}}
    for name, src in streams.items():
        row = {"compressed_bytes": int(src.numel())}
        for what in ("size", "decode"):
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                if what == "size":
                    call = lambda: inf.uncompress_large_size_dev(0, src, stream=s)         # noqa: E731
                else:
                    call = lambda: inf.inflate_large_dev(src, dst, stream=s)               # noqa: E731
                before = inf.workspace_bytes(s)
                st, n_out, used, parts = call()
                assert (st, n_out, used) == (1, plain.size, src.numel()) and parts >= 4, (what, st, n_out, used, parts)
                row[what] = {"parts": parts, "grown_bytes": inf.workspace_bytes(s) - before, "wall_ms": timed(torch, call, args.repeats),
                             "kernel_ms": traced(zr, call)}
            if what == "decode":
                assert torch.equal(dst, plain_dev)
            zr.rocm.lib().zng_rocm_stream_release(s.cuda_stream)
        d, z = row["decode"]["wall_ms"], row["size"]["wall_ms"]
        row["decode_spread_ms"] = round(max(d) - min(d), 3)
        row["size_over_decode"] = round(min(z) / min(d), 3)
        res["streams"][name] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
