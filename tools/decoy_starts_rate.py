"""What decoy block starts cost the large device inflaters: every stream of tests/decoy_cases.py -- valid streams whose stored
payload imitates block starts by the thousand -- through zng_rocm_inflate_large_dev (with and without SUBBLOCK),
zng_rocm_inflate_large_pieces_dev at 4 MiB pieces and the counting pass zng_rocm_uncompress_large_size_dev, each beside a
benign stored stream of the same size (the same carrier without a single decoy).  Per stream and call:
  parts        parts on the chain (0: the sequential decoder, or for the counting pass the one-wavefront kernel, did it)
  why          what the device path said when it declined (zng_rocm_last_error(); "" when it said nothing)
  passes, host_bytes   pieces: device passes, compressed bytes the sequential decoder took
  scratch_bytes        zng_rocm_workspace_bytes of a fresh HIP stream after the call
  wall_ms      the least of --repeats synchronous calls after one warm-up call, timed on the host from a synchronised device
Every call's status, lengths and bytes are checked.  Not part of bench.py.
    python tools/decoy_starts_rate.py [--repeats 3] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PIECE = 4 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import decoy_cases as dcy
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    inf = importlib.import_module("zlib-ng_amd.inflate")
    zr.init(0)
    lib = zr.rocm.lib()

    def dev(data):
        return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()

    tiny, tiny_dst = dev(b"\x03\x00"), torch.zeros(16, dtype=torch.uint8, device="cuda")

    def measure(comp, plain):
        src, want = dev(comp), dev(plain)
        row = {}
        for what in ("large", "large_subblock", "pieces", "size"):
            s = torch.cuda.Stream()
            dst = torch.zeros(len(plain) + 64, dtype=torch.uint8, device="cuda")
            with torch.cuda.stream(s):
                def call():
                    if what == "size":
                        return inf.uncompress_large_size_dev(0, src, stream=s) + (0, 0)
                    if what == "pieces":
                        return inf.inflate_large_pieces_dev(src, dst, piece_bytes=PIECE, stream=s)
                    return inf.inflate_large_dev(src, dst, stream=s, subblock=what == "large_subblock") + (0, 0)
                inf.inflate_large_dev(tiny, tiny_dst, stream=s)       # leaves "stream below 128 KiB" as the last error
                st, n, used, parts, passes, host = call()
                why = lib.zng_rocm_last_error().decode()
                assert (st, n, used) == (1, len(plain), len(comp)), (what, st, n, used, why)
                if what != "size":
                    s.synchronize()
                    assert torch.equal(dst[:n], want) and int(dst[n:].max()) == 0, what
                times = []
                for _ in range(args.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    s.synchronize()
                    times.append((time.perf_counter() - t0) * 1e3)
                row[what] = {"parts": parts, "why": "" if "below 128 KiB" in why else why, "scratch_bytes": inf.workspace_bytes(s),
                             "wall_ms": round(min(times), 3)}
                if what == "pieces":
                    row[what].update(passes=passes, host_bytes=host)
            lib.zng_rocm_stream_release(s.cuda_stream)
        return row

    res = {"piece_bytes": PIECE, "repeats": args.repeats, "streams": {}, "benign": {}}
    for name in dcy.ALL:
        s = dcy.get(name)
        size = len(s.comp)
        if str(size) not in res["benign"] and name != "text":          # (the text stream is mostly level-6 data: no stored twin)
            b = dcy.benign(size - 64)
            res["benign"][str(size)] = dict(measure(b.comp, b.plain), compressed_bytes=len(b.comp), blocks=len(b.genuine))
        res["streams"][name] = dict(measure(s.comp, s.plain), compressed_bytes=size, candidates=s.count, blocks=len(s.genuine),
                                    decoys={k: len(v) for k, v in s.kinds.items()}, retry_bound_bytes=s.retry_bound)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
