"""Rates of the sizing pass and of the packed decode for many small device-resident streams whose lengths nobody handed over
(zng_rocm_inflate_sizes_dev, zng_rocm_uncompress_packed_dev) against the decode with the true sizes:

  (a) sizes     zng_rocm_inflate_sizes_dev alone
  (b) decode    zng_rocm_uncompress_streams_dev with the true sizes, in the same run -- the existing decode, the
                reference for both other figures
  (c) packed    zng_rocm_uncompress_packed_dev (sizes, places, decode, verification)

Legs: --streams (4096) x --each (1 MiB) of synth.silesia_like (a base of --base-mib repeated), once as the level-1 class's own
streams and once as CPython level-6 streams, in --format (0 raw, 1 zlib, 2 gzip).  One MI355X, one host thread, device-resident
input and output.  Per leg the three ways alternate inside one process: one untimed warm-up call each (allocates the scratch;
rows, offsets and bytes checked), then --reps (5) timings each, a timing being enough consecutive calls for --window seconds
of work; a way's figure is its best timing, its spread max - min of the per-call times.  GB/s are plaintext bytes per second.

    python tools/inflate_sizes_rate.py [--streams 4096] [--each 1048576] [--reps 5] [--window 0.25] [--format 0] [--out FILE.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--each", type=int, default=1 << 20)
    ap.add_argument("--base-mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--format", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import synth
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    inf = importlib.import_module("zlib-ng_amd.inflate")
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    lib = zr.rocm.lib()
    n, each, fmt = a.streams, a.each, a.format
    total = n * each
    base_streams = min(n, max(1, (a.base_mib << 20) // each))
    assert n % base_streams == 0
    base = synth.silesia_like(base_streams * each, seed=33)
    want = torch.from_numpy(base).cuda().repeat(n // base_streams)
    pool = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))

    def cpython(i):
        data = base[i * each:(i + 1) * each].tobytes()
        c = zlib.compressobj(6, zlib.DEFLATED, {0: -15, 1: 15, 2: 31}[fmt])
        return c.compress(data) + c.flush()

    def write(writer):
        """the n members in ONE device tensor: (tensor, offsets, lengths)"""
        if writer == "own_l1":
            if fmt == 0:
                b = dfl.QuickBatch(want, [i * each for i in range(n)], [each] * n)
            else:
                b = dfl.WrappedBatch(want, [i * each for i in range(n)], [each] * n, fmt)
            b.run()
            torch.cuda.synchronize()
            return b.dst, list(b.out_off), [int(v) for v in b.results.cpu()[:, 0]]
        blobs = list(pool.map(cpython, range(base_streams)))
        offs, at = [], 0
        for b in blobs:
            offs.append(at)
            at += (len(b) + 255) & ~255
        img = np.zeros(at, dtype=np.uint8)
        for o, b in zip(offs, blobs):
            img[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
        reps = n // base_streams
        src = torch.from_numpy(img).cuda().repeat(reps)
        return src, [r * at + o for r in range(reps) for o in offs], [len(b) for b in blobs] * reps

    dst = torch.empty(total + 4096, dtype=torch.uint8, device="cuda")

    def timings(ways, st):
        calls, per = {}, {k: [] for k in ways}
        for k, fn in ways.items():                        # how many calls make a window
            st.synchronize()
            t0 = time.perf_counter()
            fn()
            st.synchronize()
            calls[k] = max(1, int(a.window / max(time.perf_counter() - t0, 1e-6)) + 1)
        for _ in range(a.reps):
            for k, fn in ways.items():
                st.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls[k]):
                    fn()
                st.synchronize()
                per[k].append((time.perf_counter() - t0) / calls[k])
        out = {}
        for k, v in per.items():
            out[k] = dict(ms=round(min(v) * 1e3, 3), gbps=round(total / min(v) / 1e9, 2), spread_ms=round((max(v) - min(v)) * 1e3, 3),
                          gbps_min=round(total / max(v) / 1e9, 2), calls_per_timing=calls[k], timings_ms=[round(x * 1e3, 3) for x in v])
        return out

    def leg(writer):
        src, offs, lens = write(writer)
        row = {"writer": writer, "streams": n, "format": fmt, "compressed_bytes": sum(lens), "output_bytes": total}
        st = torch.cuda.Stream()
        true = inf.InflateDevBatch(src, offs, lens, dst, [i * each for i in range(n)], [each] * n)
        sized = inf.InflateDevBatch(src, offs, lens, dst, [0] * n, [0] * n)
        jobs = inf.packed_jobs(src, offs, lens)
        offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        res = torch.zeros((n, 4), dtype=torch.int32, device="cuda")

        def sizes():
            sized.run_sizes(fmt, stream=st)

        def decode():
            true.run_wrapped(fmt, stream=st)

        def packed():
            assert inf.uncompress_packed_dev(fmt, jobs, n, dst[:total], offsets, res, 1, None, st) == 0

        with torch.cuda.stream(st):
            sizes()
            st.synchronize()
            r = sized.results.cpu()
            assert bool((r[:, 2] == 1).all()) and bool((r[:, 0] == each).all()) and r[:, 1].tolist() == lens, writer
            dst.zero_()
            decode()
            st.synchronize()
            assert torch.equal(true.results.cpu(), r) and torch.equal(dst[:total], want), writer
            dst.zero_()
            packed()
            st.synchronize()
            assert torch.equal(res.cpu(), r) and torch.equal(dst[:total], want), writer
            assert offsets.cpu().tolist() == [i * each for i in range(n + 1)]
            row.update(timings({"sizes": sizes, "decode": decode, "packed": packed}, st))
        lib.zng_rocm_stream_release(C.c_void_p(st.cuda_stream))
        row["sizes_over_decode"] = round(row["sizes"]["ms"] / row["decode"]["ms"], 4)
        row["packed_over_sizes_plus_decode"] = round(row["packed"]["ms"] / (row["sizes"]["ms"] + row["decode"]["ms"]), 4)
        return row

    results = {}
    for writer in ("own_l1", "cpython_l6"):
        results[writer] = leg(writer)
        print(writer, json.dumps(results[writer]), flush=True)
    out = {"tool": "tools/inflate_sizes_rate.py", "device": torch.cuda.get_device_name(0), "streams": n, "each": each, "format": fmt,
           "reps": a.reps, "window_s": a.window, "legs": results}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
