"""Rates of ONE large raw stream inflated piece by piece (zng_rocm_inflate_large_pieces_dev) against the
one-pass call (zng_rocm_inflate_large_ex_dev), and the peak device scratch each leaves on a fresh HIP stream.
cfg3 streams: 256 MiB of synth.silesia_like as this library's level-6 stream, CPython level 6, and CPython Z_FIXED (with
ZNG_ROCM_INFLATE_SUBBLOCK); 32 MiB and 64 MiB pieces.  Past 2 GiB: sync-flushed copies of a 32 MiB segment (every other MiB
incompressible) up to 2^31 + 64 MiB of input, 64 MiB pieces (the one-pass call does not take it).  Best of --reps after a
warm-up; every timed call is checked byte for byte.

    python tools/inflate_pieces_rate.py [--mib 256] [--reps 3] [--out FILE.json]
        [--streams own_l6,cpython_l6,...] [--legs one_pass,pieces_32mib,pieces_64mib] [--no-tiled]
(one leg of one stream per run under rocprofv3 --kernel-trace --stats gives that leg's kernel time per call)
"""
import argparse
import ctypes as C
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", default="own_l6,cpython_l6,cpython_fixed_l6_subblock")
    ap.add_argument("--legs", default="one_pass,pieces_32mib,pieces_64mib")
    ap.add_argument("--no-tiled", action="store_true")
    a = ap.parse_args()
    names, legs = a.streams.split(","), a.legs.split(",")
    import torch
    import synth
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    inf = importlib.import_module("zlib-ng_amd.inflate")
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    lib = zr.rocm.lib()
    plain = synth.silesia_like(a.mib << 20, seed=2026)
    want = torch.from_numpy(plain).cuda()
    streams = {}
    if "own_l6" in names:
        comp, clen = dfl.deflate_dev(want, level=6)
        streams["own_l6"] = (comp[:clen].contiguous(), False)
    for name, strategy, sub in (("cpython_l6", zlib.Z_DEFAULT_STRATEGY, False), ("cpython_fixed_l6_subblock", zlib.Z_FIXED, True)):
        if name not in names:
            continue
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strategy)
        b = c.compress(plain.tobytes()) + c.flush()
        streams[name] = (torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda(), sub)
    dst = torch.empty(plain.size + 4096, dtype=torch.uint8, device="cuda")

    def timed(fn, st):
        best = None
        for r in range(a.reps + 1):
            st.synchronize()
            t0 = time.perf_counter()
            res = fn()
            st.synchronize()
            dt = time.perf_counter() - t0
            if r and (best is None or dt < best):
                best = dt
        return best, res

    rows = {}
    for name, (src, sub) in streams.items():
        row = {"compressed_bytes": int(src.numel()), "output_bytes": int(plain.size)}
        for label, piece in (("one_pass", None), ("pieces_32mib", 32 << 20), ("pieces_64mib", 64 << 20)):
            if label not in legs:
                continue
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                if piece is None:
                    dt, res = timed(lambda: inf.inflate_large_dev(src, dst, stream=st, subblock=sub), st)
                    extra = {}
                else:
                    dt, res = timed(lambda: inf.inflate_large_pieces_dev(src, dst, piece_bytes=piece, stream=st, subblock=sub), st)
                    extra = {"passes": res[4], "host_bytes": res[5]}
                assert res[:3] == (1, plain.size, src.numel()), (name, label, res)
                assert torch.equal(dst[:plain.size], want), (name, label)
            ws = inf.workspace_bytes(st)
            lib.zng_rocm_stream_release(C.c_void_p(st.cuda_stream))
            row[label] = dict(ms=round(dt * 1e3, 3), gbps=round(plain.size / dt / 1e9, 2), parts=res[3], workspace_bytes=ws, **extra)
        if "one_pass" in row and "pieces_64mib" in row:
            row["ratio_64mib_vs_one_pass"] = round(row["pieces_64mib"]["gbps"] / row["one_pass"]["gbps"], 3)
        rows[name] = row
        print(name, json.dumps(row))
    del dst, streams
    torch.cuda.empty_cache()
    out = {"tool": "tools/inflate_pieces_rate.py", "device": torch.cuda.get_device_name(0), "mib": a.mib, "reps": a.reps,
           "results": rows}
    if a.no_tiled:
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        return

    # past 2 GiB of input
    seg_plain = synth.silesia_like(32 << 20, seed=0x2A6B, seg_bytes=1 << 20)
    rnd = np.random.default_rng(0x2A6C).integers(0, 256, size=seg_plain.size, dtype=np.uint8)
    seg_plain = np.where((np.arange(seg_plain.size) >> 20) % 2 == 1, rnd, seg_plain).astype(np.uint8)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    seg = c.compress(seg_plain.tobytes()) + c.flush(zlib.Z_SYNC_FLUSH)
    tiles = -(-((1 << 31) + (64 << 20)) // len(seg))
    total, out_total = tiles * len(seg) + 2, tiles * seg_plain.size
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        seg_dev = torch.from_numpy(np.frombuffer(seg, dtype=np.uint8).copy()).cuda()
        plain_dev = torch.from_numpy(seg_plain).cuda()
        src = torch.empty(total, dtype=torch.uint8, device="cuda")
        for i in range(tiles):
            src[i * len(seg):(i + 1) * len(seg)] = seg_dev
        src[tiles * len(seg):] = torch.tensor([3, 0], dtype=torch.uint8, device="cuda")
        dst = torch.empty(out_total, dtype=torch.uint8, device="cuda")
        dt, res = timed(lambda: inf.inflate_large_pieces_dev(src, dst, piece_bytes=64 << 20, stream=st), st)
        assert res[:3] == (1, out_total, total) and res[5] == 0, res
        assert all(torch.equal(dst[i * seg_plain.size:(i + 1) * seg_plain.size], plain_dev) for i in range(tiles))
    ws = inf.workspace_bytes(st)
    lib.zng_rocm_stream_release(C.c_void_p(st.cuda_stream))
    rows["tiled_past_2gib"] = dict(compressed_bytes=total, output_bytes=out_total, piece_bytes=64 << 20, ms=round(dt * 1e3, 2),
                                   gbps=round(out_total / dt / 1e9, 2), parts=res[3], passes=res[4], host_bytes=res[5],
                                   workspace_bytes=ws)
    print("tiled_past_2gib", json.dumps(rows["tiled_past_2gib"]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
