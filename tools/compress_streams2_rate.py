"""What zng_rocm_compress_streams2_dev and zng_rocm_compress_members_dev cost: --streams (4096) device-resident
streams of 1 MiB -- the data of bench_configs.py's cfg5 -- as gzip at level 6, beside the raw engine underneath and beside the
loop a caller wrote before.  All in one process, alternating, one untimed warm-up each, then --reps (3) timings each; a figure
is the MEDIAN host time from the call to the end of the stream's work, with min and max beside it, and GB/s of plaintext:

  streams2      zng_rocm_compress_streams2_dev(2, 6, 0, ...): every member in its own bound-sized buffer
  members       zng_rocm_compress_members_dev(2, 6, 0, ...): one file
  raw           zng_rocm_deflate_streams_dev at level 6: the same jobs, raw deflate, no check values (the floor)
  loop          zng_rocm_compress2_dev(level 6, gzip) per stream, timed over the first --prefix (256) streams and scaled to all
                ("extrapolated": true)
  level1        zng_rocm_compress_streams_dev(2, ...): the level-1 class with its padded gzip wrapper, for scale

and the kernel split of one streams2 call and one raw call from the library's own event pairs (zng_rocm_trace_*): the check
pass, the matcher (lz_rows_kernel) and the frame kernel; the raw call's matcher.  What streams2 adds to raw, beside the check
pass, is reported as "streams2_minus_raw_minus_check_ms".  Nothing is gated.

    python tools/compress_streams2_rate.py [--streams 4096] [--reps 3] [--out FILE.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MiB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prefix", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compress_streams2_rate_v1.json"))
    a = ap.parse_args()
    import torch
    import synth
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    lib = zr.rocm.lib()
    ns, each = a.streams, MiB
    prefix = min(a.prefix, ns)
    base = synth.silesia_like(min(96, ns) * MiB, seed=0x5EED0005, seg_bytes=MiB)         # cfg5: 96 distinct 1 MiB slices
    host = np.concatenate([base] * ((ns * each + base.size - 1) // base.size))[:ns * each]
    src = torch.from_numpy(host).cuda()
    offs = [i * each for i in range(ns)]
    views = [src[o:o + each] for o in offs]
    bound = dfl.compress_streams2_bound(each, 2)
    slot = (bound + 15) & ~15
    outs = torch.empty(ns * slot, dtype=torch.uint8, device="cuda")
    jobs = dfl.stream_jobs(views, [outs[i * slot:i * slot + bound] for i in range(ns)])
    results = torch.zeros((ns, 2), dtype=torch.int32, device="cuda")
    file_dst = torch.empty(ns * slot, dtype=torch.uint8, device="cuda")
    file_jobs = dfl.stream_jobs(views)
    offsets = torch.zeros(ns + 1, dtype=torch.int64, device="cuda")
    checks = torch.zeros(ns, dtype=torch.int32, device="cuda")
    raw = dfl.StreamsBatch(src, offs, [each] * ns)
    quick = dfl.WrappedBatch(src, offs, [each] * ns, 2)
    loop_dst = torch.empty(bound, dtype=torch.uint8, device="cuda")
    loop_len = C.c_size_t(0)

    def streams2():
        assert dfl.compress_streams2_dev(jobs, ns, results, 2, 6) == 0

    def members():
        assert dfl.compress_members_dev(file_jobs, ns, file_dst, offsets, 2, 6, checks=checks) == 0

    def loop():
        for i in range(prefix):
            loop_len.value = bound
            assert lib.zng_rocm_compress2_dev(loop_dst.data_ptr(), C.byref(loop_len), views[i].data_ptr(), each, 6, 2, None) == 0

    ways = {"streams2": streams2, "members": members, "raw": lambda: raw.run(level=6), "loop": loop, "level1": quick.run}
    per = {k: [] for k in ways}
    for fn in ways.values():                                  # warm-up: allocates the scratch
        fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            per[k].append(time.perf_counter() - t0)
    total = ns * each

    def row(v, scale=1.0):
        med = statistics.median(v) * scale
        return dict(ms=round(med * 1e3, 3), min_ms=round(min(v) * scale * 1e3, 3), max_ms=round(max(v) * scale * 1e3, 3),
                    input_GBps=round(total / med / 1e9, 3))
    out = {"tool": "tools/compress_streams2_rate.py", "device": torch.cuda.get_device_name(0), "streams": ns, "stream_bytes": each,
           "reps": a.reps, "figure": "median of reps, host time from the call to the end of the stream's work; GB/s of plaintext"}
    for k in ways:
        out[k] = row(per[k], ns / prefix if k == "loop" else 1.0)
    out["loop"].update(extrapolated=prefix < ns, streams_timed=prefix)

    # the kernel split, from the event pairs attached to the dispatches
    zr.trace_begin(8)
    streams2()
    split = zr.trace_end(8)
    zr.trace_begin(8)
    raw.run(level=6)
    split_raw = zr.trace_end(8)
    assert len(split) == 3 and len(split_raw) == 1, (split, split_raw)
    out["kernels_streams2_ms"] = {"check_pass": round(split[0], 3), "lz_rows_kernel": round(split[1], 3), "cs_frame_kernel": round(split[2], 3)}
    out["kernels_raw_ms"] = {"lz_rows_kernel": round(split_raw[0], 3)}
    out["streams2_minus_raw_ms"] = round(out["streams2"]["ms"] - out["raw"]["ms"], 3)
    out["streams2_minus_raw_minus_check_ms"] = round(out["streams2"]["ms"] - out["raw"]["ms"] - split[0], 3)

    # what was timed is right: sizes, a sample of members through CPython, the file the concatenation of the members
    streams2()
    members()
    torch.cuda.synchronize()
    res = results.cpu().numpy().astype(np.int64) & 0xffffffff
    off = offsets.cpu().tolist()
    assert off[0] == 0 and all(off[i + 1] - off[i] == int(res[i, 0]) for i in range(ns))
    for i in (0, 1, 5, 17, ns - 1):
        plain = host[i * each:(i + 1) * each].tobytes()
        member = outs[i * slot:i * slot + int(res[i, 0])].cpu().numpy().tobytes()
        assert zlib.decompress(member, 31) == plain and int(res[i, 1]) == zlib.crc32(plain)
        assert file_dst[off[i]:off[i + 1]].cpu().numpy().tobytes() == member
        assert raw.compressed(i) == member[10:-8]
    out["ratio"] = round(total / off[ns], 3)
    out["level1_ratio"] = round(total / int((quick.results.cpu().numpy().astype(np.int64)[:, 0]).sum()), 3)
    print(json.dumps(out, indent=1), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
