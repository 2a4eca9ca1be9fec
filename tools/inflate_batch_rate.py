"""Rates of a BATCH of large raw streams inflated in one set of launches per round (zng_rocm_inflate_large_streams_dev;
DESIGN 3.10 "Many large streams") against what the library offered for the same streams before: (a) a loop of
zng_rocm_inflate_large_ex_dev calls, (b) one zng_rocm_inflate_streams_dev call (one wavefront per stream) -- and beside
them the same plaintext as ONE stream through the one-pass call, the ceiling of the shape, and that one stream as a batch
of one job.

Legs: --mib (256) MiB of synth.silesia_like cut into 16, 64 and 256 equal streams, each written by CPython level 6 and by
this library's level 6; 16 streams of CPython Z_FIXED with ZNG_ROCM_INFLATE_SUBBLOCK; the 256-stream CPython leg with
SUBBLOCK as well.  One MI355X, one host thread, device-resident input and output.  Per leg the three ways alternate inside
one process: one untimed warm-up call each (allocates the scratch, checked byte for byte), then --reps (5) timings each, a
timing being enough consecutive calls for --window seconds of work; a leg's figure is its best timing, its spread max -
min of the per-call times.  With --parent-lib (a libzng_rocm.so built from the parent commit) the one-pass call of both
builds alternates on the three single streams: the part kernel's start search got a runtime bound.

    python tools/inflate_batch_rate.py [--mib 256] [--reps 5] [--window 0.25] [--legs 16,64,256] [--out FILE.json]
        [--parent-lib PATH] [--only LEG]       (--only: one batch leg alone, e.g. under rocprofv3 --kernel-trace --stats)
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
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--legs", default="16,64,256")
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    import torch
    import synth
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    inf = importlib.import_module("zlib-ng_amd.inflate")
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    rocm = zr.rocm
    lib = rocm.lib()
    total = a.mib << 20
    plain = synth.silesia_like(total, seed=2026)
    want = torch.from_numpy(plain).cuda()
    plain_bytes = plain.tobytes()
    pool = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))

    def cpython(data, strategy):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strategy)
        return c.compress(data) + c.flush()

    def write(writer, count):
        """`count` equal slices of the plaintext as raw streams in ONE device tensor: (tensor, offsets, lengths)"""
        each = total // count
        if writer == "own_l6":
            comps = []
            for i in range(count):
                c, n = dfl.deflate_dev(want[i * each:(i + 1) * each], level=6)
                comps.append(c[:n].clone())
            lens = [int(c.numel()) for c in comps]
        else:
            strategy = zlib.Z_FIXED if writer == "cpython_fixed" else zlib.Z_DEFAULT_STRATEGY
            raw = list(pool.map(lambda i: cpython(plain_bytes[i * each:(i + 1) * each], strategy), range(count)))
            comps = [torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() for b in raw]
            lens = [len(b) for b in raw]
        offs, at = [], 0
        for n in lens:
            offs.append(at)
            at += (n + 255) & ~255
        src = torch.zeros(at + 256, dtype=torch.uint8, device="cuda")
        for o, c in zip(offs, comps):
            src[o:o + c.numel()] = c
        return src, offs, lens

    dst = torch.empty(total + 4096, dtype=torch.uint8, device="cuda")

    def timings(ways, st):
        """ways: {name: callable}.  Warm-up (untimed, checked by the caller), then the ways in turn, --reps times."""
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

    def check(label):
        torch.cuda.synchronize()
        assert torch.equal(dst[:total], want), label
        dst.zero_()

    def leg(writer, count, sub, with_baselines=True):
        src, offs, lens = write(writer, count)
        each = total // count
        srcs = [src[o:o + n] for o, n in zip(offs, lens)]
        dsts = [dst[i * each:(i + 1) * each] for i in range(count)]
        flags = inf.SUBBLOCK if sub else 0
        row = {"streams": count, "writer": writer, "subblock": sub, "compressed_bytes": sum(lens), "output_bytes": total}
        st = torch.cuda.Stream()
        sp = C.c_void_p(st.cuda_stream)
        jobs = inf.large_jobs(srcs, dsts)
        jp = C.cast(jobs, C.c_void_p)

        def batch():
            rc = lib.zng_rocm_inflate_large_streams_dev(jp, count, 0, flags, sp)
            assert rc == 0, rc

        out_len, in_used = C.c_uint64(0), C.c_size_t(0)
        one = [(rocm._dev_ptr(s), int(s.numel()), None, 0, rocm._dev_ptr(d), int(d.numel()), C.byref(out_len), C.byref(in_used), flags, sp)
               for s, d in zip(srcs, dsts)]

        def loop():
            for args in one:
                rc = lib.zng_rocm_inflate_large_ex_dev(*args)
                assert rc == 1, rc

        many = inf.InflateDevBatch(src, offs, lens, dst, [i * each for i in range(count)], [each] * count)

        def wavefronts():
            many.run(stream=st)

        with torch.cuda.stream(st):
            ws0 = inf.workspace_bytes(st)
            batch()
            check((writer, count, "batch"))
            row["batch_workspace_bytes"] = inf.workspace_bytes(st) - ws0
            row["rounds"], row["part_launches"] = int(lib.zng_rocm_inflate_large_last_rounds()), int(lib.zng_rocm_inflate_large_last_part_launches())
            assert all(j.status == 1 and j.out_len == each for j in jobs[:count])
            row["jobs_on_device"] = sum(1 for j in jobs[:count] if j.parts > 0)
            row["device_share"] = round(row["jobs_on_device"] / count, 4)
            row["parts"] = sum(int(j.parts) for j in jobs[:count])
            ways = {"batch": batch}
            if with_baselines:
                loop()
                check((writer, count, "loop"))
                wavefronts()
                st.synchronize()
                assert all(r[:2] == (1, each) for r in many.rows()), (writer, count)
                check((writer, count, "streams_dev"))
                ways.update(loop_large_ex_dev=loop, streams_dev=wavefronts)
            row.update(timings(ways, st))
            batch()
            check((writer, count, "batch, after the timings"))
        lib.zng_rocm_stream_release(sp)
        if with_baselines:
            fast = max(("loop_large_ex_dev", "streams_dev"), key=lambda k: row[k]["gbps"])
            row["faster_baseline"] = fast
            # the bar: faster than the faster baseline by more than the spread of that baseline's own timings
            row["batch_beats_baselines"] = bool(row["batch"]["ms"] + row[fast]["spread_ms"] < row[fast]["ms"])
        return row

    results, ceilings = {}, {}
    plan = []
    for count in (int(v) for v in a.legs.split(",")):
        plan += [("%dx_cpython_l6" % count, "cpython_l6", count, False), ("%dx_own_l6" % count, "own_l6", count, False)]
        if count == 16:
            plan.append(("16x_cpython_fixed_subblock", "cpython_fixed", 16, True))
        if count == 256:
            plan.append(("256x_cpython_l6_subblock", "cpython_l6", 256, True))
    for name, writer, count, sub in plan:
        if a.only and name != a.only:
            continue
        results[name] = leg(writer, count, sub, with_baselines=not a.only)
        print(name, json.dumps(results[name]), flush=True)

    # the same plaintext as ONE stream: the one-pass call (the ceiling), the batch of one job, and the parent's one-pass call
    parent = None
    if a.parent_lib and not a.only:
        parent = C.CDLL(a.parent_lib, mode=os.RTLD_NOW | os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        parent.zng_rocm_init.restype, parent.zng_rocm_init.argtypes = C.c_int, [C.c_int]
        assert parent.zng_rocm_init(0) == 0
        parent.zng_rocm_inflate_large_ex_dev.restype = C.c_int
        parent.zng_rocm_inflate_large_ex_dev.argtypes = lib.zng_rocm_inflate_large_ex_dev.argtypes
    for writer, sub in (() if a.only else (("cpython_l6", False), ("own_l6", False), ("cpython_fixed", True))):
        src, offs, lens = write(writer, 1)
        s, flags = src[:lens[0]], inf.SUBBLOCK if sub else 0
        st = torch.cuda.Stream()
        sp = C.c_void_p(st.cuda_stream)
        out_len, in_used = C.c_uint64(0), C.c_size_t(0)
        args = (rocm._dev_ptr(s), lens[0], None, 0, rocm._dev_ptr(dst), total, C.byref(out_len), C.byref(in_used), flags, sp)
        jobs = inf.large_jobs([s], [dst[:total]])
        jp = C.cast(jobs, C.c_void_p)

        def one_pass():
            assert lib.zng_rocm_inflate_large_ex_dev(*args) == 1

        def batch_of_one():
            assert lib.zng_rocm_inflate_large_streams_dev(jp, 1, 0, flags, sp) == 0

        def parent_one_pass():
            assert parent.zng_rocm_inflate_large_ex_dev(*args) == 1

        ways = {"one_pass": one_pass, "batch_of_one": batch_of_one}
        if parent is not None:
            ways["parent_one_pass"] = parent_one_pass
        with torch.cuda.stream(st):
            for k, fn in ways.items():
                fn()
                check((writer, "single", k))
            assert jobs[0].status == 1 and jobs[0].parts > 0
            row = {"writer": writer, "subblock": sub, "compressed_bytes": lens[0], "output_bytes": total, "parts": int(jobs[0].parts)}
            row.update(timings(ways, st))
        lib.zng_rocm_stream_release(sp)
        # not slower than the one-pass call by more than that call's spread plus the 1.6 % of an extra instantiation
        row["batch_of_one_within_bar"] = bool(row["batch_of_one"]["ms"] <= row["one_pass"]["ms"] * 1.016 + row["one_pass"]["spread_ms"])
        if parent is not None:
            row["one_pass_vs_parent"] = round(row["parent_one_pass"]["ms"] / row["one_pass"]["ms"], 4)
            row["one_pass_not_slower_than_parent"] = bool(row["one_pass"]["ms"] <= row["parent_one_pass"]["ms"] + row["parent_one_pass"]["spread_ms"])
        ceilings[writer + ("_subblock" if sub else "")] = row
        print("single", writer, json.dumps(row), flush=True)

    out = {"tool": "tools/inflate_batch_rate.py", "device": torch.cuda.get_device_name(0), "mib": a.mib, "reps": a.reps,
           "window_s": a.window, "legs": results, "single_stream": ceilings}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
