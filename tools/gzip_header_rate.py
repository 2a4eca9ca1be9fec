"""What the gzip header calls cost, and that the calls without headers cost what they did: --streams (4096)
device-resident streams of 1 MiB -- the data of bench_configs.py's cfg5 -- as one gzip file at level 6.

  1  zng_rocm_compress_members_dev(2, 6, 0, ...) of THIS build against another build of the library (--parent-lib: the
     libzng_rocm.so of the parent commit).  Each library is measured in processes of its own, alternating parent, build, parent,
     build; a figure is the median of --reps (5) timed calls behind one warm-up.  The allowed margin is the parent's own
     run-to-run spread: |median of its first run - median of its second|.  "no_heads_within_parent_spread" says whether the
     build's slower run is within that margin of the parent's slower run.
  2  zng_rocm_compress_members_header_dev with a 40-byte header per member (FNAME of 27 bytes and FHCRC); no threshold
  3  zng_rocm_gzip_headers_dev over that file's members, milliseconds per call; no threshold

    python tools/gzip_header_rate.py --parent-lib PATH/libzng_rocm.so [--streams 4096] [--reps 5] [--out FILE.json]

A child process (--child LIB) loads the library it is given with ctypes alone, so that a library from before the header calls
can be measured too, and prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
MiB = 1 << 20
OWN_LIB = os.path.join(ROOT, "zlib-ng_amd", "lib", "libzng_rocm.so")


class StreamJob(C.Structure):
    _fields_ = [("in_ptr", C.c_void_p), ("out_ptr", C.c_void_p), ("in_len", C.c_uint32), ("out_cap", C.c_uint32),
                ("dict_len", C.c_uint32), ("flags", C.c_uint32)]


class GzipHeader(C.Structure):
    _fields_ = [("time", C.c_uint32), ("os", C.c_uint32), ("text", C.c_uint32), ("hcrc", C.c_uint32), ("extra", C.c_void_p),
                ("name", C.c_void_p), ("comment", C.c_void_p), ("extra_len", C.c_uint32), ("reserved", C.c_uint32)]


class GzipMember(C.Structure):
    _fields_ = [("src_off", C.c_uint64), ("src_len", C.c_uint64), ("dst_off", C.c_uint64), ("out_len", C.c_uint64),
                ("crc", C.c_uint32), ("bgzf", C.c_uint32)]


def timed(fn, sync, reps):
    fn()                                                      # warm-up: allocates the scratch
    sync()
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def figure(ms, total):
    med = statistics.median(ms)
    return dict(ms=round(med, 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), input_GBps=round(total / med / 1e6, 3))


def child(a):
    import torch          # (first: the library binds to the HIP runtime torch brought)
    import synth
    lib = C.CDLL(a.child)
    lib.zng_rocm_init.argtypes = [C.c_int]
    assert lib.zng_rocm_init(0) == 0
    ns, each = a.streams, MiB
    base = synth.silesia_like(min(96, ns) * MiB, seed=0x5EED0005, seg_bytes=MiB)          # cfg5: 96 distinct 1 MiB slices
    host = np.concatenate([base] * ((ns * each + base.size - 1) // base.size))[:ns * each]
    src = torch.from_numpy(host).cuda()
    jobs = (StreamJob * ns)()
    for i in range(ns):
        jobs[i].in_ptr, jobs[i].in_len = src.data_ptr() + i * each, each
    dst = torch.empty(ns * (each + 4096), dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(ns + 1, dtype=torch.int64, device="cuda")
    checks = torch.zeros(ns, dtype=torch.int32, device="cuda")
    members_args = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.zng_rocm_compress_members_dev.argtypes = members_args
    total = ns * each
    out = {"lib": a.child, "device": torch.cuda.get_device_name(0)}

    def members():
        assert lib.zng_rocm_compress_members_dev(2, 6, 0, jobs, ns, dst.data_ptr(), dst.numel(), 0, offsets.data_ptr(), checks.data_ptr(),
                                                 None) == 0
    out["members"] = figure(timed(members, torch.cuda.synchronize, a.reps), total)
    off = offsets.cpu().tolist()
    assert zlib.decompress(dst[off[5]:off[6]].cpu().numpy().tobytes(), 31) == host[5 * each:6 * each].tobytes()
    out["file_bytes"] = off[ns]
    if a.headers:
        names = [C.create_string_buffer(b"member-%06d-of-%06d.bin" % (i, ns)) for i in range(ns)]
        heads = (GzipHeader * ns)()
        for i in range(ns):
            heads[i].time, heads[i].os, heads[i].hcrc, heads[i].name = 1700000000 + i, 3, 1, C.addressof(names[i])
        lib.zng_rocm_gzip_header_bytes.restype = C.c_size_t
        lib.zng_rocm_gzip_header_bytes.argtypes = [C.c_void_p]
        assert all(lib.zng_rocm_gzip_header_bytes(C.byref(heads, i * C.sizeof(GzipHeader))) == 40 for i in (0, ns - 1))
        lib.zng_rocm_compress_members_header_dev.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                             C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]

        def with_heads():
            assert lib.zng_rocm_compress_members_header_dev(6, 0, 15, jobs, heads, ns, dst.data_ptr(), dst.numel(), 0, offsets.data_ptr(),
                                                            checks.data_ptr(), None) == 0
        out["members_header_40"] = figure(timed(with_heads, torch.cuda.synchronize, a.reps), total)
        off2 = offsets.cpu().tolist()
        assert off2[ns] == off[ns] + 30 * ns
        member = dst[off2[7]:off2[8]].cpu().numpy().tobytes()
        assert zlib.decompress(member, 31) == host[7 * each:8 * each].tobytes() and member[10:37] == names[7].raw[:27]
        table = (GzipMember * ns)()
        for i in range(ns):
            table[i].src_off, table[i].src_len = off2[i], off2[i + 1] - off2[i]
        rows = C.create_string_buffer(96 * ns)
        text = C.create_string_buffer(32 * ns)
        need = C.c_size_t(0)
        lib.zng_rocm_gzip_headers_dev.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                                  C.POINTER(C.c_size_t), C.c_void_p]

        def read_back():
            assert lib.zng_rocm_gzip_headers_dev(dst.data_ptr(), off2[ns], table, ns, rows, text, 32 * ns, C.byref(need), None) == 0
        ms = timed(read_back, lambda: None, a.reps)               # the call is synchronous
        assert need.value == 28 * ns and text.raw[28 * 7:28 * 8] == names[7].raw[:28]
        out["gzip_headers_dev"] = dict(members=ns, ms_per_call=round(statistics.median(ms), 3), min_ms=round(min(ms), 3),
                                       max_ms=round(max(ms), 3))
    print("RESULT " + json.dumps(out), flush=True)
    return 0


def run_child(a, lib, headers):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", lib, "--streams", str(a.streams), "--reps", str(a.reps)]
    out = subprocess.run(cmd + (["--headers"] if headers else []), capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError("child for %s failed (%d): %s" % (lib, out.returncode, out.stderr[-2000:]))
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print("# %s: members %.3f ms" % (lib, res["members"]["ms"]), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--headers", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gzip_header_rate_v1.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_lib:
        ap.error("--parent-lib: the libzng_rocm.so of the parent commit")
    runs = [("parent", run_child(a, a.parent_lib, False)), ("build", run_child(a, OWN_LIB, True)),
            ("parent", run_child(a, a.parent_lib, False)), ("build", run_child(a, OWN_LIB, True))]
    parent = [r["members"] for k, r in runs if k == "parent"]
    build = [r["members"] for k, r in runs if k == "build"]
    spread = abs(parent[0]["ms"] - parent[1]["ms"])
    out = {"tool": "tools/gzip_header_rate.py", "device": runs[0][1]["device"], "streams": a.streams, "stream_bytes": MiB, "reps": a.reps,
           "figure": "median of reps behind one warm-up, host time from the call to the end of the stream's work; GB/s of plaintext; "
                     "order of the processes: parent, build, parent, build",
           "members_no_heads": {"parent_runs": parent, "build_runs": build, "parent_spread_ms": round(spread, 3),
                                "build_slower_minus_parent_slower_ms": round(max(b["ms"] for b in build) - max(p["ms"] for p in parent), 3)},
           "members_header_40": [r["members_header_40"] for k, r in runs if k == "build"],
           "gzip_headers_dev": [r["gzip_headers_dev"] for k, r in runs if k == "build"],
           "file_bytes": runs[1][1]["file_bytes"]}
    m = out["members_no_heads"]
    m["no_heads_within_parent_spread"] = m["build_slower_minus_parent_slower_ms"] <= spread
    print(json.dumps(out, indent=1), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
