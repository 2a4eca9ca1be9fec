"""What zng_rocm_bgzf_compress_dev costs on top of the engines it frames: the whole call -- CRC-32 pass, engine,
member scan, frame / pack kernel -- against the engine alone over the same 65280-byte pieces, in one process.

Two device-resident inputs of --mib (1024) MiB:

  text      tests/golden/ref_fixtures/data_lcet10.txt repeated
  mix       the same text with every fourth MiB replaced by uniform random bytes (pieces the stored fallback takes)

and four ways over each, alternating, one untimed warm-up each (it allocates the scratch), then --reps (5) timings each; a
figure is the MEDIAN timing, with min and max beside it, and GB/s of plaintext:

  bgzf6     zng_rocm_bgzf_compress_dev(6, ...)
  streams6  zng_rocm_deflate_streams_dev(6, ...) alone: one job per piece, every job with its own bound-sized buffer
  bgzfq     zng_rocm_bgzf_compress_dev(1, ..., ZNG_ROCM_BGZF_QUICK)
  quick     zng_rocm_deflate_quick_dev alone, the same jobs

Recorded per input: framing_share_6 = (bgzf6 - streams6) / streams6 and framing_share_quick likewise -- what the CRC pass, the
scan and the frame / pack kernel add to the deflate time (negative: the call is cheaper than the engine's own per-stream
packing) -- the file sizes, and the stored members.  Each file is decoded once by CPython (the first and the last 64 members)
and compared with the plaintext.  --only WAY runs a single way on `text` (a profiler run) and leaves the report alone.

    python tools/bgzf_rate.py [--mib 1024] [--reps 5] [--only bgzf6|streams6|bgzfq|quick] [--out FILE.json]
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
PIECE = 65280
WAYS = ("bgzf6", "streams6", "bgzfq", "quick")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, choices=WAYS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_rate_v1.json"))
    a = ap.parse_args()
    assert a.reps >= 1 and a.mib >= 1
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    inf = importlib.import_module("zlib-ng_amd.inflate")
    rocm = zr.rocm
    lib = rocm.lib()
    st = torch.cuda.Stream()
    sp = C.c_void_p(st.cuda_stream)
    n = a.mib * MiB
    np_all = -(-n // PIECE)
    with open(os.path.join(ROOT, "tests", "golden", "ref_fixtures", "data_lcet10.txt"), "rb") as f:
        lcet = np.frombuffer(f.read(), dtype=np.uint8)

    def make(name):
        unit = torch.from_numpy(lcet.copy()).cuda()
        src = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        for at in range(0, n, unit.numel()):
            k = min(unit.numel(), n - at)
            src[at:at + k] = unit[:k]
        if name == "mix":
            noise = torch.from_numpy(np.frombuffer(np.random.default_rng(0).bytes(MiB), dtype=np.uint8).copy()).cuda()
            for at in range(3 * MiB, n - MiB + 1, 4 * MiB):
                src[at:at + MiB] = noise
        return src

    def timings(ways):
        per = {k: [] for k in ways}
        for fn in ways.values():                          # warm-up: allocates the scratch
            fn()
        st.synchronize()
        for _ in range(a.reps):
            for k, fn in ways.items():
                st.synchronize()
                t0 = time.perf_counter()
                fn()
                st.synchronize()
                per[k].append(time.perf_counter() - t0)
        return {k: dict(ms=round(statistics.median(v) * 1e3, 4), min_ms=round(min(v) * 1e3, 4), max_ms=round(max(v) * 1e3, 4),
                        gbps=round(n / statistics.median(v) / 1e9, 3)) for k, v in per.items()}

    def leg(name, only=None):
        src = make(name)
        cap = dfl.bgzf_bound(n, 0)
        dst = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
        out_len, nmembers = C.c_uint64(0), C.c_size_t(0)
        files = {}

        def bgzf(level, flags, key):
            def run():
                assert lib.zng_rocm_bgzf_compress_dev(level, rocm._dev_ptr(src), n, 0, rocm._dev_ptr(dst), cap, C.byref(out_len), None, 0,
                                                      C.byref(nmembers), 0, flags, sp) == 0
                files[key] = (out_len.value, nmembers.value, int(lib.zng_rocm_bgzf_last_stored()), int(lib.zng_rocm_bgzf_last_rounds()))
            return run

        # the engines alone: one job per piece, bound-sized buffers one behind the other
        def jobs_for(bound):
            buf = torch.empty(np_all * bound + 64, dtype=torch.uint8, device="cuda")
            jobs = (dfl.StreamJob * np_all)()
            base_in, base_out = src.data_ptr(), buf.data_ptr()
            for i in range(np_all):
                jobs[i].in_ptr, jobs[i].out_ptr = base_in + i * PIECE, base_out + i * bound
                jobs[i].in_len, jobs[i].out_cap, jobs[i].dict_len, jobs[i].flags = min(PIECE, n - i * PIECE), bound, 0, 0
            return buf, jobs

        ways = {}
        if only in (None, "bgzf6"):
            ways["bgzf6"] = bgzf(6, 0, "bgzf6")
        if only in (None, "streams6"):
            bound6 = (int(lib.zng_rocm_deflate_bound(PIECE)) + 15) & ~15
            buf6, jobs6 = jobs_for(bound6)
            lens6 = (C.c_size_t * np_all)()

            def streams6():
                assert lib.zng_rocm_deflate_streams_dev(6, C.byref(jobs6), np_all, lens6, sp) == 0
            ways["streams6"] = streams6
        if only in (None, "bgzfq"):
            ways["bgzfq"] = bgzf(1, dfl.BGZF_QUICK, "bgzfq")
        if only in (None, "quick"):
            boundq = int(lib.zng_rocm_deflate_quick_bound(PIECE))
            bufq, jobsq = jobs_for(boundq)
            resq = torch.zeros((np_all, 2), dtype=torch.int32, device="cuda")

            def quick():
                assert lib.zng_rocm_deflate_quick_dev(C.byref(jobsq), np_all, rocm._dev_ptr(resq), sp) == 0
            ways["quick"] = quick

        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            row = timings(ways)
            # what was written: the first and the last 64 members of each file, decoded by CPython
            for key, fn in ((k, ways[k]) for k in ("bgzf6", "bgzfq") if k in ways):
                table = np.zeros(np_all + 1, dtype=[("src_off", "<u8"), ("src_len", "<u8"), ("dst_off", "<u8"), ("out_len", "<u8"),
                                                    ("crc", "<u4"), ("bgzf", "<u4")])
                assert table.itemsize == C.sizeof(inf.GzipMember)
                dst.zero_()
                level, flags = (6, 0) if key == "bgzf6" else (1, dfl.BGZF_QUICK)
                assert lib.zng_rocm_bgzf_compress_dev(level, rocm._dev_ptr(src), n, 0, rocm._dev_ptr(dst), cap, C.byref(out_len),
                                                      C.c_void_p(table.ctypes.data), np_all + 1, C.byref(nmembers), 0, flags, sp) == 0
                st.synchronize()
                assert nmembers.value == np_all + 1 and int(table["src_off"][-1] + table["src_len"][-1]) == out_len.value
                for m in list(table[:64]) + list(table[-64:]):
                    member = dst[int(m["src_off"]):int(m["src_off"] + m["src_len"])].cpu().numpy().tobytes()
                    plain = src[int(m["dst_off"]):int(m["dst_off"] + m["out_len"])].cpu().numpy().tobytes()
                    assert zlib.decompressobj(31).decompress(member) == plain and zlib.crc32(plain) == int(m["crc"]), key
                size, members, stored, rounds = files[key]
                row[key].update(file_bytes=size, members=members, stored_members=stored, rounds=rounds, ratio=round(size / n, 4))
        if only is None:
            row["framing_share_6"] = round((row["bgzf6"]["ms"] - row["streams6"]["ms"]) / row["streams6"]["ms"], 4)
            row["framing_share_quick"] = round((row["bgzfq"]["ms"] - row["quick"]["ms"]) / row["quick"]["ms"], 4)
        row.update(plaintext_bytes=n, pieces=np_all)
        print(name, json.dumps(row), flush=True)
        return row

    out = {"tool": "tools/bgzf_rate.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "mib": a.mib,
           "figure": "median of reps, host clock around a synchronised call; GB/s of plaintext"}
    if a.only:
        leg("text", a.only)
    else:
        out["text"] = leg("text")
        torch.cuda.empty_cache()
        out["mix"] = leg("mix")
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    lib.zng_rocm_stream_release(sp)
    return 0


if __name__ == "__main__":
    sys.exit(main())
