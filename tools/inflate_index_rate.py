"""What random access into a plain gzip stream costs beside the whole-stream decode it replaces.

One stream, device-resident: gzip, --mib (1024) MiB of plaintext from synth.silesia_like compressed by CPython's zlib at level
6 (a stretch of 64 MiB is compressed on the host as raw deflate that ends in Z_FULL_FLUSH and repeated on the device up to the
size, an empty final block, header and trailer around it: a valid member whose blocks are CPython's).

The ways over it, alternating inside one process, one untimed warm-up each, then --reps (5) timings each over rotating buffers
(--rotate 2 copies of the file and of every destination, so that no call finds its bytes in the Infinity Cache from the call
before); a figure is the MEDIAN host time around a call that ends in a synchronise, with min and max beside it:

  whole       zng_rocm_uncompress_large_dev on the stream: before this tool's calls existed, the only way to serve any range
  build_S     zng_rocm_inflate_index_build_dev on the same stream at span S = 64 KiB, 256 KiB, 1 MiB (index created and
              destroyed inside the timing)
  read_4k_S   zng_rocm_inflate_index_read_dev: --ranges (4096) ranges of 4 KiB at random offsets (seeded), one call
  read_1m_S   the same with ranges of 1 MiB
  read_one_S  a single range of 4 KiB alone: the latency of one wavefront over at most one span

Recorded, not gated: build / whole, read_* / whole, the index bytes per plaintext byte at each span, the read calls' counters.
Every read is checked: all statuses 1, and the first, the last and 30 other ranges byte for byte against the plaintext.
--only-whole times `whole` alone; --lib PATH loads another build of the library (the parent commit's, to see that the whole
call's path has not become slower); --parent-whole FILE.json writes that run's figure beside this one's.

    python tools/inflate_index_rate.py [--mib 1024] [--reps 5] [--ranges 4096] [--out FILE.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KiB, MiB = 1 << 10, 1 << 20
SPANS = (64 * KiB, 256 * KiB, MiB)
HEADER = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=2)
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--only-whole", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--parent-whole", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_index_rate_v1.json"))
    a = ap.parse_args()
    assert a.reps >= 1 and a.rotate >= 1 and a.ranges >= 32 and a.mib >= 2
    import torch
    import synth
    zr = importlib.import_module("zlib-ng_amd")
    if a.lib:                                             # another build: it may be older than the index calls
        assert a.only_whole, "--lib times `whole` alone"
        zr.rocm._LIB_PATH = os.path.abspath(a.lib)
        for name in [k for k in zr.rocm._PROTOS if "inflate_index" in k]:
            del zr.rocm._PROTOS[name]
    zr.init(0)
    rocm = zr.rocm
    lib = rocm.lib()
    inf = importlib.import_module("zlib-ng_amd.inflate")
    st = torch.cuda.Stream()
    sp = C.c_void_p(st.cuda_stream)

    unit_mib = min(64, a.mib)
    p = synth.silesia_like(unit_mib * MiB, seed=0x1DE5)
    raw = p.tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    unit = c.compress(raw) + c.flush(zlib.Z_FULL_FLUSH)     # byte aligned, no reference across it: it can be repeated
    repeat = max(1, a.mib // unit_mib)
    plain_len = len(raw) * repeat
    crc1, crc = zlib.crc32(raw), 0
    for r in range(repeat):
        crc = int(lib.zng_rocm_crc32_combine(crc, crc1, len(raw))) if r else crc1
    tail = b"\x03\x00" + struct.pack("<II", crc, plain_len & 0xffffffff)
    total = len(HEADER) + len(unit) * repeat + len(tail)
    unit_dev = torch.from_numpy(np.frombuffer(unit, dtype=np.uint8).copy()).cuda()
    plain_dev = torch.from_numpy(p).cuda()
    srcs, wholes = [], []
    for _ in range(a.rotate):
        s = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        s[:len(HEADER)] = torch.from_numpy(np.frombuffer(HEADER, dtype=np.uint8).copy()).cuda()
        for r in range(repeat):
            s[len(HEADER) + r * len(unit):len(HEADER) + (r + 1) * len(unit)] = unit_dev
        s[total - len(tail):total] = torch.from_numpy(np.frombuffer(tail, dtype=np.uint8).copy()).cuda()
        srcs.append(s)
        wholes.append(torch.zeros(plain_len + 64, dtype=torch.uint8, device="cuda"))
    out_len, in_used = C.c_uint64(0), C.c_size_t(0)

    def whole(k):
        assert lib.zng_rocm_uncompress_large_dev(2, rocm._dev_ptr(srcs[k % a.rotate]), total, None, 0, rocm._dev_ptr(wholes[k % a.rotate]),
                                                 plain_len, C.byref(out_len), C.byref(in_used), 0, 0, sp) == 1

    def figure(v, nbytes):
        med = statistics.median(v)
        return dict(ms=round(med * 1e3, 4), min_ms=round(min(v) * 1e3, 4), max_ms=round(max(v) * 1e3, 4), gbps=round(nbytes / med / 1e9, 3))

    def timed(ways):
        per = {k: [] for k in ways}
        for fn in ways.values():                          # warm-up: allocates the scratch
            fn(0)
        st.synchronize()
        for rep in range(a.reps):
            for k, fn in ways.items():
                st.synchronize()
                t0 = time.perf_counter()
                fn(rep + 1)
                st.synchronize()
                per[k].append(time.perf_counter() - t0)
        return per

    out = {"tool": "tools/inflate_index_rate.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "rotate": a.rotate,
           "figure": "median of reps, host clock around a call that ends in a synchronise; GB/s of bytes delivered",
           "file_bytes": total, "plain_bytes": plain_len, "ranges": a.ranges, "lib": a.lib or "this tree's"}
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        if a.only_whole:
            out["whole"] = figure(timed({"whole": whole})["whole"], plain_len)
            assert (out_len.value, in_used.value) == (plain_len, total)
        else:
            rng = np.random.default_rng(0x1DE6)
            legs = {}
            for name, length, count in (("read_4k", 4096, a.ranges), ("read_1m", MiB, a.ranges), ("read_one", 4096, 1)):
                uoffs = [int(u) for u in rng.integers(0, plain_len - length, size=count)]
                dsts = [torch.zeros(count * length + 64, dtype=torch.uint8, device="cuda") for _ in range(a.rotate)]
                tables = []
                for d in dsts:
                    rs = (inf.InflateRange * count)()
                    for i, u in enumerate(uoffs):
                        rs[i] = inf.InflateRange(u, length, d.data_ptr() + i * length, 0, 0, None)
                    tables.append(rs)
                legs[name] = (length, uoffs, dsts, tables)
            indexes = {}

            def builder(span, keep):
                def run(k):
                    h = C.c_void_p(None)
                    assert lib.zng_rocm_inflate_index_build_dev(2, rocm._dev_ptr(srcs[k % a.rotate]), total, rocm._dev_ptr(wholes[k % a.rotate]),
                                                                plain_len, C.byref(out_len), C.byref(in_used), span, 0, 0, C.byref(h), sp) == 1
                    if keep and span not in indexes:
                        indexes[span] = h.value
                    else:
                        lib.zng_rocm_inflate_index_destroy(h)
                return run

            def reader(name, span):
                length, uoffs, dsts, tables = legs[name]

                def run(k):
                    assert lib.zng_rocm_inflate_index_read_dev(indexes[span], rocm._dev_ptr(srcs[k % a.rotate]), total,
                                                               C.cast(tables[k % a.rotate], C.c_void_p), len(uoffs), 0, sp) == 0
                return run

            ways = {"whole": whole}
            for span in SPANS:
                builder(span, True)(0)                    # the index the readers use
                ways["build_%dk" % (span // KiB)] = builder(span, False)
                for name in legs:
                    ways["%s_%dk" % (name, span // KiB)] = reader(name, span)
            per = timed(ways)
            assert (out_len.value, in_used.value) == (plain_len, total)
            out["whole"] = figure(per["whole"], plain_len)
            w = out["whole"]["ms"]
            for span in SPANS:
                tag = "%dk" % (span // KiB)
                need = C.c_size_t(0)
                lib.zng_rocm_inflate_index_export(indexes[span], None, 0, C.byref(need), sp)
                row = {"points": int(lib.zng_rocm_inflate_index_points(indexes[span], None, 0)), "index_bytes": int(need.value),
                       "index_bytes_per_plain_byte": round(need.value / plain_len, 6),
                       "build": figure(per["build_" + tag], plain_len)}
                row["build_over_whole"] = round(row["build"]["ms"] / w, 4)
                for name, (length, uoffs, dsts, tables) in legs.items():
                    for d in dsts:
                        d.zero_()
                    ways["%s_%s" % (name, tag)](0)
                    st.synchronize()
                    assert all(r.status == 1 and r.out_len == length and r.msg is None for r in tables[0]), (name, tag)
                    for i in sorted({0, len(uoffs) - 1} | {int(v) for v in rng.integers(0, len(uoffs), size=30)}):
                        u, got = uoffs[i], dsts[0][i * length:(i + 1) * length]
                        lo = u % len(raw)                 # the plaintext repeats every len(raw) bytes
                        want = torch.cat([plain_dev[lo:], plain_dev])[:length] if lo + length > len(raw) else plain_dev[lo:lo + length]
                        assert torch.equal(got, want), (name, tag, i, u)
                    row[name] = figure(per["%s_%s" % (name, tag)], len(uoffs) * length)
                    row[name].update(range_bytes=length, ranges=len(uoffs),
                                     counters={k: int(getattr(lib, "zng_rocm_inflate_index_read_last_" + k)()) for k in ("decoded", "direct", "rounds")})
                    row[name + "_over_whole"] = round(row[name]["ms"] / w, 4)
                out["span_" + tag] = row
                lib.zng_rocm_inflate_index_destroy(indexes[span])
    if a.parent_whole:
        with open(a.parent_whole) as f:
            out["whole_parent"] = json.load(f)["whole"]
        out["whole_over_parent"] = round(out["whole"]["ms"] / out["whole_parent"]["ms"], 4)
    lib.zng_rocm_stream_release(sp)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
