"""What zng_rocm_gunzip_members_dev costs and saves: the whole-file call against the loop a caller wrote before
it, and against the engine underneath handed the members' exact boundaries.

Three files, device-resident, made from synth.silesia_like by CPython's zlib at level 6 (a stretch of distinct members is
compressed on the host and repeated on the device up to the leg's size: members are independent, so the file is valid and no
two neighbours are alike):

  bgzf      BGZF, --mib (1024) MiB of plaintext in blocks of 65280 bytes, and the 28-byte end-of-file block
  shards    256 x 4 MiB members, one behind the other
  large     16 x 64 MiB members

and three ways over each, alternating inside one process, one untimed warm-up each, then --reps (5) timings each over
rotating source and destination buffers (--rotate 2 copies of both); a figure is the MEDIAN timing, with min and max beside
it, and GB/s of output:

  new       zng_rocm_gunzip_members_dev on the whole file
  baseline  the caller's loop: zng_rocm_uncompress_large_dev(2, ...) on what is left of the file, following in_used, until the
            file is used up.  bgzf: the loop is timed over the first --prefix (512) members and scaled to all of them
            ("extrapolated": true, with the members timed); the legs' other figures are never scaled
  ceiling   the engine underneath with the members' boundaries computed on the host beforehand: bgzf
            zng_rocm_uncompress_streams_dev (one launch), shards / large zng_rocm_uncompress_large_streams_dev

Required: new <= baseline on every leg ("not_slower_than_baseline"; the tool exits 1 otherwise).  Recorded, not gated: new -
ceiling, the cost of discovery, planning and verification.

    python tools/gunzip_members_rate.py [--mib 1024] [--reps 5] [--only bgzf|shards|large] [--out FILE.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MiB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=2)
    ap.add_argument("--prefix", type=int, default=512)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gunzip_members_rate_v1.json"))
    a = ap.parse_args()
    assert a.reps >= 1 and a.prefix >= 256 and a.rotate >= 1
    import torch
    import synth
    import gzip_files
    import wrapped_members as fixture
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    inf = importlib.import_module("zlib-ng_amd.inflate")
    rocm = zr.rocm
    lib = rocm.lib()
    st = torch.cuda.Stream()
    sp = C.c_void_p(st.cuda_stream)

    def timings(ways, output_bytes):
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
        return {k: dict(ms=round(statistics.median(v) * 1e3, 4), min_ms=round(min(v) * 1e3, 4), max_ms=round(max(v) * 1e3, 4),
                        gbps=round(output_bytes / statistics.median(v) / 1e9, 3)) for k, v in per.items()}

    def leg(name, stretch, repeat, tail=b""):
        """stretch: [(member bytes, plaintext length)] compressed on the host, laid out `repeat` times, then `tail`"""
        unit = b"".join(m for m, _ in stretch)
        unit_plain = sum(n for _, n in stretch)
        tail_members = [(tail, 0)] if tail else []
        members = stretch * repeat + tail_members
        total, out_total = len(unit) * repeat + len(tail), unit_plain * repeat
        unit_dev = torch.from_numpy(np.frombuffer(unit, dtype=np.uint8).copy()).cuda()
        srcs, dsts = [], []
        for _ in range(a.rotate):
            s = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
            for r in range(repeat):
                s[r * len(unit):(r + 1) * len(unit)] = unit_dev
            if tail:
                s[len(unit) * repeat:total] = torch.from_numpy(np.frombuffer(tail, dtype=np.uint8).copy()).cuda()
            srcs.append(s)
            dsts.append(torch.zeros(out_total + 64, dtype=torch.uint8, device="cuda"))
        in_off, out_off, at, out = [], [], 0, 0
        for m, n in members:
            in_off.append(at)
            out_off.append(out)
            at += len(m)
            out += n
        nm = len(members)
        table = (inf.GzipMember * nm)()
        out_len, in_used, nmembers = C.c_uint64(0), C.c_size_t(0), C.c_size_t(0)

        def new(k):
            s, d = srcs[k % a.rotate], dsts[k % a.rotate]
            assert lib.zng_rocm_gunzip_members_dev(rocm._dev_ptr(s), total, rocm._dev_ptr(d), out_total, C.byref(out_len), C.byref(in_used),
                                                   C.cast(table, C.c_void_p), nm, C.byref(nmembers), 0, sp) == 1

        loop_members = min(nm, a.prefix) if name == "bgzf" else nm

        def baseline(k):
            s, d = srcs[k % a.rotate], dsts[k % a.rotate]
            at, out = 0, 0
            for _ in range(loop_members):
                rc = lib.zng_rocm_uncompress_large_dev(2, rocm._dev_ptr(s, at), total - at, None, 0, rocm._dev_ptr(d, out), out_total - out,
                                                       C.byref(out_len), C.byref(in_used), 0, 0, sp)
                assert rc == 1
                at += in_used.value
                out += out_len.value
            assert at == (in_off[loop_members] if loop_members < nm else total)

        if name == "bgzf":
            batches = [inf.InflateDevBatch(s, in_off, [len(m) for m, _ in members], d, out_off, [n for _, n in members])
                       for s, d in zip(srcs, dsts)]

            def ceiling(k):
                batches[k % a.rotate].run_wrapped(2, stream=st)
        else:
            jobs = [inf.large_jobs([s[o:o + len(m)] for o, (m, _) in zip(in_off, members)],
                                   [d[o:o + n] for o, (_, n) in zip(out_off, members)]) for s, d in zip(srcs, dsts)]

            def ceiling(k):
                assert lib.zng_rocm_uncompress_large_streams_dev(2, C.cast(jobs[k % a.rotate], C.c_void_p), nm, 0, 0, sp) == 0

        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            row = timings({"new": new, "baseline": baseline, "ceiling": ceiling}, out_total)
            for d in dsts:
                d.zero_()
            new(0)
            st.synchronize()
            assert (out_len.value, in_used.value, nmembers.value) == (out_total, total, nm), (out_len.value, in_used.value, nmembers.value)
            counters = {k: int(getattr(lib, "zng_rocm_gunzip_last_" + k)()) for k in ("candidates", "replans", "small", "large")}
            want = torch.from_numpy(np.concatenate([p for p in plains[name]])).cuda()
            for r in (0, repeat - 1):                     # the first and the last repeat of the stretch, byte for byte
                assert torch.equal(dsts[0][r * unit_plain:(r + 1) * unit_plain], want), r
            assert all((t.src_off, t.src_len, t.dst_off, t.out_len) == (in_off[i], len(members[i][0]), out_off[i], members[i][1])
                       for i, t in enumerate(table[:nm]))
            if name == "bgzf":
                res = batches[0].rows()
                assert all(r[0] == 1 for r in res)
        if loop_members < nm:                             # the loop over a prefix, scaled by members (every BGZF block is alike)
            timed = row["baseline"]
            scale = nm / loop_members
            row["baseline"] = dict(ms=round(timed["ms"] * scale, 4), min_ms=round(timed["min_ms"] * scale, 4),
                                   max_ms=round(timed["max_ms"] * scale, 4), gbps=round(out_total / (timed["ms"] * scale / 1e3) / 1e9, 3),
                                   extrapolated=True, members_timed=loop_members, timed_ms=timed["ms"])
        row.update(members=nm, file_bytes=total, output_bytes=out_total, counters=counters,
                   new_minus_ceiling_ms=round(row["new"]["ms"] - row["ceiling"]["ms"], 4),
                   new_over_ceiling=round(row["new"]["ms"] / row["ceiling"]["ms"], 3),
                   not_slower_than_baseline=bool(row["new"]["ms"] <= row["baseline"]["ms"]))
        print(name, json.dumps(row), flush=True)
        del srcs, dsts, want
        torch.cuda.empty_cache()
        return row

    out = {"tool": "tools/gunzip_members_rate.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "rotate": a.rotate,
           "figure": "median of reps; GB/s of output"}
    plains = {}
    if a.only in (None, "bgzf"):
        unit_mib = min(64, a.mib)
        p = synth.silesia_like(unit_mib * MiB // gzip_files.BGZF_BLOCK * gzip_files.BGZF_BLOCK, seed=0xB6F)
        plains["bgzf"] = [p]
        raw = p.tobytes()
        stretch = [(gzip_files.bgzf_block(raw[at:at + gzip_files.BGZF_BLOCK]), gzip_files.BGZF_BLOCK)
                   for at in range(0, len(raw), gzip_files.BGZF_BLOCK)]
        out["bgzf"] = leg("bgzf", stretch, max(1, a.mib // unit_mib), tail=gzip_files.BGZF_EOF)
    if a.only in (None, "shards"):
        plains["shards"] = [synth.silesia_like(4 * MiB, seed=0x5A0 + k) for k in range(16)]
        out["shards"] = leg("shards", [(fixture.gzip_file(p.tobytes(), "shard-%05d.bin" % k), p.size) for k, p in enumerate(plains["shards"])], 16)
    if a.only in (None, "large"):
        plains["large"] = [synth.silesia_like(64 * MiB, seed=0x1A6 + k) for k in range(2)]
        out["large"] = leg("large", [(fixture.gzip_file(p.tobytes(), ""), p.size) for p in plains["large"]], 8)
    lib.zng_rocm_stream_release(sp)
    legs = [k for k in ("bgzf", "shards", "large") if k in out]
    out["required_new_not_slower_than_baseline"] = all(out[k]["not_slower_than_baseline"] for k in legs)
    if a.out and not a.only:                              # a single leg (a profiler run) leaves the report alone
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print("new <= baseline on every leg:", out["required_new_not_slower_than_baseline"], flush=True)
    return 0 if out["required_new_not_slower_than_baseline"] else 1


if __name__ == "__main__":
    sys.exit(main())
