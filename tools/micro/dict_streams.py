"""What one shared preset dictionary is worth for many small device-resident messages: the dictionary calls
against the two ways the library had before, in one process, legs alternating.

The workload: --messages (65536) JSON-like records of --min-bytes .. --max-bytes (1 .. 8 KiB) and one 32 KiB dictionary of
similar records.  The records are drawn from a pool of --pool (4096) distinct ones (message i = pool[i mod pool]: every
message is its own stream, so repeating a record changes nothing a stream does).

  deflate   a  zng_rocm_compress_streams_dev, format 0: no dictionary
            b  zng_rocm_deflate_quick_dev with the dictionary copied in front of EVERY message (the way before)
            c  zng_rocm_compress_streams_dict_dev, format 0: the dictionary object
  inflate   a  zng_rocm_uncompress_streams_dev, format 0, over the streams of deflate a
            b  zng_rocm_inflate_streams_dev over the streams of deflate c, the dictionary copied in front of EVERY output
            c  zng_rocm_uncompress_streams_dict_dev, format 0, over the same streams

  level 6   a  zng_rocm_compress_streams2_dev, format 0, level 6: no dictionary
            b  the same call with the dictionary copied in front of EVERY message and dict_len = W (the way before)
            c  zng_rocm_compress_streams2_dict_dev, format 0, level 6: the dictionary object
            (b and c write the same bytes: every result row is compared, and every 1024th stream)

Every leg is warmed (one untimed call: it allocates the scratch), then the legs take turns until each has been timed for
--window-s (1.0) seconds in total and at least --min-reps (5) times.  A timing is the device time between two events
recorded around the call on its stream.  Per leg: median, min, max and quartiles in ms, spread = (p75 - p25) / median, GB/s of
plaintext, and for deflate the compressed total and its ratio.  Before the timings every 1024th stream of deflate c is read
back by CPython with zdict= and every output of inflate c is compared with the plaintext on the device.

--parent-lib FILE adds the `streams` workload of bench.py (4096 x 1 MiB of the six-class mix, zng_rocm_deflate_quick_dev) and
its `deflate_lvl6` workload (one 256 MiB stream, zng_rocm_deflate_dev at level 6) through the library at FILE and through this
tree's, alternating in the same process: the existing kernels are meant to be the same code in both, and this is where that
is looked at.

--only LEG (deflate_a .. level6_c, level6 for the three level-6 legs, or all) runs that leg --min-reps + 1 times behind the checks and writes no report: the
form a profiler is pointed at.

    python tools/micro/dict_streams.py [--messages 65536] [--window-s 1.0] [--parent-lib FILE] [--only LEG] [--out FILE.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = ("deflate_a", "deflate_b", "deflate_c", "inflate_a", "inflate_b", "inflate_c", "level6_a", "level6_b", "level6_c")


def records(count, lo, hi, seed):
    """JSON-like records of lo .. hi bytes: the same keys, a shared vocabulary, different values (cut to size)"""
    rng = np.random.default_rng(seed)
    wr = np.random.default_rng(2024)
    words = ["".join(chr(int(c)) for c in wr.integers(97, 123, size=int(k))) for k in wr.integers(3, 11, size=400)]
    out = []
    for _ in range(count):
        want = int(rng.integers(lo, hi + 1))
        w = [words[int(v)] for v in rng.integers(0, 400, size=3)]
        parts = ['{"id": %d, "user": "%s", "active": %s, "email": "%s@%s.example.com", "items": ['
                 % (int(rng.integers(0, 10 ** 9)), w[0], ("true", "false")[int(rng.integers(0, 2))], w[1], w[2])]
        size = len(parts[0])
        while size < want:
            v = rng.integers(0, 400, size=4)
            item = ('{"sku": "%s-%04d", "price": %.2f, "currency": "EUR", "status": "%s", "note": "%s %s %s"}, '
                    % (words[int(v[0])], int(rng.integers(0, 10000)), float(rng.integers(1, 100000)) / 100,
                       ("shipped", "pending", "returned")[int(rng.integers(0, 3))], words[int(v[1])], words[int(v[2])], words[int(v[3])]))
            parts.append(item)
            size += len(item)
        out.append("".join(parts).encode()[:want])
    return out


def summary(ms, nbytes):
    ms = sorted(ms)
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [ms[0], statistics.median(ms), ms[-1]]
    med = statistics.median(ms)
    return dict(reps=len(ms), ms=round(med, 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), p25_ms=round(q[0], 4),
                p75_ms=round(q[2], 4), spread=round((q[2] - q[0]) / med, 4), gbps=round(nbytes / med / 1e6, 3))


def alternate(torch, st, legs, window_s, min_reps):
    """legs: {name: callable}; every leg once untimed, then turns until each has window_s seconds and min_reps timings"""
    for fn in legs.values():
        fn()
    st.synchronize()
    per = {k: [] for k in legs}
    while any(sum(v) < window_s * 1e3 or len(v) < min_reps for v in per.values()):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            per[k].append(e0.elapsed_time(e1))
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=65536)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--min-bytes", type=int, default=1024)
    ap.add_argument("--max-bytes", type=int, default=8192)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--min-reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default=None, choices=LEGS + ("level6", "all"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_streams_rate_v2.json"))
    a = ap.parse_args()
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    inf = importlib.import_module("zlib-ng_amd.inflate")
    rocm = zr.rocm
    lib = rocm.lib()
    st = torch.cuda.Stream()
    sp = C.c_void_p(st.cuda_stream)
    W = 32768

    n = a.messages
    pool = records(min(a.pool, n), a.min_bytes, a.max_bytes, seed=11)
    D = b"".join(records(64, a.min_bytes, a.max_bytes, seed=5))[-W:]
    assert len(D) == W
    lens = [len(pool[i % len(pool)]) for i in range(n)]
    total = sum(lens)

    # the plaintext, messages 16-byte aligned; and the same with the dictionary in front of every message
    pool_off, pos = [], 0
    for m in pool:
        pool_off.append(pos)
        pos += (len(m) + 15) & ~15
    pool_img = np.zeros(pos + 16, dtype=np.uint8)
    for o, m in zip(pool_off, pool):
        pool_img[o:o + len(m)] = np.frombuffer(m, dtype=np.uint8)
    d_pool = torch.from_numpy(pool_img).cuda()
    d_dict = torch.from_numpy(np.frombuffer(D, dtype=np.uint8).copy()).cuda()
    slot = (a.max_bytes + 15) & ~15
    plain = torch.zeros(n * slot + 16, dtype=torch.uint8, device="cuda")
    front = torch.zeros(n * (W + slot) + 16, dtype=torch.uint8, device="cuda")
    plain_v, front_v = plain[:n * slot].view(n, slot), front[:n * (W + slot)].view(n, W + slot)
    front_v[:, :W] = d_dict
    for k, (o, m) in enumerate(zip(pool_off, pool)):
        plain_v[k::len(pool), :len(m)] = d_pool[o:o + len(m)]
        front_v[k::len(pool), W:W + len(m)] = d_pool[o:o + len(m)]
    in_off = [i * slot for i in range(n)]
    front_off = [i * (W + slot) + W for i in range(n)]

    torch.cuda.synchronize()                                     # the buffers were filled on the default stream
    dic = dfl.Dictionary(d_dict, stream=st)
    assert dic.id == zlib.adler32(D) and dic.window == W
    with torch.cuda.stream(st):
        wa = dfl.WrappedBatch(plain, in_off, lens, 0)
        wb = dfl.QuickBatch(front, front_off, lens, dict_len=[W] * n)
        wc = dfl.WrappedBatch(plain, in_off, lens, 0, for_dict=True)
        wa.run(st)
        wb.run(st)
        wc.run_dict(dic, st)
        st.synchronize()
        ra, rb, rc = wa.results.cpu().numpy(), wb.results.cpu().numpy(), wc.results.cpu().numpy()
        ca, cb, cc = [int(v) for v in ra[:, 0]], [int(v) for v in rb[:, 0]], [int(v) for v in rc[:, 0]]
        for i in range(0, n, 1024):                              # what was written: read by CPython with the dictionary
            got = zlib.decompressobj(-15, zdict=D).decompress(wc.compressed(i, torch.from_numpy(rc)))
            assert got == pool[i % len(pool)], i
            got = zlib.decompressobj(-15, zdict=D).decompress(wb.compressed(i, torch.from_numpy(rb)))
            assert got == pool[i % len(pool)], i
        # inflate: outputs 16-byte aligned; and with the dictionary in front of every output
        back = torch.zeros(n * slot + 16, dtype=torch.uint8, device="cuda")
        back_front = torch.zeros(n * (W + slot) + 16, dtype=torch.uint8, device="cuda")
        back_front[:n * (W + slot)].view(n, W + slot)[:, :W] = d_dict
        ia = inf.InflateDevBatch(wa.dst, wa.out_off, ca, back, in_off, lens)
        ib = inf.InflateDevBatch(wc.dst, wc.out_off, cc, back_front, front_off, lens, dict_len=[W] * n)
        ic = inf.InflateDevBatch(wc.dst, wc.out_off, cc, back, in_off, lens)
        ic.run_dict(0, dic, st)
        st.synchronize()
        r = ic.results.cpu().numpy()
        assert (r[:, 2] == 1).all() and r[:, 0].tolist() == lens and r[:, 1].tolist() == cc
        assert torch.equal(back, plain)
        ib.run(st)
        st.synchronize()
        assert (ib.results.cpu().numpy() == r).all()

        legs = {"deflate_a": lambda: wa.run(st), "deflate_b": lambda: wb.run(st), "deflate_c": lambda: wc.run_dict(dic, st),
                "inflate_a": lambda: ia.run_wrapped(0, st), "inflate_b": lambda: ib.run(st), "inflate_c": lambda: ic.run_dict(0, dic, st)}
        l6_legs, l6_sizes = level6_legs(torch, st, dfl, lib, dic, D, pool, plain, front, in_off, front_off, lens)
        legs.update(l6_legs)
        if a.only:
            pick = LEGS if a.only == "all" else tuple(l6_legs) if a.only == "level6" else (a.only,)
            for _ in range(a.min_reps + 1):
                for k in pick:
                    legs[k]()
            st.synchronize()
            return 0
        out = {"tool": "tools/micro/dict_streams.py", "device": torch.cuda.get_device_name(0), "messages": n,
               "distinct_messages": len(pool), "message_bytes": [min(lens), max(lens)], "plaintext_bytes": total, "dictionary_bytes": W,
               "figure": "device time between two events around the call; median over the reps of a window of at least "
                         "%.1f s per leg, legs alternating; spread = (p75 - p25) / median; GB/s of plaintext" % a.window_s}
        for side in ("deflate", "inflate", "level6"):
            per = alternate(torch, st, {k: v for k, v in legs.items() if k.startswith(side)}, a.window_s, a.min_reps)
            for k, v in per.items():
                out[k] = summary(v, total)
        for k, c in (("deflate_a", ca), ("deflate_b", cb), ("deflate_c", cc)):
            out[k].update(compressed_bytes=sum(c), ratio=round(total / sum(c), 4))
        out["dictionary_gain"] = round(1.0 - sum(cc) / sum(ca), 4)
        for k, c in l6_sizes.items():
            out[k].update(compressed_bytes=c, ratio=round(total / c, 4))
        out["level6_dictionary_gain"] = round(1.0 - l6_sizes["level6_c"] / l6_sizes["level6_a"], 4)
        b, c = out["level6_b"], out["level6_c"]
        out["level6_c_over_b"] = round(b["ms"] / c["ms"], 4)
        out["level6_c_faster_than_b"] = bool(c["p75_ms"] < b["p25_ms"])
        b, c = out["deflate_b"], out["deflate_c"]
        out["deflate_c_within_b_spread"] = bool(c["ms"] <= b["ms"] + (b["p75_ms"] - b["p25_ms"]))
        b, c = out["inflate_b"], out["inflate_c"]
        out["inflate_c_within_b_spread"] = bool(c["ms"] <= b["ms"] + (b["p75_ms"] - b["p25_ms"]))
        for k in LEGS:
            print(k, json.dumps(out[k]), flush=True)

        if a.parent_lib:
            out["streams_parent_vs_new"], out["deflate_lvl6_parent_vs_new"] = parent_leg(a, torch, st, sp, lib)
            print("streams", json.dumps(out["streams_parent_vs_new"]), flush=True)
            print("deflate_lvl6", json.dumps(out["deflate_lvl6_parent_vs_new"]), flush=True)
    dic.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    lib.zng_rocm_stream_release(sp)
    return 0


def level6_legs(torch, st, dfl, lib, dic, D, pool, plain, front, in_off, front_off, lens):
    """the three level-6 legs over one shared set of output slots (the legs run one behind the other on one stream), checked
    once: the object's streams are read by CPython with zdict=, and the in-front call writes the same rows and bytes"""
    n, W = len(lens), len(D)
    out_off, pos = [], 0
    for v in lens:
        out_off.append(pos)
        pos += (lib.zng_rocm_compress_streams2_bound(v, 0) + 15) & ~15
    dst = torch.zeros(pos + 16, dtype=torch.uint8, device="cuda")

    def table(src, offs, dict_len):
        jobs = (dfl.StreamJob * n)()
        for i in range(n):
            jobs[i].in_ptr, jobs[i].in_len, jobs[i].dict_len = src.data_ptr() + offs[i], lens[i], dict_len
            jobs[i].out_ptr, jobs[i].out_cap = dst.data_ptr() + out_off[i], lib.zng_rocm_compress_streams2_bound(lens[i], 0)
        return jobs
    ja, jb, jc = table(plain, in_off, 0), table(front, front_off, W), table(plain, in_off, 0)
    res = {k: torch.zeros((n, 2), dtype=torch.int32, device="cuda") for k in "abc"}

    def ok(rc):
        assert rc == 0, rc
    legs = {"level6_a": lambda: ok(dfl.compress_streams2_dev(ja, n, res["a"], 0, 6, 0, 0, st)),
            "level6_b": lambda: ok(dfl.compress_streams2_dev(jb, n, res["b"], 0, 6, 0, 0, st)),
            "level6_c": lambda: ok(dfl.compress_streams2_dict_dev(dic, jc, n, res["c"], 0, 6, 0, 0, st))}
    samples = {}
    for k in ("c", "b", "a"):
        legs["level6_" + k]()
        st.synchronize()
        size = res[k].cpu().numpy()[:, 0]
        samples[k] = [dst[out_off[i]:out_off[i] + int(size[i])].cpu().numpy().tobytes() for i in range(0, n, 1024)]
    for i, c in zip(range(0, n, 1024), samples["c"]):
        assert zlib.decompressobj(-15, zdict=D).decompress(c) == pool[i % len(pool)], i
    assert torch.equal(res["b"], res["c"]) and samples["b"] == samples["c"]
    return legs, {"level6_" + k: int(res[k].cpu().numpy()[:, 0].astype(np.int64).sum()) for k in "abc"}


def parent_leg(a, torch, st, sp, lib):
    """bench.py's `streams` and `deflate_lvl6` workloads through two builds of the library in one process"""
    import synth
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    old = C.CDLL(os.path.abspath(a.parent_lib))
    for h in (old, lib):
        h.zng_rocm_deflate_quick_dev.restype = C.c_int
        h.zng_rocm_deflate_quick_dev.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    old.zng_rocm_init.argtypes = [C.c_int]
    assert old.zng_rocm_init(0) == 0
    each, distinct, count = 1 << 20, 96, 4096
    base = synth.silesia_like(distinct << 20, seed=0x5EED0005, seg_bytes=1 << 20)
    d_base = torch.from_numpy(base).cuda().view(distinct, each)
    src = d_base[torch.arange(count, device="cuda") % distinct].reshape(-1).contiguous()
    del d_base
    batch = dfl.QuickBatch(src, [i * each for i in range(count)], [each] * count)
    res_old = torch.zeros_like(batch.results)

    def new():
        assert lib.zng_rocm_deflate_quick_dev(C.byref(batch.jobs), count, C.c_void_p(batch.results.data_ptr()), sp) == 0

    def parent():
        assert old.zng_rocm_deflate_quick_dev(C.byref(batch.jobs), count, C.c_void_p(res_old.data_ptr()), sp) == 0
    per = alternate(torch, st, {"parent": parent, "new": new}, a.window_s, a.min_reps)
    st.synchronize()
    assert torch.equal(res_old, batch.results)                   # the same bytes and check values from both builds
    row = {k: summary(v, count * each) for k, v in per.items()}
    p = row["parent"]
    row["new_within_parent_spread"] = bool(p["min_ms"] <= row["new"]["ms"] <= p["max_ms"])
    del batch, src, res_old

    # deflate_lvl6: one 256 MiB stream, level 6, the synchronous call (its host synchronisation inside the timing)
    nbytes = 256 << 20
    one = torch.from_numpy(synth.silesia_like(nbytes, seed=0x5EED0003)).cuda()
    cap = lib.zng_rocm_deflate_bound(nbytes)
    outs = {"parent": torch.zeros(cap, dtype=torch.uint8, device="cuda"), "new": torch.zeros(cap, dtype=torch.uint8, device="cuda")}
    lens = {"parent": C.c_size_t(0), "new": C.c_size_t(0)}
    for h in (old, lib):
        h.zng_rocm_deflate_dev.restype = C.c_int
        h.zng_rocm_deflate_dev.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]

    def lvl6(h, k):
        return lambda: h.zng_rocm_deflate_dev(6, C.c_void_p(one.data_ptr()), nbytes, C.c_void_p(outs[k].data_ptr()), cap, C.byref(lens[k]), sp)
    per = alternate(torch, st, {"parent": lvl6(old, "parent"), "new": lvl6(lib, "new")}, a.window_s, a.min_reps)
    st.synchronize()
    assert lens["parent"].value == lens["new"].value and torch.equal(outs["parent"][:lens["new"].value], outs["new"][:lens["new"].value])
    row6 = {k: summary(v, nbytes) for k, v in per.items()}
    p = row6["parent"]
    row6["compressed_bytes"] = int(lens["new"].value)
    row6["new_within_parent_spread"] = bool(p["min_ms"] <= row6["new"]["ms"] <= p["max_ms"])
    old.zng_rocm_shutdown()
    return row, row6


if __name__ == "__main__":
    sys.exit(main())
