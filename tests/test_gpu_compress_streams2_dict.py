"""GPU: the shared preset dictionary at every level (zng_rocm_compress_streams2_dict_dev, zng_rocm_compress_members_dict_dev),
through the C ABI.

  * the oracle is existing code: the same batch through zng_rocm_compress_streams2_dev / zng_rocm_compress_members_dev with the
    window copied in front of every plaintext and dict_len = W gives the same result rows and the same bytes -- for window
    lengths around every rule of the primed tables (T = the whole batches with T + 3 <= W), levels 1 / 6 / 9, the default and
    the Z_FIXED strategy, one round and three, per-job buffers and one file;
  * format 1 is the 6 header bytes of the CPU rule, the format-0 bytes and the Adler-32 of the plaintext; CPython with zdict=
    and zng_rocm_uncompress_streams_dict_dev restore every member; level 0 is stored blocks behind the same header;
  * the dictionary is USED at level 6: random bytes cut from it compress, and on JSON-like records the device gains at least
    half of what CPython's level 6 gains from the same dictionary, and more than the level-1 dictionary call;
  * refusals, a dictionary that outlives zng_rocm_shutdown(), and the level-1 dictionary call writes what it wrote before the
    object carried the row tables."""
import ctypes as C
import importlib
import json
import struct
import zlib

import numpy as np
import pytest

import synth
from gpu_common import product, torch_mod

pytestmark = pytest.mark.gpu

DICT_LENS = (1, 3, 4, 257, 1026, 1027, 2050, 32767, 32768, 50000)
LEVELS = (1, 6, 9)
STRATEGIES = (0, 4)
GUARD = 0xA5


@pytest.fixture(scope="module")
def mods():
    zr = product()
    zr.init()
    return zr, importlib.import_module("zlib-ng_amd.deflate"), importlib.import_module("zlib-ng_amd.inflate")


_WORDS = None


def _words():
    global _WORDS
    if _WORDS is None:
        rng = np.random.default_rng(2024)
        _WORDS = ["".join(chr(int(c)) for c in rng.integers(97, 123, size=int(k))) for k in rng.integers(3, 11, size=400)]
    return _WORDS


def _records(count, seed, lo=200, hi=2000):
    """the JSON-like records of tests/test_gpu_streams_dict.py: the same keys and a shared vocabulary, different values"""
    rng = np.random.default_rng(seed)
    words = _words()
    out = []
    for k in range(count):
        want = int(rng.integers(lo, hi + 1))
        rec = {"id": int(rng.integers(0, 10 ** 9)), "user": words[int(rng.integers(0, 400))], "active": bool(rng.integers(0, 2)),
               "email": "%s@%s.example.com" % (words[int(rng.integers(0, 400))], words[int(rng.integers(0, 400))]),
               "created_at": "2024-%02d-%02dT%02d:%02d:%02dZ" % tuple(int(v) for v in rng.integers(1, 13, size=5)), "items": []}
        while len(json.dumps(rec)) < want:
            rec["items"].append({"sku": "%s-%04d" % (words[int(rng.integers(0, 400))], int(rng.integers(0, 10000))),
                                 "price": round(float(rng.integers(1, 100000)) / 100, 2), "currency": "EUR",
                                 "status": ("shipped", "pending", "returned")[int(rng.integers(0, 3))],
                                 "note": " ".join(words[int(v)] for v in rng.integers(0, 400, size=3))})
        out.append(json.dumps(rec).encode()[:want])                           # cut to size: JSON-like, not JSON
    return out


@pytest.fixture(scope="module")
def corpus():
    """the dictionaries, the long texts and the record set: made once, never changed"""
    record_dict = b"".join(_records(60, seed=5))[-32768:]
    dicts = {}
    for n in DICT_LENS:
        text = b"".join(_records(80, seed=n))
        dicts[n] = (text * (n // len(text) + 1))[:n] if n != 32768 else record_dict
    long_text = b"".join(_records(140, seed=21))
    assert len(long_text) > (128 << 10) + 5000
    return {"dicts": dicts, "records": _records(200, seed=11), "record_dict": record_dict, "long": long_text,
            "small": _records(28, seed=31, lo=1024, hi=4096), "noise": synth.silesia_like(20000, seed=9).tobytes()}


def _streams(D, corpus):
    """about 40 streams: the short lengths, the length that ends on a batch border, records that share substrings with the
    dictionary, a copy of the window from its first byte, a periodic continuation of its last 300 bytes (a match that begins in
    the window and runs into the plaintext), two blocks, two segments"""
    window = D[-32768:]
    W = len(window)
    long_text = corpus["long"]
    tail = window[-300:]
    out = [b"", b"q", long_text[:3], long_text[7:11], long_text[100:100 + 1024 - W % 1024],
           window[:min(W, 6000)] + b" and then something of its own " + window[W // 2:W // 2 + 500],
           (tail * (2000 // len(tail) + 2))[:2000],
           window[W // 3:W // 3 + 900] + corpus["noise"][:700] + window[-min(W, 1500):],
           long_text[5000:5000 + 61440 + 100],
           long_text[:(128 << 10) + 5000]]
    return out + corpus["small"]


def _pack(blobs, front=0, history=b"", pad=5, first=3):
    """the blobs at odd offsets in one host image, `front` bytes of `history` in front of each"""
    offs, pos = [], first
    for b in blobs:
        offs.append(pos + front)
        pos += front + len(b) + pad
    host = np.full(pos + 64, 0x5c, dtype=np.uint8)
    for o, b in zip(offs, blobs):
        if front:
            host[o - front:o] = np.frombuffer(history, dtype=np.uint8)
        host[o:o + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    return host, offs


class _Batch:
    """one set of plaintexts on the device, with the window in front of each (W > 0) or not, and the job table over it"""

    def __init__(self, dfl, msgs, window=b"", flags=None):
        torch = torch_mod()
        self.dfl, self.msgs, self.W = dfl, msgs, len(window)
        host, self.offs = _pack(msgs, front=len(window), history=window)
        self.src = torch.from_numpy(host).cuda()
        self.flags = flags

    def jobs(self, bounds=None):
        """per-job buffers of bounds[i] bytes at odd offsets in one guarded tensor (None: the members form)"""
        torch = torch_mod()
        n = len(self.msgs)
        jobs = (self.dfl.StreamJob * n)()
        dst, out_off = None, []
        if bounds is not None:
            pos = 7
            for b in bounds:
                out_off.append(pos)
                pos += b + 9
            dst = torch.full((pos + 64,), GUARD, dtype=torch.uint8, device="cuda")
        for i, m in enumerate(self.msgs):
            jobs[i].in_ptr = self.src.data_ptr() + self.offs[i]
            jobs[i].in_len = len(m)
            jobs[i].dict_len = self.W
            jobs[i].flags = 0 if self.flags is None else self.flags[i]
            if bounds is not None:
                jobs[i].out_ptr = dst.data_ptr() + out_off[i]
                jobs[i].out_cap = bounds[i]
        return jobs, dst, out_off


def _per_job(zr, dfl, batch, dic, fmt, level, strategy, round_bytes=0):
    """streams2 (dic None: the plain call) -> (result rows, members, rounds)"""
    torch = torch_mod()
    lib = zr.lib()
    n = len(batch.msgs)
    bound = lib.zng_rocm_compress_streams2_dict_bound if dic is not None else lib.zng_rocm_compress_streams2_bound
    bounds = [bound(len(m), fmt) for m in batch.msgs]
    jobs, dst, out_off = batch.jobs(bounds)
    res = torch.full((n, 2), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    if dic is not None:
        rc = dfl.compress_streams2_dict_dev(dic, jobs, n, res, fmt, level, strategy, round_bytes)
    else:
        rc = dfl.compress_streams2_dev(jobs, n, res, fmt, level, strategy, round_bytes)
    assert rc == 0, (rc, zr.last_error() if hasattr(zr, "last_error") else "")
    rounds = dfl.compress_streams2_last_rounds()
    torch.cuda.synchronize()
    rows = [[v & 0xffffffff for v in row] for row in res.cpu().tolist()]
    got = dst.cpu().numpy()
    members = []
    for (total, _), o, b in zip(rows, out_off, bounds):
        assert total <= b
        members.append(got[o:o + total].tobytes())
        assert got[o + b:o + b + 9].tolist() == [GUARD] * 9 and got[o - 7:o].tolist() == [GUARD] * 7, "bytes outside out_cap were written"
    return rows, members, rounds


def _file(zr, dfl, batch, dic, fmt, level, strategy, round_bytes=0, cap=None):
    """members -> (offsets, checks, the file's bytes up to min(length, cap))"""
    torch = torch_mod()
    n = len(batch.msgs)
    jobs, _, _ = batch.jobs(None)
    if cap is None:
        cap = sum(zr.lib().zng_rocm_compress_streams2_dict_bound(len(m), max(fmt, 0)) for m in batch.msgs)
    dst = torch.full((cap + 32,), GUARD, dtype=torch.uint8, device="cuda")
    offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    checks = torch.full((n,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    if dic is not None:
        rc = dfl.compress_members_dict_dev(dic, jobs, n, dst[:cap], offsets, fmt, level, strategy, round_bytes, checks)
    else:
        rc = dfl.compress_members_dev(jobs, n, dst[:cap], offsets, fmt, level, strategy, round_bytes, checks)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert got[cap:].tolist() == [GUARD] * 32, "bytes behind dst_cap were written"
    offs = offsets.cpu().tolist()
    return offs, [v & 0xffffffff for v in checks.cpu().tolist()], got[:min(offs[-1], cap)].tobytes()


# ---- 1. the same bytes as the in-front path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dict_len", DICT_LENS)
def test_same_bytes_as_the_window_in_front(mods, corpus, dict_len):
    zr, dfl, inf = mods
    D = corpus["dicts"][dict_len]
    window = D[-32768:]
    msgs = _streams(D, corpus)
    assert 35 <= len(msgs) <= 45 and len(msgs[4]) == 1024 - len(window) % 1024
    shared, front = _Batch(dfl, msgs), _Batch(dfl, msgs, window)
    dic = dfl.Dictionary(D)
    try:
        assert dic.window == len(window) and dic.id == zlib.adler32(D)
        for level in LEVELS:
            for strategy in STRATEGIES:
                rows, members, _ = _per_job(zr, dfl, shared, dic, 0, level, strategy)
                rows_y, members_y, _ = _per_job(zr, dfl, front, None, 0, level, strategy)
                bad = [i for i in range(len(msgs)) if rows[i] != rows_y[i] or members[i] != members_y[i]]
                assert not bad, (dict_len, level, strategy, bad, [(rows[i], rows_y[i]) for i in bad[:4]])
                assert all(r[1] == zlib.adler32(m) for r, m in zip(rows, msgs))
        # what was compared decodes (levels and strategies write the same plaintext: one reader run is enough)
        for m, c in zip(msgs, members):
            d = zlib.decompressobj(-15, zdict=D)
            assert d.decompress(c) == m and d.eof and d.unused_data == b""
        # three rounds, and the one-file form
        total = sum(len(m) for m in msgs)
        rows, members, rounds = _per_job(zr, dfl, shared, dic, 0, 6, 0, round_bytes=total // 3 + 1)
        rows_y, members_y, rounds_y = _per_job(zr, dfl, front, None, 0, 6, 0, round_bytes=total // 3 + 1)
        assert rounds == rounds_y and rounds >= 3, (rounds, rounds_y)
        assert rows == rows_y and members == members_y
        for level, strategy, rb in ((6, 0, 0), (1, 4, total // 3 + 1)):
            got, want = _file(zr, dfl, shared, dic, 0, level, strategy, rb), _file(zr, dfl, front, None, 0, level, strategy, rb)
            assert got == want, (dict_len, level, strategy, got[0][:5], want[0][:5])
            assert got[0][-1] == len(got[2]) and got[1] == [zlib.adler32(m) for m in msgs]
    finally:
        dic.close()


# ---- 2. / 3. zlib members, level 0 -------------------------------------------------------------------------------------------
def _header(level, strategy, D):
    """the first 6 bytes CPython writes with this dictionary (the CPU rule is checked against it in test_rows_dict_plan_cpu.py)"""
    return zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy, zdict=D).flush()[:6]


def _read_back(inf, dic, D, msgs, members):
    torch = torch_mod()
    for m, c in zip(msgs, members):
        d = zlib.decompressobj(15, zdict=D)
        assert d.decompress(c) == m and d.eof and d.unused_data == b""
    host, offs = _pack(members, pad=3, first=1)
    caps = [len(m) for m in msgs]
    out_off, pos = [], 7
    for c in caps:
        out_off.append(pos)
        pos += c + 9
    dst = torch.full((pos + 64,), GUARD, dtype=torch.uint8, device="cuda")
    b = inf.InflateDevBatch(torch.from_numpy(host).cuda(), offs, [len(x) for x in members], dst, out_off, caps)
    b.run_dict(1, dic)
    got = dst.cpu().numpy()
    for m, c, r, o in zip(msgs, members, b.results.cpu().tolist(), out_off):
        assert (r[2], r[0], r[1], r[3]) == (1, len(m), len(c), 0), r           # status, out_len, in_used = the member's length
        assert got[o:o + len(m)].tobytes() == m


@pytest.mark.parametrize("dict_len", (2050, 50000))
def test_zlib_members(mods, corpus, dict_len):
    zr, dfl, inf = mods
    D = corpus["dicts"][dict_len]
    msgs = _streams(D, corpus)[:14]
    shared = _Batch(dfl, msgs)
    dic = dfl.Dictionary(D)
    try:
        for level, strategy in ((1, 0), (6, 0), (9, 0), (-1, 1), (6, 4)):
            rows0, raw, _ = _per_job(zr, dfl, shared, dic, 0, level, strategy)
            rows, members, _ = _per_job(zr, dfl, shared, dic, 1, level, strategy)
            head = _header(level, strategy, D)
            assert head[1] & 0x20 and head[2:] == struct.pack(">I", zlib.adler32(D))
            for m, c, r, c0, r0 in zip(msgs, members, rows, raw, rows0):
                assert c == head + c0 + struct.pack(">I", zlib.adler32(m))
                assert r == [len(c0) + 10, zlib.adler32(m)] and r0 == [len(c0), zlib.adler32(m)]
            _read_back(inf, dic, D, msgs, members)
        offs, checks, data = _file(zr, dfl, shared, dic, 1, 6, 0)
        assert [data[a:b] for a, b in zip(offs, offs[1:])] == _per_job(zr, dfl, shared, dic, 1, 6, 0)[1]
        assert checks == [zlib.adler32(m) for m in msgs]
    finally:
        dic.close()


def test_level_0_is_stored_blocks_behind_the_fdict_header(mods, corpus):
    zr, dfl, inf = mods
    D = corpus["dicts"][2050]
    msgs = [b"", b"q", corpus["long"][:1000], corpus["long"][:65535], corpus["long"][:65536 + 300]]
    shared = _Batch(dfl, msgs)
    dic = dfl.Dictionary(D)
    try:
        rows, members, _ = _per_job(zr, dfl, shared, dic, 1, 0, 0)
        head = _header(0, 0, D)
        for m, c, r in zip(msgs, members, rows):
            blocks = [m[i:i + 65535] for i in range(0, len(m), 65535)] or [b""]
            body = b"".join(bytes([1 if k + 1 == len(blocks) else 0]) + struct.pack("<HH", len(b), len(b) ^ 0xffff) + b
                            for k, b in enumerate(blocks))
            assert c == head + body + struct.pack(">I", zlib.adler32(m))
            assert r == [len(c), zlib.adler32(m)]
        _read_back(inf, dic, D, msgs, members)
        assert _per_job(zr, dfl, shared, dic, 0, 0, 4)[1] == [c[6:-4] for c in members]
    finally:
        dic.close()


# ---- 4. the dictionary is used -----------------------------------------------------------------------------------------------
def test_dictionary_matches_on_random_bytes(mods):
    zr, dfl, inf = mods
    D = np.random.default_rng(404).integers(0, 256, size=32768, dtype=np.uint8).tobytes()
    msgs = [D[-1500:-500], D[-9000:-8000], D[-32000:-31000]]              # (within MAX_DIST = 32768 - 262 of the plaintext)
    dic = dfl.Dictionary(D)
    try:
        rows, members, _ = _per_job(zr, dfl, _Batch(dfl, msgs), dic, 0, 6, 0)
    finally:
        dic.close()
    for m, c, r in zip(msgs, members, rows):
        print("random bytes: %d -> %d at level 6 with the dictionary" % (len(m), r[0]))
        assert zlib.decompressobj(-15, zdict=D).decompress(c) == m
        assert r[0] < 250, (r[0], len(m))                                     # the bound of the level-1 test: a quarter


def test_dictionary_gain_on_records(mods, corpus):
    """On this set the device's level 6 goes from 94 733 to 51 034 bytes with the dictionary: 0.997 of CPython's level-6 gain
    (g = 0.463); the level-1 dictionary call writes 70 978."""
    zr, dfl, inf = mods
    torch = torch_mod()
    D, msgs = corpus["record_dict"], corpus["records"]
    assert len(msgs) == 200 and all(200 <= len(m) <= 2000 for m in msgs)

    def level6(m, zdict):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, zdict=zdict) if zdict else zlib.compressobj(6, zlib.DEFLATED, -15)
        return len(c.compress(m) + c.flush())
    g = 1.0 - sum(level6(m, D) for m in msgs) / sum(level6(m, None) for m in msgs)
    shared = _Batch(dfl, msgs)
    without, _, _ = _per_job(zr, dfl, shared, None, 0, 6, 0)
    dic = dfl.Dictionary(D)
    try:
        rows, members, _ = _per_job(zr, dfl, shared, dic, 0, 6, 0)
        # the level-1 dictionary call over the same records
        host, offs = _pack(msgs, pad=5, first=3)
        wb = dfl.WrappedBatch(torch.from_numpy(host).cuda(), offs, [len(m) for m in msgs], 0, for_dict=True)
        wb.run_dict(dic)
        torch.cuda.synchronize()
        t_l1 = sum(int(v) & 0xffffffff for v in wb.results.cpu()[:, 0].tolist())
    finally:
        dic.close()
    for m, c in zip(msgs, members):
        assert zlib.decompressobj(-15, zdict=D).decompress(c) == m
    t0, t1 = sum(r[0] for r in without), sum(r[0] for r in rows)
    gain = 1.0 - t1 / t0
    print("records: %d bytes; device level 6 %d -> %d with the dictionary (gain %.3f, %.3f of CPython's level-6 gain g = %.3f); "
          "level-1 dictionary call %d" % (sum(len(m) for m in msgs), t0, t1, gain, gain / g, g, t_l1))
    assert g > 0.05                                                           # the set is one a dictionary helps
    assert t1 <= t0 * (1.0 - g / 2.0), (t0, t1, g)
    assert t1 < t_l1, (t1, t_l1)


# ---- 5. refusals and the object's life ---------------------------------------------------------------------------------------
def _raw_calls(zr, dfl, dic_handle, fmt, level=6, strategy=0, dict_len=0, flags=0, cap_short=0):
    """both calls through ctypes with one small job; returns their return values and whether any output was touched"""
    torch = torch_mod()
    lib = zr.lib()
    src = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    res = torch.full((4,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    offs = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    j = (dfl.StreamJob * 1)()
    j[0].in_ptr, j[0].out_ptr, j[0].in_len = src.data_ptr() + 2048, dst.data_ptr(), 100
    j[0].out_cap = (lib.zng_rocm_compress_streams2_dict_bound(100, fmt) or 4096) - cap_short
    j[0].dict_len, j[0].flags = dict_len, flags
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc_s = lib.zng_rocm_compress_streams2_dict_dev(fmt, level, strategy, dic_handle, C.byref(j), 1, 0, C.c_void_p(res.data_ptr()), st)
    rc_m = lib.zng_rocm_compress_members_dict_dev(fmt, level, strategy, dic_handle, C.byref(j), 1, C.c_void_p(dst.data_ptr() + 4096), 4096,
                                                  0, C.c_void_p(offs.data_ptr()), None, st)
    torch.cuda.synchronize()
    clean = res.cpu().tolist() == [0x5a5a5a5a] * 4 and offs.cpu().tolist() == [-1, -1] and not dst.cpu().numpy().any()
    return rc_s, rc_m, clean


def test_refusals(mods, corpus):
    zr, dfl, inf = mods
    lib = zr.lib()
    for n in (0, 1, 1000, 131073):
        assert lib.zng_rocm_compress_streams2_dict_bound(n, 0) == lib.zng_rocm_compress_streams2_bound(n, 0)
        assert lib.zng_rocm_compress_streams2_dict_bound(n, 1) == lib.zng_rocm_compress_streams2_bound(n, 1) + 4
        assert lib.zng_rocm_compress_streams2_dict_bound(n, 2) == 0 and lib.zng_rocm_compress_streams2_dict_bound(n, -1) == 0
    dic = dfl.Dictionary(corpus["dicts"][257])
    try:
        assert _raw_calls(zr, dfl, dic.h, 2) == (-3, -3, True)                  # gzip has no dictionary
        assert _raw_calls(zr, dfl, None, 0) == (-3, -3, True)                   # no object
        assert _raw_calls(zr, dfl, None, 1) == (-3, -3, True)
        assert _raw_calls(zr, dfl, dic.h, 0, strategy=2) == (-3, -3, True)      # Z_HUFFMAN_ONLY, Z_RLE: no dictionary form
        assert _raw_calls(zr, dfl, dic.h, 1, strategy=3) == (-3, -3, True)
        assert _raw_calls(zr, dfl, dic.h, 0, level=10) == (-3, -3, True)
        assert _raw_calls(zr, dfl, dic.h, 0, dict_len=16) == (-3, -3, True)     # the history is the object's
        assert _raw_calls(zr, dfl, dic.h, 1, flags=1) == (-3, -3, True)         # block flags: raw streams only
        assert _raw_calls(zr, dfl, dic.h, 0, flags=3)[:2] == (0, 0)             # ... where they are taken
        rc_s, rc_m, _ = _raw_calls(zr, dfl, dic.h, 1, cap_short=1)              # out_cap below the new bound: streams2 only
        assert (rc_s, rc_m) == (-5, 0)
        assert _raw_calls(zr, dfl, dic.h, 1)[:2] == (0, 0)
    finally:
        dic.close()


def test_level_1_dictionary_call_unchanged(mods, corpus):
    """zng_rocm_compress_streams_dict_dev writes what the in-front level-1 path writes (zng_rocm_compress_streams_dev over copies
    with the window in front).  The two differ by rule in two places, which the batch stays clear of: the dictionary form cuts
    a match whose source runs across the window's end -- the window ends with a byte no message holds, so no such match exists
    --, and it leaves the window's last three positions out of the head table, whose strings reach into the plaintext -- the
    messages are those of the pool none of whose own strings falls into a bucket these three entries occupy.  W is a multiple
    of the level-1 batch (256), so both paths cut the plaintext into the same batches."""
    zr, dfl, inf = mods
    torch = torch_mod()
    lib = zr.lib()
    window = (corpus["record_dict"][-4095:] + b"\xff")
    W = len(window)

    def bucket(four):
        return ((int.from_bytes(four, "little") * 2654435761) & 0xffffffff) >> 20       # dict_hash, dict_plan.h

    msgs = []
    for m in _records(120, seed=41, lo=300, hi=1500):
        joined = window[-3:] + m
        extra = {bucket(joined[k:k + 4]) for k in range(3)}
        if not extra & {bucket(m[k:k + 4]) for k in range(len(m) - 3)}:
            msgs.append(m)
    assert len(msgs) >= 30, len(msgs)
    msgs = msgs[:40]
    dic = dfl.Dictionary(window)
    try:
        host, offs = _pack(msgs, pad=5, first=3)
        wb = dfl.WrappedBatch(torch.from_numpy(host).cuda(), offs, [len(m) for m in msgs], 0, for_dict=True)
        wb.run_dict(dic)
        torch.cuda.synchronize()
        res = wb.results.cpu()
        got = [wb.compressed(i, res) for i in range(len(msgs))]
    finally:
        dic.close()
    front = _Batch(dfl, msgs, window)
    bounds = [(lib.zng_rocm_compress_streams_bound(len(m), 0) + 15) & ~15 for m in msgs]
    dst = torch.zeros(sum(bounds) + 16, dtype=torch.uint8, device="cuda")
    jobs, _, _ = front.jobs(None)
    pos = 0
    for i, b in enumerate(bounds):
        jobs[i].out_ptr, jobs[i].out_cap = dst.data_ptr() + pos, b
        pos += b
    res_y = torch.zeros((len(msgs), 2), dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.zng_rocm_compress_streams_dev(0, C.byref(jobs), len(msgs), C.c_void_p(res_y.data_ptr()), st) == 0
    torch.cuda.synchronize()
    out, pos = dst.cpu().numpy(), 0
    for i, b in enumerate(bounds):
        n = int(res_y[i, 0])
        assert got[i] == out[pos:pos + n].tobytes(), i
        assert int(res[i, 1]) == int(res_y[i, 1])
        assert zlib.decompressobj(-15, zdict=window).decompress(got[i]) == msgs[i]
        pos += b


def test_dictionary_after_shutdown(mods, corpus):
    """runs last in this file: the context goes away under a live object and comes back"""
    zr, dfl, inf = mods
    D = corpus["dicts"][257]
    dic = dfl.Dictionary(D)
    assert _raw_calls(zr, dfl, dic.h, 0)[:2] == (0, 0)
    torch_mod().cuda.synchronize()
    assert zr.lib().zng_rocm_shutdown() == 0
    try:
        assert _raw_calls(zr, dfl, dic.h, 0) == (-1, -1, True)
        assert _raw_calls(zr, dfl, None, 0) == (-3, -3, True)                   # the argument refusals come first
    finally:
        zr.init()
    assert _raw_calls(zr, dfl, dic.h, 0) == (-1, -1, True)                      # an object of the context that is gone
    assert _raw_calls(zr, dfl, dic.h, 1) == (-1, -1, True)
    dic.close()                                                                 # ... is still freed without trouble
    fresh = dfl.Dictionary(D)
    try:
        m = D[10:200]
        rows, members, _ = _per_job(zr, dfl, _Batch(dfl, [m]), fresh, 1, 6, 0)
        assert zlib.decompressobj(15, zdict=D).decompress(members[0]) == m
    finally:
        fresh.close()
