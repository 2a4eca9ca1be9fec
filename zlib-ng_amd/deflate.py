"""Host mirror of the multi-stream deflate path of include/zng_rocm.h.

`deflate_quick_batch` compresses many independent streams (pigz-style, BASELINE.json configs[4]) that are
already resident in HBM; names follow the reference (`deflateBound`-style bound, level-1 = deflate_quick,
deflate.c:142-168)."""
import ctypes as C

from . import rocm


class StreamJob(C.Structure):
    """zng_rocm_stream_job"""
    _fields_ = [("in_ptr", C.c_void_p), ("out_ptr", C.c_void_p), ("in_len", C.c_uint32), ("out_cap", C.c_uint32),
                ("dict_len", C.c_uint32), ("flags", C.c_uint32)]


BLOCK_NOT_FINAL, BLOCK_SYNC_FLUSH = 1, 2


def deflate_quick_bound(n):
    return rocm.lib().zng_rocm_deflate_quick_bound(n)


class QuickBatch:
    """A fixed set of streams laid out in two device tensors.

    src:  uint8 CUDA tensor holding the streams; stream i = src[in_off[i] : in_off[i] + in_len[i]] at any
          in_off (no alignment, no padding behind a stream: zng_rocm.h), its dict_len[i] bytes of history
          directly in front of it.  What else lies around a stream is never looked at.
    The compressed streams land in `dst` at out_off[i] (bound-sized slots, 4-byte aligned); `results` is an int32
    CUDA tensor [n, 2] = {compressed length, adler32 of the input}.
    """

    def __init__(self, src, in_off, in_len, dict_len=None, flags=None):
        """dict_len[i] bytes in front of stream i (inside `src`) prime its hash; flags[i] = BLOCK_* bits"""
        import torch
        rocm._need_init()
        self.src = src
        self.n = len(in_len)
        self.in_off = [int(v) for v in in_off]
        self.in_len = [int(v) for v in in_len]
        self.bounds = [deflate_quick_bound(v) for v in self.in_len]
        self.out_off = [0] * self.n
        total = 0
        for i, b in enumerate(self.bounds):
            self.out_off[i] = total
            total += b
        self.dst = torch.empty(max(total, 16), dtype=torch.uint8, device=src.device)
        self.results = torch.zeros((self.n, 2), dtype=torch.int32, device=src.device)
        jobs = (StreamJob * self.n)()
        base_in, base_out = src.data_ptr(), self.dst.data_ptr()
        for i in range(self.n):
            jobs[i].dict_len = 0 if dict_len is None else int(dict_len[i])
            jobs[i].flags = 0 if flags is None else int(flags[i])
            if jobs[i].dict_len > self.in_off[i]:
                raise ValueError("the dictionary must lie inside src, in front of the stream")
            jobs[i].in_ptr = base_in + self.in_off[i]
            jobs[i].out_ptr = base_out + self.out_off[i]
            jobs[i].in_len = self.in_len[i]
            jobs[i].out_cap = self.bounds[i]
        self.jobs = jobs

    def run(self, stream=None):
        """asynchronous on `stream`: K1 match/parse + K2 static-Huffman emit for every stream"""
        rocm._check(rocm.lib().zng_rocm_deflate_quick_dev(C.byref(self.jobs), self.n, rocm._dev_ptr(self.results),
                                                          rocm._stream_ptr(stream)), "zng_rocm_deflate_quick_dev")

    def compressed(self, i, results_host=None):
        """bytes of stream i (synchronises)"""
        res = self.results.cpu() if results_host is None else results_host
        clen = int(res[i, 0])
        o = self.out_off[i]
        return self.dst[o:o + clen].cpu().numpy().tobytes()


class Dictionary:
    """zng_rocm_dict: one preset dictionary prepared once on the device (DICTID, window, the primed tables of the level-1 class and
    of the rows engine) and shared by every stream of WrappedBatch.run_dict / InflateDevBatch.run_dict / compress_streams2_dict_dev.  `data`: uint8 CUDA tensor (or bytes, copied to the
    device first).  .id = Adler-32 of all of it, .window = min(len, 32768).  close() frees the object."""

    def __init__(self, data, stream=None):
        import numpy as np
        import torch
        rocm._need_init()
        if not isinstance(data, torch.Tensor):
            data = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to("cuda")
        self.h = C.c_void_p()
        rocm._check(rocm.lib().zng_rocm_dict_create_dev(rocm._dev_ptr(data) if data.numel() else None, int(data.numel()),
                                                        C.byref(self.h), rocm._stream_ptr(stream)), "zng_rocm_dict_create_dev")
        self.id = int(rocm.lib().zng_rocm_dict_id(self.h))
        self.window = int(rocm.lib().zng_rocm_dict_window(self.h))

    def close(self):
        if self.h:
            rocm.lib().zng_rocm_dict_destroy(self.h)
            self.h = C.c_void_p()


class WrappedBatch:
    """zng_rocm_compress_streams_dev: many streams, level-1 class, with their zlib (fmt 1) / gzip (fmt 2) wrapper written on
    the device.  Layout as QuickBatch; results: int32 CUDA tensor [n, 2] = {total bytes, check value}."""

    def __init__(self, src, in_off, in_len, fmt, for_dict=False):
        """for_dict: slots sized by zng_rocm_compress_streams_dict_bound (the 16-byte wrapper), for run_dict"""
        import torch
        rocm._need_init()
        self.src, self.fmt = src, fmt
        self.n = len(in_len)
        bound = rocm.lib().zng_rocm_compress_streams_dict_bound if for_dict else rocm.lib().zng_rocm_compress_streams_bound
        self.bounds = [(bound(int(v), fmt) + 15) & ~15 for v in in_len]
        self.out_off, total = [], 0
        for b in self.bounds:
            self.out_off.append(total)
            total += b
        self.dst = torch.zeros(max(total, 16), dtype=torch.uint8, device=src.device)
        self.results = torch.zeros((self.n, 2), dtype=torch.int32, device=src.device)
        self.jobs = (StreamJob * self.n)()
        bi, bo = src.data_ptr(), self.dst.data_ptr()
        for i in range(self.n):
            self.jobs[i].in_ptr = bi + int(in_off[i])
            self.jobs[i].out_ptr = bo + self.out_off[i]
            self.jobs[i].in_len = int(in_len[i])
            self.jobs[i].out_cap = self.bounds[i]
            self.jobs[i].dict_len = 0
            self.jobs[i].flags = 0

    def run(self, stream=None):
        rocm._check(rocm.lib().zng_rocm_compress_streams_dev(self.fmt, C.byref(self.jobs), self.n, rocm._dev_ptr(self.results),
                                                             rocm._stream_ptr(stream)), "zng_rocm_compress_streams_dev")

    def run_dict(self, dictionary, stream=None):
        """the same streams against a shared preset Dictionary (fmt 0 raw, 1 zlib with FDICT / DICTID):
        zng_rocm_compress_streams_dict_dev.  The batch must have been made with for_dict=True."""
        rocm._check(rocm.lib().zng_rocm_compress_streams_dict_dev(self.fmt, dictionary.h, C.byref(self.jobs), self.n,
                                                                  rocm._dev_ptr(self.results), rocm._stream_ptr(stream)),
                    "zng_rocm_compress_streams_dict_dev")

    def compressed(self, i, results_host=None):
        res = self.results.cpu() if results_host is None else results_host
        o = self.out_off[i]
        return self.dst[o:o + int(res[i, 0])].cpu().numpy().tobytes()


def deflate_bound(n):
    return rocm.lib().zng_rocm_deflate_bound(n)


class StreamsBatch:
    """Many independent device-resident streams at a chain level (zng_rocm_deflate_streams_dev).  Layout as QuickBatch:
    stream i = src[in_off[i] : in_off[i] + in_len[i]] with dict_len[i] bytes of history in front of it; the compressed
    streams land in `dst` at out_off[i] (bound-sized slots); run() returns the list of compressed lengths."""

    def __init__(self, src, in_off, in_len, dict_len=None, flags=None):
        import torch
        rocm._need_init()
        self.src = src
        self.n = len(in_len)
        self.in_len = [int(v) for v in in_len]
        self.bounds = [(deflate_bound(v) + 15) & ~15 for v in self.in_len]
        self.out_off, total = [], 0
        for b in self.bounds:
            self.out_off.append(total)
            total += b
        self.dst = torch.empty(max(total, 16), dtype=torch.uint8, device=src.device)
        self.jobs = (StreamJob * self.n)()
        bi, bo = src.data_ptr(), self.dst.data_ptr()
        for i in range(self.n):
            self.jobs[i].dict_len = 0 if dict_len is None else int(dict_len[i])
            self.jobs[i].flags = 0 if flags is None else int(flags[i])
            if self.jobs[i].dict_len > int(in_off[i]):
                raise ValueError("the dictionary must lie inside src, in front of the stream")
            self.jobs[i].in_ptr = bi + int(in_off[i])
            self.jobs[i].out_ptr = bo + self.out_off[i]
            self.jobs[i].in_len = self.in_len[i]
            self.jobs[i].out_cap = self.bounds[i]
        self.out_lens = (C.c_size_t * self.n)()

    def run(self, level=6, stream=None, strategy=0, window_bits=15):
        """strategy: zlib's (Z_DEFAULT_STRATEGY 0, Z_FILTERED 1, Z_HUFFMAN_ONLY 2, Z_RLE 3, Z_FIXED 4).  window_bits: deflateInit2's
        windowBits, 9..15 -- no match reaches further back than (1 << window_bits) - 262 (zng_rocm_deflate_window_streams_dev)"""
        if window_bits != 15:
            rc = rocm.lib().zng_rocm_deflate_window_streams_dev(level, strategy, int(window_bits), C.byref(self.jobs), self.n,
                                                                 C.byref(self.out_lens), rocm._stream_ptr(stream))
            rocm._check(rc, "zng_rocm_deflate_window_streams_dev")
        elif strategy:
            rc = rocm.lib().zng_rocm_deflate_strategy_streams_dev(level, strategy, C.byref(self.jobs), self.n,
                                                                   C.byref(self.out_lens), rocm._stream_ptr(stream))
            rocm._check(rc, "zng_rocm_deflate_strategy_streams_dev")
        else:
            rocm._check(rocm.lib().zng_rocm_deflate_streams_dev(level, C.byref(self.jobs), self.n, C.byref(self.out_lens),
                                                                rocm._stream_ptr(stream)), "zng_rocm_deflate_streams_dev")
        return [int(v) for v in self.out_lens]

    def compressed(self, i):
        o = self.out_off[i]
        return self.dst[o:o + int(self.out_lens[i])].cpu().numpy().tobytes()


def deflate_dev(src, level=6, length=None, offset=0, stream=None, dict_len=0, flags=0, strategy=0, window_bits=15):
    """one large device-resident stream (or, with dict_len / flags, one BLOCK of a longer stream whose dict_len
    bytes of history sit in src in front of `offset`) -> (uint8 CUDA tensor with raw deflate, compressed length).
    level 0 = stored, 1 = single probe, 2..9 = chain walk.  strategy: zlib's (0 default, 1 Z_FILTERED, 2 Z_HUFFMAN_ONLY,
    3 Z_RLE, 4 Z_FIXED; zng_rocm_deflate_strategy_block_dev).  window_bits: deflateInit2's windowBits, 9..15
    (zng_rocm_deflate_window_block_dev)."""
    import torch
    rocm._need_init()
    n = src.numel() - offset if length is None else length
    cap = deflate_bound(n)
    dst = torch.empty(cap, dtype=torch.uint8, device=src.device)
    out_len = C.c_size_t(0)
    if window_bits != 15:
        rc = rocm.lib().zng_rocm_deflate_window_block_dev(level, strategy, int(window_bits), rocm._dev_ptr(src, offset), n, dict_len,
                                                          flags, rocm._dev_ptr(dst), cap, C.byref(out_len), rocm._stream_ptr(stream))
        rocm._check(rc, "zng_rocm_deflate_window_block_dev")
    elif strategy:
        rc = rocm.lib().zng_rocm_deflate_strategy_block_dev(level, strategy, rocm._dev_ptr(src, offset), n, dict_len, flags,
                                                            rocm._dev_ptr(dst), cap, C.byref(out_len), rocm._stream_ptr(stream))
        rocm._check(rc, "zng_rocm_deflate_strategy_block_dev")
    else:
        rc = rocm.lib().zng_rocm_deflate_block_dev(level, rocm._dev_ptr(src, offset), n, dict_len, flags, rocm._dev_ptr(dst),
                                                   cap, C.byref(out_len), rocm._stream_ptr(stream))
        rocm._check(rc, "zng_rocm_deflate_block_dev")
    return dst, out_len.value


def deflate_async_dev(src, dst, result, level=6, length=None, offset=0, stream=None, dict_len=0, flags=0):
    """zng_rocm_deflate_async_dev: as deflate_dev, but nothing is synchronised -- `dst` (uint8 CUDA tensor of at least
    deflate_bound(n) bytes) and `result` (int64 CUDA tensor, 2 elements: {compressed size, does-not-fit flag}) are filled
    when `stream` gets there."""
    rocm._need_init()
    n = src.numel() - offset if length is None else length
    rocm._check(rocm.lib().zng_rocm_deflate_async_dev(level, rocm._dev_ptr(src, offset), n, dict_len, flags, rocm._dev_ptr(dst),
                                                      dst.numel(), rocm._dev_ptr(result), rocm._stream_ptr(stream)),
                "zng_rocm_deflate_async_dev")


BGZF_BLOCK, BGZF_NO_EOF, BGZF_QUICK = 65280, 1, 2


def bgzf_bound(n, block_bytes=0):
    return rocm.lib().zng_rocm_bgzf_bound(int(n), int(block_bytes))


def bgzf_compress_dev(src_dev, dst, level=-1, block_bytes=0, members_cap=None, round_bytes=0, no_eof=False, quick=False,
                      flags=None, stream=None):
    """zng_rocm_bgzf_compress_dev: the uint8 CUDA tensor `src_dev` written as a BGZF file into the uint8 CUDA tensor `dst`
    (dst.numel() is dst_cap; it need not reach bgzf_bound()), one member per `block_bytes` (0 = 65280) of plaintext.
    `members_cap`: rows of the member table to take (None = all).  Returns (status, file bytes -- with status -5 the bytes the
    file needs --, members, nmembers, counters) with members = [(src_off, src_len, dst_off, out_len, crc, bgzf)], the rows
    gunzip_members_dev reports for the file, and counters = {"rounds", "stored"} (zng_rocm_bgzf_last_*)."""
    import numpy as np
    from .inflate import GzipMember
    rocm._need_init()
    lib = rocm.lib()
    n, bb = int(src_dev.numel()), int(block_bytes)
    piece = bb if 0 < bb <= BGZF_BLOCK else BGZF_BLOCK
    cap = -(-n // piece) + 1 if members_cap is None else int(members_cap)
    table = np.empty(max(cap, 1) * C.sizeof(GzipMember), dtype=np.uint8)
    out_len, nmembers = C.c_uint64(0), C.c_size_t(0)
    fl = ((BGZF_NO_EOF if no_eof else 0) | (BGZF_QUICK if quick else 0)) if flags is None else int(flags)
    st = lib.zng_rocm_bgzf_compress_dev(int(level), rocm._dev_ptr(src_dev) if n else None, n, bb,
                                        rocm._dev_ptr(dst) if dst.numel() else None, int(dst.numel()), C.byref(out_len),
                                        C.c_void_p(table.ctypes.data) if cap else None, cap, C.byref(nmembers), int(round_bytes), fl,
                                        rocm._stream_ptr(stream))
    rows = [(int(m.src_off), int(m.src_len), int(m.dst_off), int(m.out_len), int(m.crc), int(m.bgzf))
            for m in (GzipMember * min(cap, int(nmembers.value))).from_buffer(table)]
    counters = {"rounds": int(lib.zng_rocm_bgzf_last_rounds()), "stored": int(lib.zng_rocm_bgzf_last_stored())}
    return st, int(out_len.value), rows, int(nmembers.value), counters


def compress_streams2_bound(n, fmt):
    return rocm.lib().zng_rocm_compress_streams2_bound(int(n), int(fmt))


def stream_jobs(srcs, dsts=None, dict_len=None, flags=None):
    """zng_rocm_stream_job[] for the two calls below: srcs[i] a uint8 CUDA tensor (a view at any address; its dict_len[i] bytes
    of history lie in front of it in the same storage), dsts[i] the buffer of member i (None: out / out_cap stay 0, as
    compress_members_dev wants them)."""
    jobs = (StreamJob * max(len(srcs), 1))()
    for i, s in enumerate(srcs):
        jobs[i].in_ptr = s.data_ptr() if s.numel() else None
        jobs[i].in_len = int(s.numel())
        if dsts is not None:
            jobs[i].out_ptr = dsts[i].data_ptr()
            jobs[i].out_cap = int(dsts[i].numel())
        jobs[i].dict_len = 0 if dict_len is None else int(dict_len[i])
        jobs[i].flags = 0 if flags is None else int(flags[i])
    return jobs


def compress_streams2_dev(jobs, njobs, results, fmt, level=-1, strategy=0, round_bytes=0, stream=None, window_bits=15):
    """zng_rocm_compress_streams2_dev: every job deflated at `level` (-1 = 6, 0..9) and `strategy` (0..4) and wrapped (fmt 0 raw,
    1 zlib, 2 gzip) into its own buffer; `results` an int32 CUDA tensor [njobs, 2] = {bytes written, check value}, valid once
    `stream` has got there.  window_bits: deflateInit2's windowBits, 9..15 (8 for fmt 1: taken as 9);
    zng_rocm_compress_streams2_window_dev when it is not 15.  Returns the status (0, ZNG_ROCM_E*, -5)."""
    rocm._need_init()
    if window_bits != 15:
        return rocm.lib().zng_rocm_compress_streams2_window_dev(int(fmt), int(level), int(strategy), int(window_bits), C.byref(jobs),
                                                                int(njobs), int(round_bytes),
                                                                rocm._dev_ptr(results) if results is not None else None,
                                                                rocm._stream_ptr(stream))
    return rocm.lib().zng_rocm_compress_streams2_dev(int(fmt), int(level), int(strategy), C.byref(jobs), int(njobs), int(round_bytes),
                                                     rocm._dev_ptr(results) if results is not None else None, rocm._stream_ptr(stream))


def compress_members_dev(jobs, njobs, dst, offsets, fmt, level=-1, strategy=0, round_bytes=0, checks=None, stream=None,
                         window_bits=15):
    """zng_rocm_compress_members_dev: the members back to back in the uint8 CUDA tensor `dst` (dst.numel() is dst_cap; None: no
    destination); `offsets` an int64 CUDA tensor of njobs + 1 (member starts, then the file's length -- above dst_cap when the
    file did not fit), `checks` an int32 CUDA tensor of njobs or None.  window_bits as compress_streams2_dev
    (zng_rocm_compress_members_window_dev when it is not 15).  Returns the status."""
    rocm._need_init()
    cap = int(dst.numel()) if dst is not None else 0
    if window_bits != 15:
        return rocm.lib().zng_rocm_compress_members_window_dev(int(fmt), int(level), int(strategy), int(window_bits), C.byref(jobs),
                                                               int(njobs), rocm._dev_ptr(dst) if cap else None, cap, int(round_bytes),
                                                               rocm._dev_ptr(offsets) if offsets is not None else None,
                                                               rocm._dev_ptr(checks) if checks is not None else None,
                                                               rocm._stream_ptr(stream))
    return rocm.lib().zng_rocm_compress_members_dev(int(fmt), int(level), int(strategy), C.byref(jobs), int(njobs),
                                                    rocm._dev_ptr(dst) if cap else None, cap, int(round_bytes),
                                                    rocm._dev_ptr(offsets) if offsets is not None else None,
                                                    rocm._dev_ptr(checks) if checks is not None else None, rocm._stream_ptr(stream))


class GzipHeader(C.Structure):
    """zng_rocm_gzip_header: deflateSetHeader's fields for one member; make() builds one from Python values"""
    _fields_ = [("time", C.c_uint32), ("os", C.c_uint32), ("text", C.c_uint32), ("hcrc", C.c_uint32), ("extra", C.c_void_p),
                ("name", C.c_void_p), ("comment", C.c_void_p), ("extra_len", C.c_uint32), ("reserved", C.c_uint32)]

    @classmethod
    def make(cls, time=0, os=3, text=False, hcrc=False, extra=None, name=None, comment=None):
        """extra / name / comment: bytes or None (the field is absent); name and comment without their terminator"""
        h = cls(int(time), int(os), int(bool(text)), int(bool(hcrc)), None, None, None, 0, 0)
        h.set_fields(extra, name, comment)
        return h

    def set_fields(self, extra, name, comment):
        self._keep = [None if v is None else C.create_string_buffer(bytes(v), len(v) + 1) for v in (extra, name, comment)]
        self.extra, self.name, self.comment = (None if k is None else C.addressof(k) for k in self._keep)
        self.extra_len = 0 if extra is None else len(extra)


def gzip_headers(heads):
    """a ctypes array of zng_rocm_gzip_header from GzipHeader objects (their buffers stay alive with the array)"""
    arr = (GzipHeader * max(len(heads), 1))()
    arr._keep = list(heads)
    for i, h in enumerate(heads):
        C.memmove(C.byref(arr, i * C.sizeof(GzipHeader)), C.byref(h), C.sizeof(GzipHeader))
    return arr


def gzip_header_bytes(head):
    """zng_rocm_gzip_header_bytes: the rendered length of a GzipHeader (None: the canonical 10 bytes); 0 for a refused one"""
    return int(rocm.lib().zng_rocm_gzip_header_bytes(C.byref(head) if head is not None else None))


def gzip_header_write(head, level=-1, strategy=0):
    """zng_rocm_gzip_header_write: the header bytes deflate.c:923-1020 write for these fields, on the host (no device needed);
    b"" for a refused header, level or strategy"""
    n = gzip_header_bytes(head)
    buf = (C.c_uint8 * max(n, 1))()
    got = rocm.lib().zng_rocm_gzip_header_write(C.byref(head) if head is not None else None, int(level), int(strategy), buf, n)
    return bytes(buf)[:got]


def compress_streams2_header_dev(jobs, heads, njobs, results, level=-1, strategy=0, round_bytes=0, stream=None, window_bits=15):
    """zng_rocm_compress_streams2_header_dev: compress_streams2_dev(fmt 2) with a gzip header per member; `heads` a gzip_headers()
    array or None (exactly the call without headers).  Returns the status."""
    rocm._need_init()
    return rocm.lib().zng_rocm_compress_streams2_header_dev(int(level), int(strategy), int(window_bits), C.byref(jobs),
                                                            C.byref(heads) if heads is not None else None, int(njobs),
                                                            int(round_bytes), rocm._dev_ptr(results) if results is not None else None,
                                                            rocm._stream_ptr(stream))


def compress_members_header_dev(jobs, heads, njobs, dst, offsets, level=-1, strategy=0, round_bytes=0, checks=None, stream=None,
                                window_bits=15):
    """zng_rocm_compress_members_header_dev: compress_members_dev(fmt 2) with a gzip header per member -- name, mtime, comment,
    FEXTRA subfields, header CRC (deflateSetHeader) --; `heads` a gzip_headers() array or None.  Returns the status."""
    rocm._need_init()
    cap = int(dst.numel()) if dst is not None else 0
    return rocm.lib().zng_rocm_compress_members_header_dev(int(level), int(strategy), int(window_bits), C.byref(jobs),
                                                           C.byref(heads) if heads is not None else None, int(njobs),
                                                           rocm._dev_ptr(dst) if cap else None, cap, int(round_bytes),
                                                           rocm._dev_ptr(offsets) if offsets is not None else None,
                                                           rocm._dev_ptr(checks) if checks is not None else None,
                                                           rocm._stream_ptr(stream))


def compress_streams2_dict_bound(n, fmt):
    return rocm.lib().zng_rocm_compress_streams2_dict_bound(int(n), int(fmt))


def compress_streams2_dict_dev(dictionary, jobs, njobs, results, fmt, level=-1, strategy=0, round_bytes=0, stream=None):
    """zng_rocm_compress_streams2_dict_dev: compress_streams2_dev with the Dictionary's window as every stream's history (fmt 0
    raw, 1 zlib with the 6-byte FDICT header; strategy 0, 1 or 4; a job has no dict_len of its own).  `dictionary` may be None
    (the call refuses it).  Returns the status."""
    rocm._need_init()
    return rocm.lib().zng_rocm_compress_streams2_dict_dev(int(fmt), int(level), int(strategy), dictionary.h if dictionary is not None else None,
                                                          C.byref(jobs), int(njobs), int(round_bytes),
                                                          rocm._dev_ptr(results) if results is not None else None, rocm._stream_ptr(stream))


def compress_members_dict_dev(dictionary, jobs, njobs, dst, offsets, fmt, level=-1, strategy=0, round_bytes=0, checks=None, stream=None):
    """zng_rocm_compress_members_dict_dev: compress_members_dev with the Dictionary's window as every stream's history."""
    rocm._need_init()
    cap = int(dst.numel()) if dst is not None else 0
    return rocm.lib().zng_rocm_compress_members_dict_dev(int(fmt), int(level), int(strategy), dictionary.h if dictionary is not None else None,
                                                         C.byref(jobs), int(njobs), rocm._dev_ptr(dst) if cap else None, cap, int(round_bytes),
                                                         rocm._dev_ptr(offsets) if offsets is not None else None,
                                                         rocm._dev_ptr(checks) if checks is not None else None, rocm._stream_ptr(stream))


def compress_streams2_last_rounds():
    return int(rocm.lib().zng_rocm_compress_streams2_last_rounds())
