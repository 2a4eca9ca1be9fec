"""Host mirror of the inflate path of include/zng_rocm.h (token decode on the host, copy
resolution on the device).  Names follow the reference's API: `inflate_raw` is a one-shot
`zng_inflate` of a raw (windowBits < 0) stream, Z_* codes as in zlib-ng.h.in:180-188."""
import ctypes as C

from . import rocm

Z_OK, Z_STREAM_END, Z_DATA_ERROR, Z_MEM_ERROR, Z_BUF_ERROR = 0, 1, -3, -4, -5


class InflateTokens(C.Structure):
    """zng_rocm_inflate_tokens"""
    _fields_ = [
        ("tokens", C.POINTER(C.c_uint32)), ("ntokens", C.c_size_t),
        ("literals", C.POINTER(C.c_uint8)), ("nliterals", C.c_size_t),
        ("segs", C.POINTER(C.c_uint64)), ("nsegs", C.c_size_t),
        ("out_len", C.c_uint64), ("in_used", C.c_size_t),
        ("status", C.c_int), ("msg", C.c_char_p),
    ]


class DecodedStream:
    """numpy views of one decoded stream (copies; the C buffers are freed immediately)"""

    def __init__(self, src, window_len=0, nthreads=1, start_bit=None):
        import numpy as np
        lib = rocm.lib()
        raw = bytes(src)
        buf = C.create_string_buffer(raw, max(len(raw), 1))
        tk = InflateTokens()
        self.end_bit = None
        if start_bit is not None:
            end_bit = C.c_uint64(0)
            self.status = lib.zng_rocm_inflate_tokens_decode_blocks(C.addressof(buf), len(raw), start_bit, window_len,
                                                                    C.byref(tk), C.byref(end_bit))
            self.end_bit = int(end_bit.value)
        elif nthreads == 1:
            self.status = lib.zng_rocm_inflate_tokens_decode_window(C.addressof(buf), len(raw), window_len, C.byref(tk))
        else:
            self.status = lib.zng_rocm_inflate_tokens_decode_threads(C.addressof(buf), len(raw), window_len, nthreads,
                                                                     C.byref(tk))
        self.msg = (tk.msg or b"").decode()
        self.out_len = tk.out_len
        self.in_used = tk.in_used
        self.tokens = np.ctypeslib.as_array(tk.tokens, shape=(tk.ntokens,)).copy() if tk.ntokens else \
            np.zeros(0, dtype=np.uint32)
        self.literals = np.ctypeslib.as_array(tk.literals, shape=(tk.nliterals,)).copy() if tk.nliterals else \
            np.zeros(0, dtype=np.uint8)
        nseg = tk.nsegs
        self.nsegs = nseg
        self.segs = np.ctypeslib.as_array(tk.segs, shape=((nseg + 1) * 3,)).copy() if tk.segs else \
            np.zeros(3, dtype=np.uint64)
        lib.zng_rocm_inflate_tokens_free(C.byref(tk))


def decode_tokens(src, window_len=0, nthreads=1):
    """nthreads != 1: the multi-threaded decode of ONE stream (0 = one thread per hardware thread)"""
    return DecodedStream(src, window_len, nthreads)


def decode_blocks(src, start_bit=0, window_len=0):
    """zng_rocm_inflate_tokens_decode_blocks: every COMPLETE block from bit `start_bit` on; .status 1 (BFINAL decoded) / 0
    (input ends inside a block) / -3, .end_bit = where the delivered blocks end"""
    return DecodedStream(src, window_len, start_bit=start_bit)


class InflateHook:
    """the device side of the streaming inflate hook (zng_rocm_hook_*): history in HBM across calls"""

    def __init__(self):
        rocm._need_init()
        self.lib = rocm.lib()
        self.h = C.c_void_p()
        rocm._check(self.lib.zng_rocm_hook_create(C.byref(self.h), 1 << 20), "zng_rocm_hook_create")

    def close(self):
        if self.h:
            self.lib.zng_rocm_hook_destroy(self.h)
            self.h = C.c_void_p()

    def set_history(self, data):
        data = bytes(data)
        buf = C.create_string_buffer(data, max(len(data), 1))
        rocm._check(self.lib.zng_rocm_hook_set_history(self.h, C.addressof(buf), len(data)), "zng_rocm_hook_set_history")

    def get_history(self):
        n = C.c_uint32(0)
        buf = C.create_string_buffer(32768)
        rocm._check(self.lib.zng_rocm_hook_get_history(self.h, C.addressof(buf), C.byref(n)), "zng_rocm_hook_get_history")
        return buf.raw[:n.value]

    def clone(self):
        """zng_rocm_hook_clone: a second hook with this one's history and nothing else of it (inflateCopy / deflateCopy)"""
        other = InflateHook.__new__(InflateHook)
        other.lib = self.lib
        other.h = C.c_void_p()
        rocm._check(self.lib.zng_rocm_hook_clone(self.h, C.byref(other.h)), "zng_rocm_hook_clone")
        return other

    def inflate_blocks(self, data, start_bit=0, check=0, check_value=0):
        """zng_rocm_hook_inflate_blocks on host bytes `data` (the stream from the byte that holds bit start_bit on):
        returns (status, plaintext bytes, end_bit, check value, message)"""
        data = bytes(data)
        buf = C.create_string_buffer(data, max(len(data), 1))
        cv = C.c_uint32(check_value)
        out, out_len, end_bit, msg = C.c_void_p(), C.c_size_t(0), C.c_uint64(0), C.c_char_p()
        st = self.lib.zng_rocm_hook_inflate_blocks(self.h, C.addressof(buf), len(data), start_bit, check, C.byref(cv),
                                                   C.byref(out), C.byref(out_len), C.byref(end_bit), C.byref(msg))
        plain = C.string_at(out.value, out_len.value) if out_len.value else b""
        return st, plain, int(end_bit.value), int(cv.value), (msg.value or b"").decode()


def resolve_dev(dec, stream=None):
    """run the device stage on a DecodedStream; returns a uint8 CUDA tensor with the plaintext"""
    import numpy as np
    import torch
    rocm._need_init()
    n = int(dec.out_len)
    out = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
    if n == 0:
        return out[:0]
    d_tok = torch.from_numpy(dec.tokens.view(np.int32)).cuda()
    d_lit = torch.from_numpy(dec.literals).cuda() if dec.literals.size else torch.zeros(1, dtype=torch.uint8,
                                                                                        device="cuda")
    d_seg = torch.from_numpy(dec.segs.view(np.int64)).cuda()
    d_sym = torch.empty(n, dtype=torch.int16, device="cuda")
    rocm._check(rocm.lib().zng_rocm_inflate_resolve_dev(
        rocm._dev_ptr(d_tok), dec.tokens.size, rocm._dev_ptr(d_lit), dec.literals.size, rocm._dev_ptr(d_seg),
        dec.nsegs, rocm._dev_ptr(d_sym), rocm._dev_ptr(out), n, rocm._stream_ptr(stream)),
        "zng_rocm_inflate_resolve_dev")
    torch.cuda.current_stream().synchronize()
    return out[:n]


def resolve_arrays_dev(tokens, literals, segs, out_len, window=None, sym_shift=0, out_shift=0, guard=64, stream=None):
    """the device stage on raw arrays (numpy): tokens uint32, literals uint8, segs uint64 of (nsegs + 1) triples, as
    include/zng_rocm.h defines them.  window=None: zng_rocm_inflate_resolve_dev; a bytes-like window (it may be empty):
    zng_rocm_inflate_resolve_window_dev.  d_symbols starts `sym_shift` elements and d_out `out_shift` bytes into larger
    tensors.  Returns the whole destination tensor: out_shift + out_len + guard bytes that were filled with 0xA5 before the
    call, the plaintext at [out_shift, out_shift + out_len).  The arrays must be valid: this stage has no error channel."""
    import numpy as np
    import torch
    rocm._need_init()
    tokens = np.array(tokens, dtype=np.uint32)                      # copies: the caller's arrays may be read-only
    literals = np.array(literals, dtype=np.uint8)
    segs = np.array(segs, dtype=np.uint64).reshape(-1)
    n, nsegs = int(out_len), segs.size // 3 - 1
    dst = torch.full((int(out_shift) + n + int(guard),), 0xA5, dtype=torch.uint8, device="cuda")
    d_tok = torch.from_numpy(tokens.view(np.int32)).cuda() if tokens.size else torch.zeros(1, dtype=torch.int32, device="cuda")
    d_lit = torch.from_numpy(literals).cuda() if literals.size else torch.zeros(1, dtype=torch.uint8, device="cuda")
    d_seg = torch.from_numpy(segs.view(np.int64)).cuda()
    front = 0 if window is None else 32768
    d_sym = torch.empty(int(sym_shift) + front + n + 8, dtype=torch.int16, device="cuda")
    args = (rocm._dev_ptr(d_tok), tokens.size, rocm._dev_ptr(d_lit), literals.size, rocm._dev_ptr(d_seg), nsegs,
            rocm._dev_ptr(d_sym, 2 * int(sym_shift)), rocm._dev_ptr(dst, int(out_shift)), n)
    if window is None:
        rocm._check(rocm.lib().zng_rocm_inflate_resolve_dev(*args, rocm._stream_ptr(stream)), "zng_rocm_inflate_resolve_dev")
    else:
        w = np.frombuffer(bytes(window), dtype=np.uint8)
        d_win = torch.from_numpy(w.copy()).cuda() if w.size else None
        rocm._check(rocm.lib().zng_rocm_inflate_resolve_window_dev(*args, rocm._dev_ptr(d_win) if w.size else None, w.size,
                                                                   rocm._stream_ptr(stream)),
                    "zng_rocm_inflate_resolve_window_dev")
    torch.cuda.current_stream().synchronize()
    return dst


def inflate_raw(src, dst, stream=None):
    """one-shot: host bytes (or a HostStream, which saves the Python copy) in, plaintext into the CUDA tensor `dst`;
    returns (zlib status, bytes produced)"""
    rocm._need_init()
    hs = src if isinstance(src, HostStream) else HostStream(src)
    produced = C.c_uint64(0)
    rc = rocm.lib().zng_rocm_inflate_raw(C.addressof(hs.buf), hs.n, rocm._dev_ptr(dst), dst.numel(),
                                         C.byref(produced), rocm._stream_ptr(stream))
    return rc, produced.value


def inflate_raw_window(src, window, dst, stream=None):
    """one-shot raw inflate of a stream that continues `window` (uint8 CUDA tensor, <= 32768 bytes: a preset
    dictionary or the tail of earlier output); returns (zlib status, bytes produced, input bytes used)"""
    rocm._need_init()
    raw = bytes(src)
    buf = C.create_string_buffer(raw, max(len(raw), 1))
    produced, used = C.c_uint64(0), C.c_size_t(0)
    wl = 0 if window is None else window.numel()
    rc = rocm.lib().zng_rocm_inflate_raw_window(C.addressof(buf), len(raw), None if not wl else rocm._dev_ptr(window), wl,
                                                rocm._dev_ptr(dst), dst.numel(), C.byref(produced), C.byref(used),
                                                rocm._stream_ptr(stream))
    return rc, produced.value, used.value


class InflateJob(C.Structure):
    """zng_rocm_inflate_job"""
    _fields_ = [("src", C.c_void_p), ("src_len", C.c_size_t), ("d_dst", C.c_void_p), ("dst_cap", C.c_size_t),
                ("d_window", C.c_void_p), ("window_len", C.c_uint32), ("status", C.c_int), ("out_len", C.c_uint64),
                ("in_used", C.c_size_t), ("msg", C.c_char_p)]


class InflateBatch:
    """a prepared zng_rocm_inflate_many call: the job array and the host copies of the streams are built once"""

    def __init__(self, streams, dsts, windows=None):
        rocm._need_init()
        self.n = len(streams)
        self._keep = [C.create_string_buffer(bytes(s), max(len(s), 1)) for s in streams]
        self._dsts, self._windows = dsts, windows
        self.jobs = (InflateJob * self.n)()
        for i in range(self.n):
            self.jobs[i].src = C.addressof(self._keep[i])
            self.jobs[i].src_len = len(streams[i])
            self.jobs[i].d_dst = dsts[i].data_ptr()
            self.jobs[i].dst_cap = dsts[i].numel()
            w = None if windows is None else windows[i]
            self.jobs[i].d_window = None if w is None or not w.numel() else w.data_ptr()
            self.jobs[i].window_len = 0 if w is None else w.numel()

    def run(self, nthreads=0):
        rc = rocm.lib().zng_rocm_inflate_many(C.byref(self.jobs), self.n, nthreads)
        rocm._check(rc, "zng_rocm_inflate_many")
        return [(self.jobs[i].status, self.jobs[i].out_len, self.jobs[i].in_used, (self.jobs[i].msg or b"").decode())
                for i in range(self.n)]


def inflate_many(streams, dsts, windows=None, nthreads=0):
    """streams: list of bytes-like raw deflate streams (host); dsts: list of uint8 CUDA tensors; windows: optional list
    of uint8 CUDA tensors (or None) holding each stream's history.  Returns [(status, out_len, in_used, msg), ...]."""
    return InflateBatch(streams, dsts, windows).run(nthreads)


class HostStream:
    """a host copy of one compressed stream, made once (keeps the timing of repeated calls free of Python copies)"""

    def __init__(self, src):
        raw = bytes(src)
        self.n = len(raw)
        self.buf = C.create_string_buffer(raw, max(len(raw), 1))


def inflate_raw_threads(src, dst, window=None, nthreads=0):
    """one raw stream, host decode on `nthreads` threads (0 = all hardware threads), device resolve; `src` bytes-like or
    a HostStream.  Returns (zlib status, bytes produced, input bytes used)"""
    rocm._need_init()
    hs = src if isinstance(src, HostStream) else HostStream(src)
    produced, used = C.c_uint64(0), C.c_size_t(0)
    wl = 0 if window is None else window.numel()
    rc = rocm.lib().zng_rocm_inflate_raw_threads(C.addressof(hs.buf), hs.n, None if not wl else rocm._dev_ptr(window), wl,
                                                 rocm._dev_ptr(dst), dst.numel(), C.byref(produced), C.byref(used), nthreads)
    return rc, produced.value, used.value


class InflateDevJob(C.Structure):
    """zng_rocm_inflate_dev_job"""
    _fields_ = [("in_ptr", C.c_void_p), ("out_ptr", C.c_void_p), ("in_len", C.c_uint64), ("out_cap", C.c_uint64),
                ("dict_len", C.c_uint32), ("flags", C.c_uint32)]


def inflate_message(msg_id):
    return (rocm.lib().zng_rocm_inflate_message(int(msg_id)) or b"").decode()


class InflateDevBatch:
    """Many raw deflate streams that already sit in device memory, decoded on the device (zng_rocm_inflate_streams_dev).

    src: uint8 CUDA tensor; stream i = src[in_off[i] : in_off[i] + in_len[i]].
    dst: uint8 CUDA tensor; stream i's plaintext goes to dst[out_off[i] : out_off[i] + out_cap[i]], with dict_len[i]
         bytes of history directly in front of out_off[i] (inside dst).
    results: int32 CUDA tensor [n, 4] = {bytes produced, input bytes used, zlib status, message id}."""

    def __init__(self, src, in_off, in_len, dst, out_off, out_cap, dict_len=None):
        import torch
        rocm._need_init()
        self.src, self.dst = src, dst
        self.n = len(in_len)
        self.results = torch.zeros((self.n, 4), dtype=torch.int32, device=src.device)
        self.jobs = (InflateDevJob * self.n)()
        bi, bo = src.data_ptr(), dst.data_ptr()
        for i in range(self.n):
            d = 0 if dict_len is None else int(dict_len[i])
            if d > int(out_off[i]):
                raise ValueError("the history must lie inside dst, in front of the stream's output")
            if int(in_off[i]) + int(in_len[i]) > src.numel() or int(out_off[i]) + int(out_cap[i]) > dst.numel():
                raise ValueError("stream %d does not fit its tensor" % i)
            self.jobs[i].in_ptr = bi + int(in_off[i])
            self.jobs[i].out_ptr = bo + int(out_off[i])
            self.jobs[i].in_len = int(in_len[i])
            self.jobs[i].out_cap = int(out_cap[i])
            self.jobs[i].dict_len = d
            self.jobs[i].flags = 0

    def run(self, stream=None):
        """asynchronous on `stream`"""
        rocm._check(rocm.lib().zng_rocm_inflate_streams_dev(C.byref(self.jobs), self.n, rocm._dev_ptr(self.results),
                                                            rocm._stream_ptr(stream)), "zng_rocm_inflate_streams_dev")

    def run_wrapped(self, fmt, stream=None):
        """the same streams with their zlib (1) / gzip (2) wrapper: header parse, inflate, check values of the outputs and
        trailer comparison, all on the device (zng_rocm_uncompress_streams_dev)"""
        rocm._check(rocm.lib().zng_rocm_uncompress_streams_dev(fmt, C.byref(self.jobs), self.n, rocm._dev_ptr(self.results),
                                                               rocm._stream_ptr(stream)), "zng_rocm_uncompress_streams_dev")

    def run_dict(self, fmt, dictionary, stream=None):
        """the same streams decoded against a shared preset dictionary (deflate.Dictionary): fmt 0 raw -- every stream with
        the dictionary's window as history --, fmt 1 zlib with FDICT / DICTID judged per member
        (zng_rocm_uncompress_streams_dict_dev).  The jobs' own dict_len must be 0."""
        rocm._check(rocm.lib().zng_rocm_uncompress_streams_dict_dev(fmt, dictionary.h, C.byref(self.jobs), self.n,
                                                                    rocm._dev_ptr(self.results), rocm._stream_ptr(stream)),
                    "zng_rocm_uncompress_streams_dict_dev")

    def run_sizes(self, fmt, dictionary=None, stream=None):
        """the sizing pass over the same streams (zng_rocm_inflate_sizes_dev): fmt 0 raw, 1 zlib, 2 gzip; `results` gets the row
        the decode would write with all the room there is -- plaintext length, input consumed, status, message -- with no byte
        of output or history touched and no check value compared.  Of the history only its length counts: dict_len (fmt 0
        without a dictionary) or the deflate.Dictionary's window.  Asynchronous on `stream`."""
        rocm._check(rocm.lib().zng_rocm_inflate_sizes_dev(int(fmt), dictionary.h if dictionary is not None else None,
                                                          C.byref(self.jobs), self.n, rocm._dev_ptr(self.results),
                                                          rocm._stream_ptr(stream)), "zng_rocm_inflate_sizes_dev")

    def rows(self):
        """[(status, out_len, in_used, message)] (synchronises)"""
        r = self.results.cpu().tolist()
        return [(row[2], row[0], row[1], inflate_message(row[3])) for row in r]


def packed_jobs(src, in_off, in_len):
    """the job table of uncompress_packed_dev: member i = src[in_off[i] : in_off[i] + in_len[i]] of the uint8 CUDA tensor `src`"""
    n = len(in_len)
    jobs = (InflateDevJob * max(n, 1))()
    base = src.data_ptr() if src is not None and src.numel() else 0
    for i in range(n):
        if int(in_off[i]) + int(in_len[i]) > (src.numel() if src is not None else 0):
            raise ValueError("stream %d does not fit its tensor" % i)
        jobs[i].in_ptr = base + int(in_off[i]) if int(in_len[i]) else None
        jobs[i].in_len = int(in_len[i])
    return jobs


def uncompress_packed_dev(fmt, jobs, njobs, dst, offsets, results, align=1, dictionary=None, stream=None):
    """zng_rocm_uncompress_packed_dev: the members of `jobs` (packed_jobs) sized, placed and decoded back to back in the uint8
    CUDA tensor `dst` (dst.numel() is dst_cap; None: no destination), every start rounded up to `align`.  `offsets`: int64
    CUDA tensor of njobs + 1 (starts, then the room the batch needs -- above dst_cap when it did not all fit); `results`: int32
    CUDA tensor [njobs, 4] = {bytes, input used, status, message id}.  Asynchronous on `stream`; returns the status."""
    rocm._need_init()
    cap = int(dst.numel()) if dst is not None else 0
    return rocm.lib().zng_rocm_uncompress_packed_dev(int(fmt), dictionary.h if dictionary is not None else None, C.byref(jobs),
                                                     int(njobs), rocm._dev_ptr(dst) if cap else None, cap, int(align),
                                                     rocm._dev_ptr(offsets) if offsets is not None else None,
                                                     rocm._dev_ptr(results) if results is not None else None,
                                                     rocm._stream_ptr(stream))


SUBBLOCK = 1                                              # ZNG_ROCM_INFLATE_SUBBLOCK


def inflate_large_dev(src_dev, dst, window=None, stream=None, subblock=False):
    """zng_rocm_inflate_large_dev: ONE large raw stream that is already in device memory (`src_dev`: uint8 CUDA tensor),
    cut into parts and decoded on the device; plaintext into the CUDA tensor `dst`, optional history `window` (CUDA tensor,
    <= 32768 bytes).  Returns (zlib status, bytes produced, compressed bytes used, parts on the chain -- 0 when the
    sequential decoder did it).  subblock=True: zng_rocm_inflate_large_ex_dev with ZNG_ROCM_INFLATE_SUBBLOCK -- parts may
    also begin inside a block (inflate_large_last_subparts() says how many did)."""
    rocm._need_init()
    lib = rocm.lib()
    out_len, in_used = C.c_uint64(0), C.c_size_t(0)
    wl = 0 if window is None else int(window.numel())
    args = (rocm._dev_ptr(src_dev), int(src_dev.numel()), rocm._dev_ptr(window) if wl else None, wl, rocm._dev_ptr(dst),
            int(dst.numel()), C.byref(out_len), C.byref(in_used))
    if subblock:
        st = lib.zng_rocm_inflate_large_ex_dev(*args, SUBBLOCK, rocm._stream_ptr(stream))
    else:
        st = lib.zng_rocm_inflate_large_dev(*args, rocm._stream_ptr(stream))
    return st, int(out_len.value), int(in_used.value), int(lib.zng_rocm_inflate_large_last_parts())


def inflate_large_pieces_dev(src_dev, dst, piece_bytes=0, window=None, stream=None, subblock=False, flags=None):
    """zng_rocm_inflate_large_pieces_dev: inflate_large_dev for a stream of any length, decoded on the device in pieces of at
    most `piece_bytes` compressed bytes (0 = the library's default) with scratch that does not grow with the stream.
    Returns (zlib status, bytes produced, compressed bytes used, parts on the chains, device passes, compressed bytes the
    sequential decoder took).  `flags` overrides subblock (raw flag word)."""
    rocm._need_init()
    lib = rocm.lib()
    out_len, in_used = C.c_uint64(0), C.c_size_t(0)
    wl = 0 if window is None else int(window.numel())
    fl = (SUBBLOCK if subblock else 0) if flags is None else int(flags)
    st = lib.zng_rocm_inflate_large_pieces_dev(rocm._dev_ptr(src_dev), int(src_dev.numel()), rocm._dev_ptr(window) if wl else None,
                                               wl, rocm._dev_ptr(dst), int(dst.numel()), C.byref(out_len), C.byref(in_used),
                                               int(piece_bytes), fl, rocm._stream_ptr(stream))
    return (st, int(out_len.value), int(in_used.value), int(lib.zng_rocm_inflate_large_last_parts()),
            int(lib.zng_rocm_inflate_large_last_pieces()), int(lib.zng_rocm_inflate_large_last_host_bytes()))


def workspace_bytes(stream=None):
    """zng_rocm_workspace_bytes: device bytes the library's per-stream state of `stream` holds now"""
    return int(rocm.lib().zng_rocm_workspace_bytes(rocm._stream_ptr(stream)))


def inflate_large_last_subparts():
    """zng_rocm_inflate_large_last_subparts: of the parts on the calling thread's last chain, how many began inside a
    block (0 when none did or the sequential decoder did the work)."""
    return int(rocm.lib().zng_rocm_inflate_large_last_subparts())


def inflate_large_last_substarts():
    """zng_rocm_inflate_large_last_substarts: sub-starts the calling thread's last SUBBLOCK call placed"""
    return int(rocm.lib().zng_rocm_inflate_large_last_substarts())


class LargeJob(C.Structure):
    """zng_rocm_inflate_large_job"""
    _fields_ = [("d_src", C.c_void_p), ("src_len", C.c_size_t), ("d_window", C.c_void_p), ("window_len", C.c_uint32),
                ("d_dst", C.c_void_p), ("dst_cap", C.c_size_t), ("status", C.c_int), ("out_len", C.c_uint64),
                ("in_used", C.c_size_t), ("msg", C.c_char_p), ("parts", C.c_uint32), ("subparts", C.c_uint32)]


def large_jobs(srcs_dev, dsts, windows=None):
    """the job array of inflate_large_streams_dev for CUDA tensors (kept alive by the caller); output fields zeroed"""
    n = len(srcs_dev)
    jobs = (LargeJob * max(n, 1))()
    for i in range(n):
        w = None if windows is None else windows[i]
        wl = 0 if w is None else int(w.numel())
        jobs[i].d_src, jobs[i].src_len = rocm._dev_ptr(srcs_dev[i]), int(srcs_dev[i].numel())
        jobs[i].d_window, jobs[i].window_len = (rocm._dev_ptr(w) if wl else None), wl
        jobs[i].d_dst, jobs[i].dst_cap = rocm._dev_ptr(dsts[i]), int(dsts[i].numel())
    return jobs


def inflate_large_streams_dev(srcs_dev, dsts, windows=None, round_bytes=0, subblock=False, stream=None, flags=None, jobs=None):
    """zng_rocm_inflate_large_streams_dev: a batch of large raw streams that are already in device memory (`srcs_dev`: uint8
    CUDA tensors), decoded in rounds of one set of launches each; plaintext into the CUDA tensors `dsts`, optional per-job
    history `windows` (CUDA tensors of <= 32768 bytes, or None).  Returns (return value, rows, rounds, part launches) with
    rows = [(status, out_len, in_used, msg or None, parts, subparts)] per job.  `flags` overrides subblock (raw flag word);
    `jobs` (from large_jobs) is used as it is when given."""
    rocm._need_init()
    lib = rocm.lib()
    n = len(srcs_dev)
    if jobs is None:
        jobs = large_jobs(srcs_dev, dsts, windows)
    fl = (SUBBLOCK if subblock else 0) if flags is None else int(flags)
    rc = lib.zng_rocm_inflate_large_streams_dev(C.cast(jobs, C.c_void_p), n, int(round_bytes), fl, rocm._stream_ptr(stream))
    rows = [(int(j.status), int(j.out_len), int(j.in_used), j.msg.decode() if j.msg else None, int(j.parts), int(j.subparts))
            for j in jobs[:n]]
    return rc, rows, int(lib.zng_rocm_inflate_large_last_rounds()), int(lib.zng_rocm_inflate_large_last_part_launches())


class WrapperInfo(C.Structure):
    """zng_rocm_wrapper_info"""
    _fields_ = [("header_len", C.c_uint64), ("dictid", C.c_uint32), ("fdict", C.c_uint32)]


def wrapper_parse(fmt, data):
    """zng_rocm_wrapper_parse: the zlib (fmt 1) / gzip (fmt 2) wrapper of host bytes alone, by the rules the header kernel of
    the wrapped large calls runs; needs no device.  Returns (status, header_len, dictid, fdict, msg or None): status 0
    accepted, 2 accepted with a preset dictionary announced (dictid), -3 refused with the reference's text, -5 the bytes end
    inside the header."""
    keep, ptr, n = rocm._host_ptr(data)
    info, msg = WrapperInfo(), C.c_char_p()
    st = rocm.lib().zng_rocm_wrapper_parse(int(fmt), ptr, n, C.byref(info), C.byref(msg))
    return st, int(info.header_len), int(info.dictid), int(info.fdict), msg.value.decode() if msg.value else None


def uncompress_large_streams_dev(fmt, srcs_dev, dsts, dicts=None, round_bytes=0, subblock=False, stream=None, flags=None,
                                 jobs=None):
    """zng_rocm_uncompress_large_streams_dev: inflate_large_streams_dev for zlib (fmt 1) / gzip (fmt 2) members (fmt 0: the
    raw call).  `srcs_dev`: the whole members, wrapper included; `dicts`: per job the preset dictionary of a zlib member or
    None.  Returns (return value, rows, rounds, part launches), rows = [(status, out_len, in_used, msg or None, parts,
    subparts)] as the raw call; status 2 = the member needs a dictionary."""
    rocm._need_init()
    lib = rocm.lib()
    n = len(srcs_dev)
    if jobs is None:
        jobs = large_jobs(srcs_dev, dsts, dicts)
    fl = (SUBBLOCK if subblock else 0) if flags is None else int(flags)
    rc = lib.zng_rocm_uncompress_large_streams_dev(int(fmt), C.cast(jobs, C.c_void_p), n, int(round_bytes), fl,
                                                   rocm._stream_ptr(stream))
    rows = [(int(j.status), int(j.out_len), int(j.in_used), j.msg.decode() if j.msg else None, int(j.parts), int(j.subparts))
            for j in jobs[:n]]
    return rc, rows, int(lib.zng_rocm_inflate_large_last_rounds()), int(lib.zng_rocm_inflate_large_last_part_launches())


def uncompress_large_dev(fmt, src_dev, dst, dict=None, piece_bytes=0, stream=None, subblock=False, flags=None):
    """zng_rocm_uncompress_large_dev: inflate_large_pieces_dev for ONE zlib (fmt 1) / gzip (fmt 2) member of any length
    (fmt 0: the raw call).  Returns (status, bytes produced, member bytes used, parts on the chains, device passes,
    compressed bytes the sequential decoder took) as the raw call."""
    rocm._need_init()
    lib = rocm.lib()
    out_len, in_used = C.c_uint64(0), C.c_size_t(0)
    dl = 0 if dict is None else int(dict.numel())
    fl = (SUBBLOCK if subblock else 0) if flags is None else int(flags)
    st = lib.zng_rocm_uncompress_large_dev(int(fmt), rocm._dev_ptr(src_dev), int(src_dev.numel()), rocm._dev_ptr(dict) if dl else None,
                                           dl, rocm._dev_ptr(dst), int(dst.numel()), C.byref(out_len), C.byref(in_used),
                                           int(piece_bytes), fl, rocm._stream_ptr(stream))
    return (st, int(out_len.value), int(in_used.value), int(lib.zng_rocm_inflate_large_last_parts()),
            int(lib.zng_rocm_inflate_large_last_pieces()), int(lib.zng_rocm_inflate_large_last_host_bytes()))


def uncompress_large_size_dev(fmt, src_dev, dict=None, dict_len=None, stream=None, flags=0):
    """zng_rocm_uncompress_large_size_dev: the plaintext length of ONE large stream that is already in device memory, found by
    a counting pass that decodes nothing (fmt 0 raw, 1 zlib, 2 gzip; the member with its wrapper).  `dict`: the preset
    dictionary of a zlib member (CUDA tensor); fmt 0: the history the caller will put in front -- only its length matters, so
    `dict_len` alone will do.  Returns (status, plaintext bytes, member bytes used, parts on the chain -- 0 when the
    one-wavefront kernel sized the stream)."""
    rocm._need_init()
    lib = rocm.lib()
    out_len, in_used = C.c_uint64(0), C.c_size_t(0)
    dl = (0 if dict is None else int(dict.numel())) if dict_len is None else int(dict_len)
    n = 0 if src_dev is None else int(src_dev.numel())
    st = lib.zng_rocm_uncompress_large_size_dev(int(fmt), rocm._dev_ptr(src_dev) if n else None, n,
                                                rocm._dev_ptr(dict) if dict is not None and dict.numel() else None, dl,
                                                C.byref(out_len), C.byref(in_used), int(flags), rocm._stream_ptr(stream))
    return st, int(out_len.value), int(in_used.value), int(lib.zng_rocm_inflate_large_last_parts())


def uncompress_large_sizes_dev(fmt, srcs_dev, dicts=None, round_bytes=0, stream=None, flags=0, jobs=None):
    """zng_rocm_uncompress_large_sizes_dev: uncompress_large_size_dev for a batch, in rounds of one finder pass and ONE
    counting part launch each.  Returns (return value, rows, rounds, part launches), rows = [(status, out_len, in_used,
    msg or None, parts, subparts = 0)].  `jobs` (from large_jobs; d_dst / dst_cap are not looked at) is used as it is when
    given."""
    rocm._need_init()
    lib = rocm.lib()
    n = len(srcs_dev)
    if jobs is None:
        jobs = (LargeJob * max(n, 1))()
        for i in range(n):
            d = None if dicts is None else dicts[i]
            dl = 0 if d is None else int(d.numel())
            jobs[i].d_src, jobs[i].src_len = (rocm._dev_ptr(srcs_dev[i]) if srcs_dev[i].numel() else None), int(srcs_dev[i].numel())
            jobs[i].d_window, jobs[i].window_len = (rocm._dev_ptr(d) if dl else None), dl
    rc = lib.zng_rocm_uncompress_large_sizes_dev(int(fmt), C.cast(jobs, C.c_void_p), n, int(round_bytes), int(flags),
                                                 rocm._stream_ptr(stream))
    rows = [(int(j.status), int(j.out_len), int(j.in_used), j.msg.decode() if j.msg else None, int(j.parts), int(j.subparts))
            for j in jobs[:n]]
    return rc, rows, int(lib.zng_rocm_inflate_large_last_rounds()), int(lib.zng_rocm_inflate_large_last_part_launches())


class GzipMember(C.Structure):
    """zng_rocm_gzip_member"""
    _fields_ = [("src_off", C.c_uint64), ("src_len", C.c_uint64), ("dst_off", C.c_uint64), ("out_len", C.c_uint64),
                ("crc", C.c_uint32), ("bgzf", C.c_uint32)]


def gunzip_members_dev(src_dev, dst, members_cap=None, stream=None, subblock=False, flags=None):
    """zng_rocm_gunzip_members_dev: EVERY member of a gzip file that is already in device memory (`src_dev`: uint8 CUDA tensor;
    concatenated members, BGZF), plaintexts one behind the other in the CUDA tensor `dst`.  `members_cap`: rows of the member
    table to take (None = all: room for src_len / 18 + 1 rows, the most a file can hold, is reserved as address space -- a numpy
    array that is not initialised, so only the rows the call writes cost memory).  Returns
    (status, bytes produced, file bytes used, members, nmembers, counters) with members = [(src_off, src_len, dst_off,
    out_len, crc, bgzf)] and counters = {"candidates", "replans", "small", "large"} (zng_rocm_gunzip_last_*)."""
    import numpy as np
    rocm._need_init()
    lib = rocm.lib()
    n = int(src_dev.numel())
    cap = n // 18 + 1 if members_cap is None else int(members_cap)
    table = np.empty(max(cap, 1) * C.sizeof(GzipMember), dtype=np.uint8)
    out_len, in_used, nmembers = C.c_uint64(0), C.c_size_t(0), C.c_size_t(0)
    fl = (SUBBLOCK if subblock else 0) if flags is None else int(flags)
    st = lib.zng_rocm_gunzip_members_dev(rocm._dev_ptr(src_dev) if n else None, n, rocm._dev_ptr(dst) if dst.numel() else None,
                                         int(dst.numel()), C.byref(out_len), C.byref(in_used),
                                         C.c_void_p(table.ctypes.data) if cap else None, cap, C.byref(nmembers), fl,
                                         rocm._stream_ptr(stream))
    rows = [(int(m.src_off), int(m.src_len), int(m.dst_off), int(m.out_len), int(m.crc), int(m.bgzf))
            for m in (GzipMember * min(cap, int(nmembers.value))).from_buffer(table)]
    counters = {"candidates": int(lib.zng_rocm_gunzip_last_candidates()), "replans": int(lib.zng_rocm_gunzip_last_replans()),
                "small": int(lib.zng_rocm_gunzip_last_small()), "large": int(lib.zng_rocm_gunzip_last_large())}
    return st, int(out_len.value), int(in_used.value), rows, int(nmembers.value), counters


class BgzfRange(C.Structure):
    """zng_rocm_bgzf_range"""
    _fields_ = [("uoff", C.c_uint64), ("len", C.c_uint64), ("d_dst", C.c_void_p), ("status", C.c_int), ("out_len", C.c_uint64),
                ("msg", C.c_char_p)]


def member_table(rows):
    """[(src_off, src_len, dst_off, out_len, crc, bgzf)] -> a ctypes array of zng_rocm_gzip_member (host memory)"""
    table = (GzipMember * max(len(rows), 1))()
    for k, row in enumerate(rows):
        table[k] = GzipMember(*(int(v) for v in row))
    return table


class GzipHeaderRow(C.Structure):
    """zng_rocm_gzip_header_row"""
    _fields_ = [("status", C.c_int32), ("flg", C.c_uint32), ("msg", C.c_char_p), ("header_len", C.c_uint64), ("time", C.c_uint32),
                ("xflags", C.c_uint32), ("os", C.c_uint32), ("text", C.c_uint32), ("hcrc", C.c_uint32), ("extra_len", C.c_uint32),
                ("name_len", C.c_uint64), ("comment_len", C.c_uint64), ("extra_off", C.c_uint64), ("name_off", C.c_uint64),
                ("comment_off", C.c_uint64), ("text_off", C.c_uint64)]

    def as_dict(self):
        d = {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "msg"}
        d["msg"] = self.msg.decode() if self.msg else None
        return d


def gzip_header_parse(data):
    """zng_rocm_gzip_header_parse: the header fields of ONE gzip member in host bytes (inflateGetHeader), by the rules
    wrapper_parse(2, ...) judges with; needs no device.  Returns (status, row) with row the zng_rocm_gzip_header_row as a dict:
    the offsets count from the member's first byte, 0 = the field is absent."""
    keep, ptr, n = rocm._host_ptr(data)
    row = GzipHeaderRow()
    st = rocm.lib().zng_rocm_gzip_header_parse(ptr, n, C.byref(row))
    return st, row.as_dict()


def gzip_headers_dev(src_dev, members, text_cap=None, stream=None):
    """zng_rocm_gzip_headers_dev: the header fields of the members of the gzip file in `src_dev` (uint8 CUDA tensor); `members`
    the rows of gunzip_members_dev / bgzf_index_dev / bgzf_compress_dev, rows built from the offsets compress_members_header_dev
    left, or a member_table() of them.  `text_cap`: bytes of the text buffer (None: the call is made twice, the first time to
    learn the size).  Returns (status, rows, text, text_need): rows = one dict per member (GzipHeaderRow.as_dict), text = the
    bytes object of text_cap bytes the fields were gathered into -- extra, name and a 0, comment and a 0 of every accepted member
    at its row's text_off -- untouched (zeros) when the status is -5."""
    rocm._need_init()
    lib = rocm.lib()
    n = len(members)
    table = members if isinstance(members, C.Array) else member_table(members)
    rows = (GzipHeaderRow * max(n, 1))()
    need = C.c_size_t(0)
    src_len = int(src_dev.numel())

    def call(cap):
        text = (C.c_uint8 * max(cap, 1))()
        st = lib.zng_rocm_gzip_headers_dev(rocm._dev_ptr(src_dev) if src_len else None, src_len, C.cast(table, C.c_void_p), n,
                                           C.cast(rows, C.c_void_p), C.cast(text, C.c_void_p) if cap else None, cap, C.byref(need),
                                           rocm._stream_ptr(stream))
        return st, bytes(text)[:cap]
    st, text = call(0 if text_cap is None else int(text_cap))
    if text_cap is None and st == -5:
        st, text = call(int(need.value))
    return st, [rows[k].as_dict() for k in range(n)], text, int(need.value)


def bgzf_index_dev(src_dev, members_cap=None, stream=None):
    """zng_rocm_bgzf_index_dev: the members table of a BGZF file in device memory (`src_dev`: uint8 CUDA tensor) without
    decoding it.  `members_cap`: rows to take (None = all, reserved as in gunzip_members_dev).  Returns (status, members,
    nmembers, plaintext bytes, file bytes used) with members = [(src_off, src_len, dst_off, out_len, crc, bgzf)]."""
    import numpy as np
    rocm._need_init()
    lib = rocm.lib()
    n = int(src_dev.numel())
    cap = n // 28 + 1 if members_cap is None else int(members_cap)
    table = np.empty(max(cap, 1) * C.sizeof(GzipMember), dtype=np.uint8)
    nmembers, plain_len, in_used = C.c_size_t(0), C.c_uint64(0), C.c_size_t(0)
    st = lib.zng_rocm_bgzf_index_dev(rocm._dev_ptr(src_dev) if n else None, n, C.c_void_p(table.ctypes.data) if cap else None, cap,
                                     C.byref(nmembers), C.byref(plain_len), C.byref(in_used), rocm._stream_ptr(stream))
    rows = [(int(m.src_off), int(m.src_len), int(m.dst_off), int(m.out_len), int(m.crc), int(m.bgzf))
            for m in (GzipMember * min(cap, int(nmembers.value))).from_buffer(table)]
    return st, rows, int(nmembers.value), int(plain_len.value), int(in_used.value)


def bgzf_read_dev(src_dev, members, ranges, scratch_bytes=0, stream=None):
    """zng_rocm_bgzf_read_dev: `ranges` = [(uoff, len, dst)] with dst a uint8 CUDA tensor of at least len bytes, a device
    address or None, `members` the rows of bgzf_index_dev / gunzip_members_dev / bgzf_compress_dev for the file in `src_dev`, or a
    member_table() of them.  Returns (return value, [(status, out_len, msg)] per range, counters) with counters = {"decoded",
    "direct", "rounds"} (zng_rocm_bgzf_read_last_*)."""
    rocm._need_init()
    lib = rocm.lib()
    n = int(src_dev.numel())
    table, nm = (member_table(members), len(members)) if isinstance(members, (list, tuple)) else (members, len(members))
    rs = (BgzfRange * max(len(ranges), 1))()
    for k, (uoff, length, dst) in enumerate(ranges):
        rs[k] = BgzfRange(int(uoff), int(length), None if dst is None else int(dst) if isinstance(dst, int) else dst.data_ptr(), 0, 0, None)
    st = lib.zng_rocm_bgzf_read_dev(rocm._dev_ptr(src_dev) if n else None, n, C.cast(table, C.c_void_p), nm, C.cast(rs, C.c_void_p),
                                    len(ranges), int(scratch_bytes), rocm._stream_ptr(stream))
    out = [(int(r.status), int(r.out_len), None if r.msg is None else r.msg.decode()) for r in rs[:len(ranges)]]
    counters = {"decoded": int(lib.zng_rocm_bgzf_read_last_decoded()), "direct": int(lib.zng_rocm_bgzf_read_last_direct()),
                "rounds": int(lib.zng_rocm_bgzf_read_last_rounds())}
    return st, out, counters



class AccessPoint(C.Structure):
    """zng_rocm_access_point"""
    _fields_ = [("in_bit", C.c_uint64), ("out_off", C.c_uint64), ("window_len", C.c_uint32), ("reserved", C.c_uint32)]


class InflateRange(BgzfRange):
    """zng_rocm_inflate_range: the fields of zng_rocm_bgzf_range"""


class InflateIndex:
    """A zng_rocm_inflate_index: access points into ONE raw deflate (fmt 0), zlib (1) or gzip (2) stream in device memory.
    Made by InflateIndex.build() or InflateIndex.load(); immutable; close() (or the garbage collector) frees it."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def build(cls, fmt, src_dev, dst, span_bytes=0, piece_bytes=0, stream=None, subblock=False, flags=None):
        """zng_rocm_inflate_index_build_dev.  Returns (status, bytes produced, member bytes used, index or None): the first
        three are uncompress_large_dev's for the same arguments (the last_* counters too); an index exists on status 1."""
        rocm._need_init()
        lib = rocm.lib()
        out_len, in_used, h = C.c_uint64(0), C.c_size_t(0), C.c_void_p(None)
        fl = (SUBBLOCK if subblock else 0) if flags is None else int(flags)
        n, cap = int(src_dev.numel()), int(dst.numel())
        st = lib.zng_rocm_inflate_index_build_dev(int(fmt), rocm._dev_ptr(src_dev) if n else None, n, rocm._dev_ptr(dst) if cap else None,
                                                  cap, C.byref(out_len), C.byref(in_used), int(span_bytes), int(piece_bytes), fl,
                                                  C.byref(h), rocm._stream_ptr(stream))
        return st, int(out_len.value), int(in_used.value), cls(h.value) if h.value else None

    @classmethod
    def load(cls, blob, stream=None):
        """zng_rocm_inflate_index_import_dev: (return value, index or None) from the bytes save() gave"""
        rocm._need_init()
        raw = bytes(blob)
        h = C.c_void_p(None)
        st = rocm.lib().zng_rocm_inflate_index_import_dev(raw, len(raw), C.byref(h), rocm._stream_ptr(stream))
        return st, cls(h.value) if h.value else None

    def save(self, stream=None):
        """zng_rocm_inflate_index_export: the index as bytes"""
        lib = rocm.lib()
        need = C.c_size_t(0)
        lib.zng_rocm_inflate_index_export(self._h, None, 0, C.byref(need), rocm._stream_ptr(stream))
        buf = (C.c_uint8 * max(need.value, 1))()
        rocm._check(lib.zng_rocm_inflate_index_export(self._h, buf, need.value, C.byref(need), rocm._stream_ptr(stream)),
                    "zng_rocm_inflate_index_export")
        return bytes(buf[:need.value])

    def points(self):
        """[(in_bit, out_off, window_len)]"""
        lib = rocm.lib()
        n = int(lib.zng_rocm_inflate_index_points(self._h, None, 0))
        pts = (AccessPoint * max(n, 1))()
        lib.zng_rocm_inflate_index_points(self._h, C.cast(pts, C.c_void_p), n)
        return [(int(p.in_bit), int(p.out_off), int(p.window_len)) for p in pts[:n]]

    @property
    def plain_len(self):
        return int(rocm.lib().zng_rocm_inflate_index_plain_len(self._h))

    def read(self, src_dev, ranges, scratch_bytes=0, stream=None, src_len=None):
        """zng_rocm_inflate_index_read_dev: `ranges` = [(uoff, len, dst)] with dst a uint8 CUDA tensor of at least len bytes, a
        device address or None; `src_len`: the file's length when it is not all of `src_dev`.  Returns (return value,
        [(status, out_len, msg)] per range, counters) with counters = {"decoded", "direct", "rounds"}."""
        rocm._need_init()
        lib = rocm.lib()
        n = int(src_dev.numel()) if src_len is None else int(src_len)
        rs = (InflateRange * max(len(ranges), 1))()
        for k, (uoff, length, dst) in enumerate(ranges):
            rs[k] = InflateRange(int(uoff), int(length), None if dst is None else int(dst) if isinstance(dst, int) else dst.data_ptr(),
                                 0, 0, None)
        st = lib.zng_rocm_inflate_index_read_dev(self._h, rocm._dev_ptr(src_dev) if n else None, n, C.cast(rs, C.c_void_p), len(ranges),
                                                 int(scratch_bytes), rocm._stream_ptr(stream))
        out = [(int(r.status), int(r.out_len), None if r.msg is None else r.msg.decode()) for r in rs[:len(ranges)]]
        counters = {"decoded": int(lib.zng_rocm_inflate_index_read_last_decoded()),
                    "direct": int(lib.zng_rocm_inflate_index_read_last_direct()),
                    "rounds": int(lib.zng_rocm_inflate_index_read_last_rounds())}
        return st, out, counters

    def close(self):
        if self._h:
            rocm.lib().zng_rocm_inflate_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bgzf_voffset(members, uoff):
    """zng_rocm_bgzf_voffset: the virtual offset of plaintext byte `uoff` (htslib's convention), or None when the call refuses;
    needs no device"""
    table = member_table(members) if isinstance(members, (list, tuple)) else members
    voff = C.c_uint64(0)
    st = rocm.lib().zng_rocm_bgzf_voffset(C.cast(table, C.c_void_p), len(members), int(uoff), C.byref(voff))
    return int(voff.value) if st == 0 else None


def bgzf_uoffset(members, voff):
    """zng_rocm_bgzf_uoffset: the plaintext offset a virtual offset stands for, or None when the call refuses; needs no device"""
    table = member_table(members) if isinstance(members, (list, tuple)) else members
    uoff = C.c_uint64(0)
    st = rocm.lib().zng_rocm_bgzf_uoffset(C.cast(table, C.c_void_p), len(members), int(voff), C.byref(uoff))
    return int(uoff.value) if st == 0 else None
