"""zng_rocm_hook_clone (zlib-ng_amd/csrc/hook.hip) through ctypes: the clone has the source's history, copied on the device;
afterwards the two share nothing -- a block through either leaves the other's history alone, and either may be destroyed
first."""
import ctypes as C
import importlib
import zlib

import pytest

import synth

pytestmark = pytest.mark.gpu

EINVAL = -3


@pytest.fixture(scope="module")
def lib():
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return zr.lib()


def create(lib):
    h = C.c_void_p()
    assert lib.zng_rocm_hook_create(C.byref(h), 1 << 20) == 0
    return h


def clone(lib, h):
    out = C.c_void_p()
    assert lib.zng_rocm_hook_clone(h, C.byref(out)) == 0
    assert out.value and out.value != h.value
    return out


def history(lib, h):
    n = C.c_uint32(0)
    buf = C.create_string_buffer(32768)
    assert lib.zng_rocm_hook_get_history(h, C.addressof(buf), C.byref(n)) == 0
    return buf.raw[:n.value]


def deflate_block(lib, h, data, level=6, final=False):
    """one raw block (or the last) of the hook's stream -> its bytes"""
    cap = lib.zng_rocm_hook_deflate_bound(len(data))
    out = C.create_string_buffer(cap)
    out_len = C.c_size_t(0)
    src = C.create_string_buffer(data, max(len(data), 1))
    rc = lib.zng_rocm_hook_deflate_block(h, level, C.addressof(src), len(data), 0 if final else 1, 0, None,
                                         C.addressof(out), cap, C.byref(out_len))
    assert rc == 0
    return out.raw[:out_len.value]


def test_clone_of_a_fresh_hook_has_no_history(lib):
    h = create(lib)
    c = clone(lib, h)
    assert history(lib, c) == b"" and history(lib, h) == b""
    lib.zng_rocm_hook_destroy(c)
    lib.zng_rocm_hook_destroy(h)


@pytest.mark.parametrize("hist_len", [1, 5000, 32767, 32768])
def test_clone_has_the_sources_history(lib, hist_len):
    """every length from one byte to the full window: the history sits at the END of its 32 KiB, so a copy from the wrong
    end or of the wrong length shows"""
    data = synth.silesia_like(40000, seed=51).tobytes()[:hist_len]
    h = create(lib)
    assert lib.zng_rocm_hook_set_history(h, data, len(data)) == 0
    c = clone(lib, h)
    assert history(lib, c) == data and history(lib, h) == data
    lib.zng_rocm_hook_destroy(h)
    lib.zng_rocm_hook_destroy(c)


def test_streams_are_independent_after_the_clone(lib):
    first = synth.silesia_like(300000, seed=52).tobytes()
    a = synth.silesia_like(100000, seed=53).tobytes()
    b = synth.silesia_like(70001, seed=54).tobytes()
    h = create(lib)
    head = deflate_block(lib, h, first)
    assert history(lib, h) == first[-32768:]
    c = clone(lib, h)
    assert history(lib, c) == first[-32768:]
    # a block through the source: the clone's history stays, and the other way round
    tail_a = deflate_block(lib, h, a, final=True)
    assert history(lib, h) == a[-32768:] and history(lib, c) == first[-32768:]
    tail_b = deflate_block(lib, c, b, final=True)
    assert history(lib, c) == b[-32768:] and history(lib, h) == a[-32768:]
    assert zlib.decompressobj(-15).decompress(head + tail_a) == first + a
    assert zlib.decompressobj(-15).decompress(head + tail_b) == first + b
    lib.zng_rocm_hook_destroy(c)
    lib.zng_rocm_hook_destroy(h)


def test_the_clone_outlives_the_source(lib):
    """the tail repeats the end of the first block: with the history it costs a few hundred bytes, without it thousands"""
    first = synth.silesia_like(200000, seed=55).tobytes()
    tail = first[-20000:]
    h = create(lib)
    head = deflate_block(lib, h, first)
    c = clone(lib, h)
    lib.zng_rocm_hook_destroy(h)
    assert history(lib, c) == first[-32768:]
    block = deflate_block(lib, c, tail, final=True)
    assert zlib.decompressobj(-15).decompress(head + block) == first + tail
    assert len(block) < 2000, len(block)
    c2 = clone(lib, c)                                  # a clone of a clone, the middle one leaves first
    lib.zng_rocm_hook_destroy(c)
    assert history(lib, c2) == (first + tail)[-32768:]
    lib.zng_rocm_hook_destroy(c2)


def test_clone_through_the_python_class(lib):
    inf = importlib.import_module("zlib-ng_amd.inflate")
    plain = synth.silesia_like(500000, seed=56).tobytes()
    comp = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = comp.compress(plain) + comp.flush(zlib.Z_SYNC_FLUSH)
    more = synth.silesia_like(90000, seed=57).tobytes()
    rest = comp.compress(plain[-30000:] + more) + comp.flush()
    hook = inf.InflateHook()
    try:
        st, out, end_bit, cv, msg = hook.inflate_blocks(raw, check=1, check_value=1)
        assert (st, out, end_bit) == (0, plain, 8 * len(raw)), (st, msg)
        other = hook.clone()
        try:
            assert other.get_history() == plain[-32768:] == hook.get_history()
            for h in (other, hook):                     # both continue the same stream, each from its own history
                st, out, end_bit, cv2, msg = h.inflate_blocks(rest, check=1, check_value=cv)
                assert (st, out) == (1, plain[-30000:] + more), (st, msg)
                assert cv2 == zlib.adler32(plain + plain[-30000:] + more)
        finally:
            other.close()
    finally:
        hook.close()


def test_null_arguments(lib):
    h = create(lib)
    out = C.c_void_p(0xdead)
    assert lib.zng_rocm_hook_clone(None, C.byref(out)) == EINVAL
    assert out.value is None
    assert lib.zng_rocm_hook_clone(h, None) == EINVAL
    assert history(lib, h) == b""
    lib.zng_rocm_hook_destroy(h)
