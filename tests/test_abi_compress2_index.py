"""CPU checks of zng_rocm_compress2_index_dev: the built library exports it with the signature include/zng_rocm.h declares, the
header is strict C11 with it, and before zng_rocm_init a refused span_bytes or a null result pointer answers ZNG_ROCM_EINVAL
ahead of everything else, a call that passes it answers ZNG_ROCM_ENODEV as zng_rocm_compress2_dev does, and neither leaves an
index or touches *dst_len."""
import importlib
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = ("int zng_rocm_compress2_index_dev(uint8_t *d_dst, size_t *dst_len, const uint8_t *d_src, size_t src_len, int level, int format, "
        "uint64_t span_bytes, zng_rocm_inflate_index **out, void *stream);")


def test_symbol_exported_with_the_declared_signature():
    zr = importlib.import_module("zlib-ng_amd")
    lib = zr.lib()
    hdr = open(os.path.join(ROOT, "include", "zng_rocm.h")).read()
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))
    assert DECL in hdr
    assert hasattr(lib, "zng_rocm_compress2_index_dev") and "zng_rocm_compress2_index_dev" in zr.rocm.exported_names()
    # compress2_dev's seven arguments with span_bytes and the result pointer in front of the stream
    assert len(lib.zng_rocm_compress2_index_dev.argtypes) == 9
    assert lib.zng_rocm_compress2_index_dev.argtypes[:6] == lib.zng_rocm_compress2_dev.argtypes[:6]


def test_c11_consumer_before_init():
    zr = importlib.import_module("zlib-ng_amd")
    libdir = os.path.dirname(zr.lib_path())
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "abi_compress2_index")
        subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2",
                               "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "abi_compress2_index.c"),
                               "-o", exe, "-L" + libdir, "-lzng_rocm", "-Wl,-rpath," + libdir])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr)
    assert out.stdout.strip() == "ok nodev"


def test_python_wrapper_exists():
    one = importlib.import_module("zlib-ng_amd.oneshot")
    assert callable(one.compress2_index_dev)
