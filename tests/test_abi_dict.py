"""CPU checks of the shared-dictionary entry points (zng_rocm_dict_create_dev, zng_rocm_dict_destroy, zng_rocm_dict_id,
zng_rocm_dict_window, zng_rocm_compress_streams_dict_bound, zng_rocm_compress_streams_dict_dev,
zng_rocm_uncompress_streams_dict_dev): the built library exports them with the signatures include/zng_rocm.h declares, the
header is strict C11 with them, and before zng_rocm_init the create call returns ZNG_ROCM_ENODEV, destroy(NULL) is harmless
and the bound is 0 for a format the call refuses."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = (
    "typedef struct zng_rocm_dict zng_rocm_dict;",
    "int zng_rocm_dict_create_dev(const uint8_t *d_dict, size_t dict_len, zng_rocm_dict **out, void *stream);",
    "void zng_rocm_dict_destroy(zng_rocm_dict *d);",
    "uint32_t zng_rocm_dict_id(const zng_rocm_dict *d);",
    "uint32_t zng_rocm_dict_window(const zng_rocm_dict *d);",
    "size_t zng_rocm_compress_streams_dict_bound(size_t source_len, int format);",
    "int zng_rocm_compress_streams_dict_dev(int format, const zng_rocm_dict *dict, const zng_rocm_stream_job *jobs, "
    "size_t njobs, uint32_t *d_results, void *stream);",
    "int zng_rocm_uncompress_streams_dict_dev(int format, const zng_rocm_dict *dict, const zng_rocm_inflate_dev_job *jobs, "
    "size_t njobs, uint32_t *d_results, void *stream);",
)


def test_symbols_exported_with_the_declared_signatures():
    zr = importlib.import_module("zlib-ng_amd")
    lib = zr.lib()
    hdr = open(os.path.join(ROOT, "include", "zng_rocm.h")).read()
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))
    for decl in DECLS:
        assert decl in hdr, decl
    for name in re.findall(r"\b(zng_rocm_[a-z0-9_]+)\(", " ".join(DECLS)):
        assert hasattr(lib, name) and name in zr.rocm.exported_names(), name


def test_c11_consumer_before_init():
    zr = importlib.import_module("zlib-ng_amd")
    libdir = os.path.dirname(zr.lib_path())
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "abi_dict")
        subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2",
                               "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "abi_dict.c"),
                               "-o", exe, "-L" + libdir, "-lzng_rocm", "-Wl,-rpath," + libdir])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr)
    assert out.stdout.strip() == "ok nodev"


def test_bound_and_null_handles_through_ctypes():
    zr = importlib.import_module("zlib-ng_amd")
    lib = zr.lib()
    for n in (0, 1, 1000, 100000):
        assert lib.zng_rocm_compress_streams_dict_bound(n, 2) == 0 and lib.zng_rocm_compress_streams_dict_bound(n, -1) == 0
        assert lib.zng_rocm_compress_streams_dict_bound(n, 0) == lib.zng_rocm_deflate_quick_bound(n)
        assert lib.zng_rocm_compress_streams_dict_bound(n, 1) == lib.zng_rocm_deflate_quick_bound(n) + 16 + 4 + 4
    lib.zng_rocm_dict_destroy(None)
    assert lib.zng_rocm_dict_id(None) == 0 and lib.zng_rocm_dict_window(None) == 0
    if zr.device_count() > 0:
        return                                    # (a process without zng_rocm_init: the C consumer above)
    h = C.c_void_p(1234)
    buf = (C.c_uint8 * 64)()
    assert lib.zng_rocm_dict_create_dev(buf, 64, C.byref(h), None) == -1 and not h.value
