"""CPU checks of the sizing calls for large device-resident streams (zng_rocm_uncompress_large_size_dev,
zng_rocm_uncompress_large_sizes_dev): the built library exports them with the signatures include/zng_rocm.h declares, the
header is strict C11 with them, and before zng_rocm_init every refusal the header lists answers ZNG_ROCM_EINVAL, an accepted
call ZNG_ROCM_ENODEV, and neither writes a job field or an out-parameter."""
import importlib
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = (
    "int zng_rocm_uncompress_large_size_dev(int format, const uint8_t *d_src, size_t src_len, const uint8_t *d_dict, "
    "uint32_t dict_len, uint64_t *out_len, size_t *in_used, uint32_t flags, void *stream);",
    "int zng_rocm_uncompress_large_sizes_dev(int format, zng_rocm_inflate_large_job *jobs, size_t njobs, size_t round_bytes, "
    "uint32_t flags, void *stream);",
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
    # the ctypes signatures of the package follow the declarations: nine and six arguments
    assert len(lib.zng_rocm_uncompress_large_size_dev.argtypes) == 9
    assert len(lib.zng_rocm_uncompress_large_sizes_dev.argtypes) == 6


def test_c11_consumer_before_init():
    zr = importlib.import_module("zlib-ng_amd")
    libdir = os.path.dirname(zr.lib_path())
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "abi_inflate_large_size")
        subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2",
                               "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "abi_inflate_large_size.c"),
                               "-o", exe, "-L" + libdir, "-lzng_rocm", "-Wl,-rpath," + libdir])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr)
    assert out.stdout.strip() == "ok nodev"


def test_python_wrappers_exist():
    inf = importlib.import_module("zlib-ng_amd.inflate")
    assert callable(inf.uncompress_large_size_dev) and callable(inf.uncompress_large_sizes_dev)
