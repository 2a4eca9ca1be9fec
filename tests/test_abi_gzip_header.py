"""CPU checks of the gzip header entry points (zng_rocm_gzip_header_bytes, zng_rocm_gzip_header_write,
zng_rocm_compress_streams2_header_dev, zng_rocm_compress_members_header_dev, zng_rocm_gzip_header_parse,
zng_rocm_gzip_headers_dev): the built library exports them with the signatures include/zng_rocm.h declares, the header is strict
C11 with them and both structures have the layout it states, before zng_rocm_init the three device calls return
ZNG_ROCM_ENODEV and write nothing -- refusals first --, and the two host calls work without a GPU."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = (
    "size_t zng_rocm_gzip_header_bytes(const zng_rocm_gzip_header *h);",
    "size_t zng_rocm_gzip_header_write(const zng_rocm_gzip_header *h, int level, int strategy, uint8_t *buf, size_t cap);",
    "int zng_rocm_compress_streams2_header_dev(int level, int strategy, int window_bits, const zng_rocm_stream_job *jobs, "
    "const zng_rocm_gzip_header *heads, size_t njobs, size_t round_bytes, uint32_t *d_results, void *stream);",
    "int zng_rocm_compress_members_header_dev(int level, int strategy, int window_bits, const zng_rocm_stream_job *jobs, "
    "const zng_rocm_gzip_header *heads, size_t njobs, uint8_t *d_dst, size_t dst_cap, size_t round_bytes, uint64_t *d_offsets, "
    "uint32_t *d_checks, void *stream);",
    "int zng_rocm_gzip_header_parse(const uint8_t *src, size_t src_len, zng_rocm_gzip_header_row *row);",
    "int zng_rocm_gzip_headers_dev(const uint8_t *d_src, size_t src_len, const zng_rocm_gzip_member *members, size_t nmembers, "
    "zng_rocm_gzip_header_row *rows, uint8_t *text, size_t text_cap, size_t *text_need, void *stream);",
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
    for cite in ("zlib-ng.h.in:127-141", "deflate.c:922-1023", "inflate.c:556-700"):
        assert cite in open(os.path.join(ROOT, "include", "zng_rocm.h")).read(), cite


def test_c11_consumer_before_init():
    zr = importlib.import_module("zlib-ng_amd")
    libdir = os.path.dirname(zr.lib_path())
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "abi_gzip_header")
        subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2",
                               "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "abi_gzip_header.c"),
                               "-o", exe, "-L" + libdir, "-lzng_rocm", "-Wl,-rpath," + libdir])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr)
    assert out.stdout.strip() == "ok nodev"


def test_python_structures_mirror_the_header():
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    inf = importlib.import_module("zlib-ng_amd.inflate")
    assert C.sizeof(dfl.GzipHeader) == 48 and dfl.GzipHeader.extra.offset == 16 and dfl.GzipHeader.extra_len.offset == 40
    assert C.sizeof(inf.GzipHeaderRow) == 96 and inf.GzipHeaderRow.msg.offset == 8 and inf.GzipHeaderRow.text_off.offset == 88
    heads = dfl.gzip_headers([dfl.GzipHeader.make(name=b"a"), dfl.GzipHeader.make(time=5, extra=b"xy", comment=b"c")])
    assert dfl.gzip_header_bytes(heads[0]) == 12 and dfl.gzip_header_bytes(heads[1]) == 16
    assert dfl.gzip_header_write(heads[1], 6, 0) == bytes.fromhex("1f8b0814" "05000000" "0003" "0200" "7879" "6300")


def test_refusals_through_ctypes_leave_the_results_alone():
    zr = importlib.import_module("zlib-ng_amd")
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    lib = zr.lib()
    jobs = (dfl.StreamJob * 1)()
    buf = (C.c_uint8 * 4096)()
    jobs[0].in_ptr = jobs[0].out_ptr = C.addressof(buf)
    jobs[0].in_len, jobs[0].out_cap = 64, 4096
    words = (C.c_uint64 * 2)(7, 8)
    head = dfl.GzipHeader.make(name=b"n" * 100, hcrc=True)
    s2, mem = lib.zng_rocm_compress_streams2_header_dev, lib.zng_rocm_compress_members_header_dev
    assert s2(6, 0, 15, C.byref(jobs), C.byref(head), 1, 0, None, None) == -3
    assert s2(6, 0, 16, C.byref(jobs), C.byref(head), 1, 0, C.addressof(words), None) == -3
    assert s2(6, 5, 15, C.byref(jobs), C.byref(head), 1, 0, C.addressof(words), None) == -3
    jobs[0].flags = 1                                 # a wrapped format takes no flags
    assert s2(6, 0, 15, C.byref(jobs), C.byref(head), 1, 0, C.addressof(words), None) == -3
    jobs[0].flags = 0
    bound = lib.zng_rocm_compress_streams2_bound(64, 2) - 10 + dfl.gzip_header_bytes(head)
    assert dfl.gzip_header_bytes(head) == 10 + 101 + 2
    jobs[0].out_cap = bound - 1
    assert s2(6, 0, 15, C.byref(jobs), C.byref(head), 1, 0, C.addressof(words), None) == -5
    head.extra_len = 3                                # extra_len without extra
    jobs[0].out_cap = 4096
    assert s2(6, 0, 15, C.byref(jobs), C.byref(head), 1, 0, C.addressof(words), None) == -3
    assert mem(6, 0, 15, C.byref(jobs), C.byref(head), 1, C.addressof(buf), 4096, 0, C.addressof(words), None, None) == -3
    head.extra_len = 0
    assert mem(6, 0, 15, C.byref(jobs), C.byref(head), 1, None, 1, 0, C.addressof(words), None, None) == -3
    if zr.device_count() > 0:
        return                                        # (a process without zng_rocm_init: the C consumer above)
    assert list(words) == [7, 8] and bytes(buf) == bytes(4096)
    assert s2(6, 0, 15, C.byref(jobs), C.byref(head), 1, 0, C.addressof(words), None) == -1 and list(words) == [7, 8]
