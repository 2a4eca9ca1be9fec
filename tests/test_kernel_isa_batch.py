"""Build check (no GPU): every kernel added or changed for zng_rocm_inflate_large_streams_dev -- the finder over a stream
table, which the one-stream calls use as a table of one (inflate_large.hip), the part kernel with the runtime bound on
the start search and the sync kernel whose regions name their stream (inflate_dev.hip), and the kernels the batch resolve
launches (inflate_resolve.hip) -- compiles for gfx950 without scratch memory, VGPR spills or out-of-line calls.  The batch
launches the part kernel's existing instantiations and no other: their LDS is what sets 12 (plain layout) or 13 (packed)
parts per CU of 160 KiB, and a SUB part takes no more than the flags-0 part of the same ring and layout."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zlib-ng_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 << 10


def _kernels(source):
    tmp = tempfile.mkdtemp(prefix="zng_isa_")
    try:
        out = os.path.join(tmp, "k.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", out, os.path.join(CSRC, source)], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert "s_swappc_b64" not in text, source + ": a device function or lambda is called out of line"
    kernels = {}
    for entry in text.split("\n  - .agpr_count")[1:]:               # one metadata entry per kernel
        name = re.search(r"\.name:\s*(\S+)", entry).group(1)
        kernels[name] = (int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", entry).group(1)),
                         int(re.search(r"\.vgpr_spill_count:\s*(\d+)", entry).group(1)),
                         int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", entry).group(1)))
    return kernels


def _clean(kernels, pattern, count):
    hit = {k: v for k, v in kernels.items() if re.search(pattern, k)}
    assert len(hit) == count, (pattern, sorted(kernels))
    for k, (scratch, spills, _) in hit.items():
        assert scratch == 0 and spills == 0, (k, scratch, spills)
    return hit


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_finder_and_compaction_kernels():
    kernels = _kernels("inflate_large.hip")
    table = _clean(kernels, r"find_headers_table_kernelILb[01]E", 2)
    # one stream is a table of one: no one-stream form of the scan or of the header check is left
    _clean(kernels, r"find_headers_kernelILb", 0)
    _clean(kernels, r"validate_headers_kernel", 0)
    _clean(kernels, r"validate_headers_table_kernel", 1)
    _clean(kernels, r"first_bytes_kernel", 1)
    _clean(kernels, r"compact_parts_kernel", 1)
    # the scan's LDS: the per-workgroup survivor list (2048 x 8 bytes) and its two counters; with the bit positions, the Kraft
    # table (512 bytes) as well
    assert sorted(v[2] for v in table.values()) == [16392, 16904]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_part_and_sync_kernels_keep_their_lds():
    kernels = _kernels("inflate_dev.hip")
    _clean(kernels, r"subblock_sync_kernel", 1)
    # ring 4096, PART: plain / packed layout, each without and with SUB -- the four the one-stream call launches too
    parts = _clean(kernels, r"inflate_streams_kernelILi4096ELb1ELb[01]ELb[01]E", 4)
    for k, (_, _, lds) in parts.items():
        packed = "ELb1ELb1ELb" in k
        assert lds * (13 if packed else 12) <= LDS_PER_CU, (k, lds)
        if k.endswith("ELb1EEEvPKNS_13InflateJobDevEjPjPKyS4_"):   # SUB: no more than the flags-0 part of the same layout
            plain = k.replace("ELb1EEEv", "ELb0EEEv")
            assert plain in parts and lds <= parts[plain][2], (k, lds)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_resolve_kernels_of_the_batch():
    kernels = _kernels("inflate_resolve.hip")
    for name in ("inflate_windows_kernel", "inflate_context_group_kernel", "inflate_context_chain_kernel", "inflate_translate_kernel"):
        _clean(kernels, name, 1)
