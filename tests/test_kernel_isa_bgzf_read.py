"""Build check (no GPU): the kernels of BGZF random access (bgzf_read.hip) -- the index's link kernel with the BSIZE walk
(framing_parse.h) and the flag rule (bgzf_read_plan.h) inlined, and the slice kernel with the shared mover (bgzf_copy.h) inlined
-- compile for gfx950 without scratch memory, VGPR spills, LDS or out-of-line calls, and the slice kernel moves its bytes with
16-byte vector loads and stores."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zlib-ng_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_bgzf_read_kernels():
    tmp = tempfile.mkdtemp(prefix="zng_isa_")
    try:
        out = os.path.join(tmp, "k.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", out, os.path.join(CSRC, "bgzf_read.hip")], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert "s_swappc_b64" not in text, "a device function or lambda is called out of line"
    kernels = {}
    for entry in text.split("\n  - .agpr_count")[1:]:                   # one metadata entry per kernel
        name = re.search(r"\.name:\s*(\S+)", entry).group(1)
        kernels[name] = tuple(int(re.search(r"\.%s:\s*(\d+)" % key, entry).group(1)) for key in
                              ("private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size", "max_flat_workgroup_size"))
    for name in ("bgzf_index_link_kernel", "bgzf_slices_kernel"):
        hit = {k: v for k, v in kernels.items() if name in k}
        assert len(hit) == 1, (name, sorted(kernels))
        assert list(hit.values()) == [(0, 0, 0, 256)], (name, hit)
    assert len(kernels) == 2, sorted(kernels)                           # scan, scatter and headers are gzip_members.hip's
    body = text.split("bgzf_slices_kernel", 1)[1].split("s_endpgm", 1)[0]
    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body
