"""Build check (no GPU): the kernels of the gzip member finder (gzip_members.hip) -- the scan over the file with the candidate
rule (gzip_members_plan.h) inlined, the offsets scan, the scatter into the sorted candidate list, and the link kernel with the
BSIZE walk (framing_parse.h) and the binary search of next(i) inlined -- compile for gfx950 without scratch memory, VGPR spills
or out-of-line calls."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zlib-ng_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


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
                         int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", entry).group(1)),
                         int(re.search(r"\.max_flat_workgroup_size:\s*(\d+)", entry).group(1)))
    return kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_gzip_members_kernels():
    kernels = _kernels("gzip_members.hip")
    for name, threads in (("members_scan_kernel", 256), ("members_offsets_kernel", 256), ("members_scatter_kernel", 256),
                          ("members_link_kernel", 256)):
        hit = {k: v for k, v in kernels.items() if name in k}
        assert len(hit) == 1, (name, sorted(kernels))
        (scratch, spills, lds, wg), = hit.values()
        assert scratch == 0 and spills == 0, (name, scratch, spills)
        assert wg == threads, (name, wg)
        assert lds <= 16, (name, lds)                               # four words for the workgroup's sums, or none
    assert len(kernels) == 4, sorted(kernels)                       # the header kernels are framing_large.hip's, unchanged
