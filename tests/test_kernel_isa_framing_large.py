"""Build check (no GPU): the kernels of the wrapped large calls (framing_large.hip) -- the header kernel with the shared
wrapper rules (framing_parse.h) and the wavefront-wide terminator search inlined, the FHCRC compare, the kernel that writes the
descriptors of the sub-messages from messages passed as kernel arguments, the segmented fold of their checks and the trailer
compare -- compile for gfx950 without scratch memory, VGPR spills or out-of-line
calls."""
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
def test_framing_large_kernels():
    kernels = _kernels("framing_large.hip")
    for name, threads in (("large_header_kernel", 64), ("large_hcrc_kernel", 256), ("large_cut_kernel", 256), ("large_fold_kernel", 256),
                          ("large_trailer_kernel", 256)):
        hit = {k: v for k, v in kernels.items() if name in k}
        assert len(hit) == 1, (name, sorted(kernels))
        (scratch, spills, lds, wg), = hit.values()
        assert scratch == 0 and spills == 0, (name, scratch, spills)
        assert wg == threads, (name, wg)                            # the header kernel is one wavefront per member
    assert len(kernels) == 5, sorted(kernels)                       # the checksum pass itself is checksum.hip's
