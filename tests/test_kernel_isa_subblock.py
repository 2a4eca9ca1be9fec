"""Build check (no GPU): the kernels of ZNG_ROCM_INFLATE_SUBBLOCK -- subblock_sync_kernel and the part kernel's SUB
instantiations (inflate_dev.hip) -- compile for gfx950 without scratch memory, VGPR spills or out-of-line calls, and a SUB
part takes no more LDS than the flags-0 part of the same ring and layout (LDS is what bounds the parts per CU)."""
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
def test_subblock_kernels_no_scratch_no_calls_same_lds():
    tmp = tempfile.mkdtemp(prefix="zng_isa_")
    try:
        out = os.path.join(tmp, "k.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", out, os.path.join(CSRC, "inflate_dev.hip")], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert "s_swappc_b64" not in text, "a device function or lambda is called out of line"
    kernels = {}
    for entry in text.split("\n  - .agpr_count")[1:]:               # one metadata entry per kernel
        name = re.search(r"\.name:\s*(\S+)", entry).group(1)
        kernels[name] = (int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", entry).group(1)),
                         int(re.search(r"\.vgpr_spill_count:\s*(\d+)", entry).group(1)),
                         int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", entry).group(1)))
    sync = [k for k in kernels if "subblock_sync_kernel" in k]
    sub = {k: v for k, v in kernels.items() if re.search(r"inflate_streams_kernelILi4096ELb1ELb[01]ELb1E", k)}
    assert len(sync) == 1 and len(sub) == 2, sorted(kernels)
    for k in sync + list(sub):
        scratch, spills, _ = kernels[k]
        assert scratch == 0 and spills == 0, (k, scratch, spills)
    for k, (_, _, lds) in sub.items():
        plain = k.replace("ELb1EEEv", "ELb0EEEv")                    # the same ring and layout, flags 0
        assert plain in kernels, (k, sorted(kernels))
        assert lds <= kernels[plain][2], (k, lds, kernels[plain][2])
