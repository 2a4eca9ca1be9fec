"""GPU: the coarse adapter (integration/arch/rocm/rocm_deflate.c) with zlib's strategies, switched mid-stream the way
deflateParams does it (a Z_BLOCK flush, then the new strategy), for raw, zlib and gzip streams; CPython's zlib reads the
result and verifies the trailer the adapter's check value went into."""
import zlib

import pytest

import strategy_util as su
import synth
from test_deflate_strategy_cpu import driver, run_driver  # noqa: F401  (the driver fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wrap", [0, 1, 2])
@pytest.mark.parametrize("order", ["30241", "2", "4", "3"])
def test_adapter_switches_strategy_mid_stream(driver, tmp_path, wrap, order):  # noqa: F811
    plain = su.run_heavy(3 << 20, seed=60 + wrap) + synth.silesia_like(3 << 20, seed=61 + wrap).tobytes()
    (tmp_path / "in.bin").write_bytes(plain)
    line = run_driver(driver, "d", 6, wrap, 700001, order, tmp_path / "in.bin", tmp_path / "out.z")
    assert line.startswith("device %d " % len(plain)), line
    comp = (tmp_path / "out.z").read_bytes()
    assert len(comp) == int(line.split()[2])
    wbits = {0: -15, 1: 15, 2: 31}[wrap]
    d = zlib.decompressobj(wbits)
    assert d.decompress(comp) == plain and d.eof and d.unused_data == b""
