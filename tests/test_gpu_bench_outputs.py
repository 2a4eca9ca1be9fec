"""bench.py --dump-outputs: the files hold what the timed path returned in its last step.  For the top-level line that is
the {adler32, crc32} of the rank's seeded shard: equal to the line's own `checksums`, to CPython zlib over the same
bytes, and the same in a second run with the same inputs.  A plain run carries none of the --full objects."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARD_MIB = 16


def _bench(out_dir, steps):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--settle", "0", "--shard-mib", str(SHARD_MIB), "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dump_outputs_hold_the_last_steps_checksums(tmp_path):
    line = _bench(tmp_path / "a", steps=3)
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert not {"streams", "deflate_lvl6", "inflate", "cpu_baseline"} & set(line)
    got = np.load(tmp_path / "a" / "checksums.npy")
    assert got.dtype == np.float64 and got.shape == (2,)
    assert [int(v) for v in got] == [int(h, 16) for h in line["config"]["checksums"]]
    # the same seeded shard, rebuilt here, through an independent implementation
    import torch
    import bench
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(bench.SEED)
    host = torch.randint(0, 256, (SHARD_MIB << 20,), dtype=torch.uint8, device="cuda:0", generator=gen).cpu().numpy()
    assert [int(v) for v in got] == [zlib.adler32(host), zlib.crc32(host)]
    # same inputs on the next run, whatever its step count
    _bench(tmp_path / "b", steps=5)
    assert np.array_equal(np.load(tmp_path / "b" / "checksums.npy"), got)
