"""GPU: a plain `python bench.py --gpus 1 --steps K --warmup W` prints the
headline line only, and `--dump-outputs DIR` writes what the last timed step
returned: every message's status and length, every message's byte sum, and
the bytes of a seeded sample of messages, which must be the plaintext the
inputs were compressed from."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSGS = 4096   # past the 2048-message threshold of the lane kernel, the headline's kernel


def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    import bench
    from beast_amd import synth

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--msgs", str(MSGS), "--dump-outputs", str(tmp_path)]
    env = {k: v for k, v in os.environ.items() if k != "WORLD_SIZE"}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    # value is the batch's uncompressed GiB over one step's time (ms_per_step is rounded to 1e-4 ms of a step
    # that takes some 0.1 ms, value to 1e-3 of some 100 GiB/s)
    assert line["value"] == pytest.approx(MSGS * bench.MSG_BYTES / (1 << 30) / (line["ms_per_step"] * 1e-3), rel=5e-3)
    # nothing besides the headline ran
    assert not {"parity_ok", "north_star", "cpu_baseline", "detail"} & set(line)

    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"status", "out_len", "out_msg_sum", "out_sample_index", "out_sample"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    raw, _, _ = synth.make_batch("json", np.full(MSGS, bench.MSG_BYTES, dtype=np.uint32), seed=bench.SEED_C2)
    raw = raw[: MSGS * bench.MSG_BYTES].reshape(MSGS, bench.MSG_BYTES)
    assert got["status"].shape == (MSGS,) and not got["status"].any()
    assert (got["out_len"] == bench.MSG_BYTES).all()
    assert np.array_equal(got["out_msg_sum"], raw.sum(axis=1, dtype=np.int64).astype(np.float64))
    idx = got["out_sample_index"].astype(np.int64)
    assert len(idx) == min(MSGS, bench.DUMP_SAMPLE_MSGS) and (np.diff(idx) > 0).all()
    assert np.array_equal(got["out_sample"], raw[idx].astype(np.float32))
