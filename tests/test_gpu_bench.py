"""bench.py's contract: a plain run prints one result line with the headline fields and nothing of the --full legs,
`--steps` is the number of timed steps, and `--dump-outputs` writes the last timed step's arrays as float32 .npy files"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_plain_line_and_dump_outputs(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["unit"] == "vol/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) / d["value"] < 0.01    # batch 2 per step
    assert not {"roofline", "cpu_baseline", "sliding_window"} & set(d)
    files = sorted(os.listdir(out))
    assert files == ["logits.npy", "loss.npy", "params.npy"]
    arrs = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert arrs["logits"].shape == (2, 3, 96, 96, 96)
    assert abs(float(arrs["loss"][0]) - d["config"]["final_loss"]) < 1e-4
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
