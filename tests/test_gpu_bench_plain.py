"""A plain `bench.py --gpus 1 --steps K --warmup W` run: the result line with the headline figure
and ms_per_step, nothing that belongs to --full, and --dump-outputs writing the last timed frame
and the timed region's summed counters, both equal to the oracle's (C1: 256x256, the cheapest
workload)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cpu_baseline", "dropin", "dropin_ms_per_frame", "dropin_sync_ms_per_frame", "dropin_q4",
             "frame_sha256", "frame_sha_ok", "counters_ok")


def test_plain_run_line_and_dumped_outputs(tmp_path, oracle):
    import frm

    steps = 3
    out_dir = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "C1",
           "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=110, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["n_gpus"] == 1
    assert out["unit"] == "Gray-march-steps/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] > 0 and out["ms_per_step"] > 0 and isinstance(out["metric"], str)
    assert not [k for k in FULL_ONLY if k in out]
    assert out["roofline"]["traffic_source"] is None  # the PMC summary is --full's

    w = frm.WORKLOADS["C1"]
    ref = oracle.render(frm.make_parameters(w, pose="P1"), w.width, w.height, w.max_steps, flags=1)
    assert sorted(os.listdir(out_dir)) == ["counters.npy", "frame.npy"]
    px = np.load(out_dir / "frame.npy")
    assert px.dtype == np.float32 and px.shape == (w.width * w.height, 4)
    assert np.array_equal(px, ref["rgba"].reshape(-1, 4).astype(np.float32))
    c = np.load(out_dir / "counters.npy")
    assert c.dtype == np.float64
    assert c[:7].tolist() == [steps * int(v) for v in ref["counters"][:7]]
    # value is the counted march steps over the timed wall time
    march = c[2] + c[3]
    assert out["value"] == pytest.approx(march / (out["ms_per_step"] * 1e-3 * steps) / 1e9, rel=1e-9)
