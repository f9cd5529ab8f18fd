"""A plain bench.py run and `--dump-outputs` (one small run of the CLI).

A plain run (no `--full`) times its steps and prints the result line with the
headline keys; what `--full` adds (the counting re-render's `roofline` and
`events_per_path`, the CPU-baseline leg) is null. `--dump-outputs DIR` writes
the GridRenderPlane arrays the timed steps left: two queued 2-spp steps of a
96 x 80 frame (not a multiple of the 16-row tile or the 64-lane wave) must be
bit-identical to the oracle's replay of the same four passes.
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_binding as ob
from ipt_amd import capi, scenes

ROOT = Path(__file__).resolve().parents[1]
W, H, SPP, STEPS = 96, 80, 2, 2


@pytest.mark.gpu
def test_plain_run_result_line_and_dumped_outputs(oracle, tmp_path):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--width", str(W), "--height", str(H),
           "--spp-per-step", str(SPP), "--steps", str(STEPS), "--warmup", "1", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == STEPS and d["warmup"] == 1 and d["config"]["spp"] == SPP * STEPS
    assert d["unit"] == "Mpaths/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0
    # value and ms_per_step are the same measurement
    assert d["value"] == pytest.approx(W * H * SPP / (d["ms_per_step"] * 1e3), rel=1e-9)
    for k in ("roofline", "cpu_baseline", "gpu_vs_cpu", "events_per_path", "mrays_per_s"):
        assert d[k] is None, k

    ov, oc = ob.render_values(scenes.make_scene_box(), capi.make_params(W, H, SPP * STEPS))
    ref = ob.accumulate(ov, oc)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["counters.npy", "pixel_max.npy", "pixels.npy",
                                                                     "sums.npy"]
    for k in ("pixels", "sums", "pixel_max"):
        a = np.load(tmp_path / "out" / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == (H, W)
        assert np.array_equal(a.reshape(-1).view(np.uint32), ref[k].view(np.uint32)), k
    c = np.load(tmp_path / "out" / "counters.npy")
    assert c.dtype == np.float64 and np.array_equal(c.reshape(-1), ref["counters"])
    assert d["mean_pixel"] == pytest.approx(float(np.load(tmp_path / "out" / "pixels.npy").mean()), rel=1e-5)
