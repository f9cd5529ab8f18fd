"""The adaptive loop through the C++ host layer: ipt_render --adaptive
(GpuRenderer::render_adaptive over ipt_render_adaptive) writes the plane of
tests/adaptive_cases.py's numpy loop and reports its passes and active count."""
import json
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import adaptive_cases as ac
import drift_cases as dc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("plane", ac.PLANES)
def test_cli_adaptive_matches_the_numpy_loop(gpu_ctx, oracle, tmp_path, plane):
    ge.build_host()
    W, H = ac.LOOP_FRAMES[0]
    a = ac.LOOP_ADAPT
    cmd = [str(ge.HOST_BIN), "--scene", "box", "--width", str(W), "--height", str(H), "--spp", str(ac.LOOP_SPP),
           "--n-rays", str(dc.N_RAYS), "--depth", str(dc.DEPTH_MAX), "--adaptive", repr(a["rel_tol"]),
           "--adaptive-abs", repr(a["abs_tol"]), "--min-spp", str(a["min_count"]), "--round-spp", str(ac.LOOP_ROUND),
           "--out", "", "--pfm", str(tmp_path / "r.pfm"), "--counts", str(tmp_path / "r.u32")]
    if plane == ac.GUI:
        cmd.append("--gui-plane")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    v, _, _ = dc.oracle_samples(W, H, ac.LOOP_SPP)
    rounds, used = ac.loop(v, ac.codes_of(W, H, ac.LOOP_SPP, plane), plane, ac.LOOP_ROUND, **a)
    img, _, _, stats = rounds[-1]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert (out["adaptive_passes"], out["adaptive_active"]) == (used, int(stats[0]))
    raw = (tmp_path / "r.pfm").read_bytes()
    px = np.frombuffer(raw[raw.index(b"-1.0\n") + 5:], np.float32).reshape(H, W)[::-1].reshape(-1)
    assert np.array_equal(np.fromfile(tmp_path / "r.u32", np.uint32), img["counters"])
    assert np.array_equal(dc.bits(px), dc.bits(img["pixels"]))
    # the options' own rules
    bad = subprocess.run(cmd + ["--passes", "2"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "one batch" in bad.stderr
