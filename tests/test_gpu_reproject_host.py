"""Temporal reprojection through the C++ host layer: ipt_render
--reproject-from (GpuRenderer::render_m2 / guides / reproject over the C-ABI's
host-buffer forms) writes the bytes of the Python chain on the device: masked
render with m2 at the displaced camera -> guides -> the scene's own camera ->
guides -> ipt_reproject_device -> the masked render continued; and its
refusals hold."""
import json
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import adaptive_cases as ac
import drift_cases as dc
import reproject_cases as rc
from ipt_amd import capi, scenes

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F = np.float32
SHIFT = (0.15, 0.0, 0.05)
SPP = rc.RENDER_SPP


def _python_chain(ctx, W, H, plane, history_spp, sigma=None):
    """(pixels, counters, stats) of the device chain, on the host."""
    n = W * H
    flags = ac.FLAG[plane]
    box = scenes.make_scene_box()
    prev_cam = rc.move_camera(box["camera"], SHIFT)
    planes = [{k: torch.zeros(n, dtype=torch.float32 if dt == np.float32 else torch.int32, device=DEV)
               for k, dt in dc.PLANE_KEYS} for _ in range(2)]
    m2 = [torch.zeros(n, dtype=torch.float32, device=DEV) for _ in range(2)]
    g = [torch.zeros(n * 32, dtype=torch.uint8, device=DEV) for _ in range(2)]
    st = torch.zeros(4, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()

    def render(k, spp, offset):
        p = capi.make_params(W, H, spp, spp_offset=offset, flags=flags, **rc.RENDER)
        ctx.render_masked_device_async(p, planes[k]["pixels"].data_ptr(), planes[k]["counters"].data_ptr(),
                                       planes[k]["sums"].data_ptr(), planes[k]["pixel_max"].data_ptr(), mask_ptr=None,
                                       m2_ptr=m2[k].data_ptr())

    g1 = capi.make_params(W, H, 1, flags=flags)
    ctx.upload_scene(rc.with_camera(box, prev_cam))
    render(0, history_spp, 0)
    ctx.guides_device(g1, g[0].data_ptr())
    ctx.upload_scene(box)
    ctx.guides_device(g1, g[1].data_ptr())
    kw = {} if sigma is None else dict(sigma_z=sigma[0], normal_min=sigma[1], max_count=sigma[2])
    ctx.reproject_device(capi.make_reproject_params(W, H, prev_cam, flags=flags, **kw), planes[0]["pixels"].data_ptr(),
                         planes[0]["counters"].data_ptr(), m2[0].data_ptr(), g[0].data_ptr(), g[1].data_ptr(),
                         planes[1]["pixels"].data_ptr(), planes[1]["counters"].data_ptr(), m2[1].data_ptr(),
                         st.data_ptr())
    render(1, SPP, history_spp)
    ctx.wait()
    torch.cuda.synchronize()
    return (planes[1]["pixels"].cpu().numpy(), planes[1]["counters"].cpu().numpy().view(np.uint32),
            st.cpu().numpy().view(np.uint32))


def _cli(W, H, tmp_path, extra):
    return [str(ge.HOST_BIN), "--scene", "box", "--width", str(W), "--height", str(H), "--spp", str(SPP), "--n-rays",
            str(rc.RENDER["n_rays"]), "--depth", str(rc.RENDER["depth_max"]), "--out", "", "--pfm",
            str(tmp_path / "o.pfm"), "--counts", str(tmp_path / "o.u32")] + extra


@pytest.mark.parametrize("plane,history_spp,sigma", ((rc.GRID, None, None), (rc.GUI, None, None),
                                                      (rc.GRID, 7, (0.05, 0.5, 3))))
def test_cli_reproject_matches_the_python_chain(gpu_ctx, oracle, tmp_path, plane, history_spp, sigma):
    ge.build_host()
    W, H = 64, 48
    frm = "%r,%r,%r" % SHIFT + ("" if history_spp is None else ":%d" % history_spp)
    extra = ["--reproject-from", frm]
    if plane == rc.GUI:
        extra.append("--gui-plane")
    if sigma is not None:
        extra += ["--reproject-sigma", "%r,%r,%d" % sigma]
    r = subprocess.run(_cli(W, H, tmp_path, extra), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    px, cn, st = _python_chain(gpu_ctx, W, H, plane, history_spp or SPP, sigma)
    assert [line["reproject_reused"], line["reproject_disoccluded"], line["reproject_not_surface"]] == st[:3].tolist()
    assert st[0] > W * H // 2 and st[1] > 0 and int(st.sum()) == W * H
    # the reprojection is the restatement's (the planes' own test is tests/test_gpu_reproject.py)
    case = rc.rendered_case("box", "shift", W, H, plane, spp=history_spp or SPP)
    kw = {} if sigma is None else dict(sigma_z=sigma[0], normal_min=sigma[1], max_count=sigma[2])
    assert rc.reproject(*case[:5], W, H, case[5], plane, **kw)[3].tolist() == st.tolist()
    raw = (tmp_path / "o.pfm").read_bytes()
    got = np.frombuffer(raw[raw.index(b"-1.0\n") + 5:], np.float32).reshape(H, W)[::-1].reshape(-1)
    assert np.array_equal(dc.bits(got), dc.bits(px))
    assert np.array_equal(np.fromfile(tmp_path / "o.u32", np.uint32), cn)
    assert cn.max() > SPP + 1  # the counters continue the history


def test_cli_reproject_composes_and_keeps_its_rules(gpu_ctx, oracle, tmp_path):
    """--adaptive and --denoise take the reprojected second moments; more than
    one device, --preview and more than one batch are refused."""
    ge.build_host()
    W, H = 37, 23
    frm = ["--reproject-from", "0.15,0,0.05:8"]

    def run(extra):
        return subprocess.run(_cli(W, H, tmp_path, frm + extra), capture_output=True, text=True, timeout=120)

    def pixels():
        raw = (tmp_path / "o.pfm").read_bytes()
        return np.frombuffer(raw[raw.index(b"-1.0\n") + 5:], np.float32).copy()

    r = run([])
    assert r.returncode == 0, r.stderr
    plain = pixels()
    r = run(["--adaptive", "0.05", "--min-spp", "2", "--round-spp", "2"])
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["reproject_reused"] > 0 and 0 < line["adaptive_passes"] <= SPP
    r = run(["--denoise", "2", "--gpu-display", "--out", str(tmp_path / "o.png"), "--pgm", str(tmp_path / "o.pgm")])
    assert r.returncode == 0, r.stderr
    assert not np.array_equal(pixels(), plain) and (tmp_path / "o.png").stat().st_size > 0
    for extra, msg in ((["--devices", "0,0"], "one device"), (["--preview"], "--preview"), (["--passes", "2"], "one batch"),
                       (["--reproject-sigma", "0,0.9,64"], "Z > 0"), (["--reproject-sigma", "0.1,0.9,1"], "CAP")):
        bad = run(extra)
        assert bad.returncode == 2 and msg in bad.stderr, (extra, bad.stderr)
    bad = subprocess.run(_cli(W, H, tmp_path, ["--reproject-from", "0.1,0.2"]), capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "DX,DY,DZ" in bad.stderr
