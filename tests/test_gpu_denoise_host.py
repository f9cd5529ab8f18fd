"""The denoiser through the C++ host layer: ipt_render --denoise
(GpuRenderer::render_m2 / guides / denoise over the C-ABI's host-buffer
forms) writes the bytes of the Python chain on the device: masked render with
m2 -> ipt_guides_device -> ipt_denoise_device -> ipt_display_device."""
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import adaptive_cases as ac
import denoise_cases as dn
import drift_cases as dc
from ipt_amd import capi, scenes
from test_display_cpu import read_png_gray8

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _python_chain(ctx, W, H, plane, iterations, sigma=None):
    """(denoised pixels, gray8) of the device chain, on the host."""
    n = W * H
    ctx.upload_scene(scenes.make_scene_box())
    img = {k: torch.zeros(n, dtype=torch.float32 if dt == np.float32 else torch.int32, device=DEV)
           for k, dt in dc.PLANE_KEYS}
    m2 = torch.zeros(n, dtype=torch.float32, device=DEV)
    g = torch.zeros(n * 32, dtype=torch.uint8, device=DEV)
    out = torch.zeros(n, dtype=torch.float32, device=DEV)
    g8 = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    flags = ac.FLAG[plane]
    p = capi.make_params(W, H, dn.RENDER_SPP, flags=flags, **dn.RENDER)
    ctx.render_masked_device_async(p, img["pixels"].data_ptr(), img["counters"].data_ptr(), img["sums"].data_ptr(),
                                   img["pixel_max"].data_ptr(), mask_ptr=None, m2_ptr=m2.data_ptr())
    ctx.guides_device(capi.make_params(W, H, 1, flags=flags), g.data_ptr())
    kw = {} if sigma is None else dict(sigma_l=sigma[0], normal_pow=sigma[1], sigma_z=sigma[2])
    ctx.denoise_device(capi.make_denoise_params(W, H, iterations=iterations, **kw), img["pixels"].data_ptr(),
                       img["counters"].data_ptr(), m2.data_ptr(), g.data_ptr(), out.data_ptr())
    ctx.display_device(capi.make_display_params(W, H), out.data_ptr(), g8.data_ptr())
    ctx.wait()
    torch.cuda.synchronize()
    return out.cpu().numpy(), g8.cpu().numpy()


@pytest.mark.parametrize("plane,sigma", ((dn.GRID, None), (dn.GUI, None), (dn.GRID, (8.0, 2, 0.05))))
def test_cli_denoise_matches_the_python_chain(gpu_ctx, oracle, tmp_path, plane, sigma):
    ge.build_host()
    W, H = 64, 48
    cmd = [str(ge.HOST_BIN), "--scene", "box", "--width", str(W), "--height", str(H), "--spp", str(dn.RENDER_SPP),
           "--n-rays", str(dn.RENDER["n_rays"]), "--depth", str(dn.RENDER["depth_max"]), "--denoise", "3",
           "--gpu-display", "--out", str(tmp_path / "o.png"), "--pfm", str(tmp_path / "o.pfm")]
    if plane == dn.GUI:
        cmd.append("--gui-plane")
    if sigma is not None:
        cmd += ["--denoise-sigma", "%r,%d,%r" % sigma]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out, g8 = _python_chain(gpu_ctx, W, H, plane, 3, sigma)
    img, m2 = dn.box_plane(W, H, plane=plane)
    kw = {} if sigma is None else dict(sigma_l=sigma[0], normal_pow=sigma[1], sigma_z=sigma[2])
    ro, _ = dn.denoise(img["pixels"], img["counters"], m2, dn.box_guides(W, H, plane), W, H, iterations=3, **kw)
    assert dn.same(out, ro).all() and not np.array_equal(ro, img["pixels"])
    raw = (tmp_path / "o.pfm").read_bytes()
    px = np.frombuffer(raw[raw.index(b"-1.0\n") + 5:], np.float32).reshape(H, W)[::-1].reshape(-1)
    assert np.array_equal(dc.bits(px), dc.bits(out))
    assert np.array_equal(read_png_gray8(tmp_path / "o.png").reshape(-1), g8)


def test_cli_denoise_composes_with_adaptive_and_keeps_its_rules(gpu_ctx, oracle, tmp_path):
    """--adaptive hands its m2 to the filter: the undenoised plane of the same
    command differs, the pixels that take no part (the row without a source,
    among others) are the same bytes."""
    ge.build_host()
    W, H = 37, 23
    base = [str(ge.HOST_BIN), "--scene", "box", "--width", str(W), "--height", str(H), "--spp", "16", "--n-rays", "4",
            "--depth", "3", "--adaptive", "0.05", "--out", ""]

    def pixels(extra, name):
        r = subprocess.run(base + extra + ["--pfm", str(tmp_path / name)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        raw = (tmp_path / name).read_bytes()
        return np.frombuffer(raw[raw.index(b"-1.0\n") + 5:], np.float32).reshape(H, W)[::-1]

    plain, filtered = pixels([], "a.pfm"), pixels(["--denoise", "2"], "b.pfm")
    assert not np.array_equal(plain, filtered)
    assert np.array_equal(dc.bits(plain[H - 1]), dc.bits(filtered[H - 1]))
    for extra, msg in ((["--denoise", "7"], "1..6"), (["--denoise", "2", "--passes", "2"], "one batch"),
                       (["--denoise", "2", "--denoise-sigma", "0,2,0.1"], "L > 0")):
        bad = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert bad.returncode == 2 and msg in bad.stderr, (extra, bad.stderr)
