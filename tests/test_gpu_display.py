"""Display pipeline on the GPU (ipt_display_device / ipt_display, ipt_post.hip):
glare -> tone map -> 8-bit on device buffers, bit for bit against the CPU
reference of tests/display_ref.py (oracle glare pinned to the reference's
gui.cpp, numpy float32 folds, host libm powf). Device buffers are torch
tensors; every comparison is on bit patterns."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import display_ref as dr
from ipt_amd import capi, scenes
from test_display_cpu import read_png_gray8

pytestmark = pytest.mark.gpu

ONE = 0x3f800000
P = float(dr.GAMMA)


def run_device(ctx, px, W, H, cutoff=0.0, stream=None, offset=0, want=("processed", "tone")):
    """ipt_display_device on torch tensors; `offset` floats / bytes of slack in
    front of every buffer (unaligned base pointers)."""
    import torch

    n = W * H
    src = torch.zeros(n + offset, dtype=torch.float32, device="cuda")
    src[offset:] = torch.from_numpy(np.ascontiguousarray(px, np.float32).reshape(-1)).cuda()
    bufs = {k: torch.full((n + offset,), -7.0, dtype=torch.float32, device="cuda") for k in want}
    g8 = torch.full((n + offset,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def ptr(t):
        return t.data_ptr() + offset * t.element_size()

    ctx.display_device(capi.make_display_params(W, H, cutoff), ptr(src), ptr(g8),
                       ptr(bufs["processed"]) if "processed" in bufs else None,
                       ptr(bufs["tone"]) if "tone" in bufs else None, stream)
    ctx.wait()
    out = {k: v.cpu().numpy()[offset:] for k, v in bufs.items()}
    out["gray8"] = g8.cpu().numpy()[offset:]
    assert np.array_equal(src.cpu().numpy()[offset:].view(np.uint32), dr.bits(px).reshape(-1)), "input was written"
    for t in list(bufs.values()) + [g8]:  # nothing in front of the base pointer is touched
        head = t.cpu().numpy()[:offset]
        assert (head == (9 if t.dtype == torch.uint8 else -7.0)).all()
    return out


def assert_same(got, ref, keys=("processed", "tone", "gray8"), tag=None):
    for k in keys:
        a, b = (got[k], ref[k]) if k == "gray8" else (dr.bits(got[k]), dr.bits(ref[k]))
        bad = a != b
        assert not bad.any(), (tag, k, int(bad.sum()), np.flatnonzero(bad)[:5], a[bad][:5], b[bad][:5])


# ---- 1. powf ---------------------------------------------------------------
def test_powf_device_equals_host(gpu_ctx):
    pats = [np.arange(0, ONE + 1, 4093, dtype=np.uint64)]
    for c in (0, 0x00800000, ONE):
        pats.append(np.arange(max(c - 64, 0), c + 65, dtype=np.uint64))
    pats.append(np.array([0x80000000, 0x7f800000, 0x7fc00000], np.uint64))
    x = np.concatenate(pats).astype(np.uint32).view(np.float32)
    for y in (P, 0.6):
        a, b = dr.bits(gpu_ctx.powf_device(x, y)), dr.bits(capi.powf_host(x, y))
        bad = a != b
        assert not bad.any(), (y, dr.bits(x)[bad][:5], a[bad][:5], b[bad][:5])
    with pytest.raises(capi.IptError):
        gpu_ctx.powf_device(x, 2.0)


# ---- 2. glare stage against the reference's own gui.cpp glare() ------------
def test_glare_stage_matches_reference(gpu_ctx):
    cases = dr.glare_golden_cases()
    assert len(cases) == 9
    for W, H, cutoff, inp, ref in cases:
        got = run_device(gpu_ctx, inp, W, H, float(cutoff))
        assert np.array_equal(dr.bits(got["processed"]), dr.bits(ref)), (W, H, float(cutoff))


# ---- 3. compaction edges ---------------------------------------------------
def _dim(rng, n):
    return (rng.random(n, dtype=np.float32) * np.float32(0.49)).astype(np.float32)


def _compaction_cases():
    rng = np.random.default_rng(17)
    out = []

    def hot(k):
        return (rng.random(k, dtype=np.float32) * 40 + np.float32(1.5)).astype(np.float32)

    out.append(("none", 64, 48, _dim(rng, 64 * 48)))
    for k in (512, 513):  # the glare kernel's LDS chunk
        img = _dim(rng, 64 * 48)
        img[rng.choice(64 * 48, k, replace=False)] = hot(k)
        out.append((f"{k}_bright", 64, 48, img))
    img = _dim(rng, 97 * 33)
    m = rng.random(97 * 33) < 0.2
    img[m] = hot(int(m.sum()))
    out.append(("20_percent", 97, 33, img))
    out.append(("all_bright", 40, 30, hot(40 * 30)))
    img = _dim(rng, 300 * 200)
    img[[0, 300 * 100 + 150, 300 * 200 - 1]] = hot(3)
    out.append(("empty_blocks", 300, 200, img))
    img = _dim(rng, 257 * 3)
    for y in range(3):
        img[y * 257 + 255] = 7.0 + y
        img[y * 257 + 256] = 3.0 + y
    out.append(("block_edge", 257, 3, img))
    out = [c + (1.0,) for c in out]
    # (with cutoff 1 the denser cases saturate to the cutoff everywhere; here the
    # halos stay below it, so the order of the float sums shows in the result)
    img = _dim(rng, 97 * 33)
    m = rng.random(97 * 33) < 0.2
    img[m] = (hot(int(m.sum())) + np.float32(50.0)).astype(np.float32)
    out.append(("20_percent_unsaturated", 97, 33, img, 50.0))
    return out


@pytest.mark.parametrize("name,W,H,img,cutoff", _compaction_cases(), ids=[c[0] for c in _compaction_cases()])
def test_compaction_edges(gpu_ctx, oracle, name, W, H, img, cutoff):
    if name.endswith("_bright") and name[0].isdigit():
        assert int((img > cutoff).sum()) == int(name.split("_")[0])
    ref = dr.display_ref(img, W, H, cutoff)
    if name.endswith("unsaturated"):
        assert (ref["processed"] < cutoff).sum() > 0.5 * W * H
    assert_same(run_device(gpu_ctx, img, W, H, cutoff), ref, tag=name)


# ---- 4. tone and 8-bit, no glare -------------------------------------------
def _tone_cases():
    rng = np.random.default_rng(23)
    rnd = (rng.random(64 * 48, dtype=np.float32) * np.float32(3.0)).astype(np.float32)
    rnd[7] = 0.0
    nan0, nan100, inf1 = rnd.copy(), rnd.copy(), rnd.copy()
    nan0[0] = np.nan
    nan100[100] = np.nan
    inf1[1234] = np.inf
    mixed = (rnd - np.float32(1.5)).astype(np.float32)  # negative quotients: powf -> NaN
    zeros_max = -rnd[:35].copy()
    zeros_max[[4, 9]] = [-0.0, 0.0]  # the maximum is the FIRST zero: -0, so x / mx = +inf for x < 0
    small = (rng.random(21, dtype=np.float32) + np.float32(0.1)).astype(np.float32)
    return [("random", 64, 48, rnd), ("nan_first", 64, 48, nan0), ("nan_100", 64, 48, nan100),
            ("zeros", 64, 48, np.zeros(64 * 48, np.float32)), ("constant", 64, 48, np.full(64 * 48, 0.3, np.float32)),
            ("negative", 64, 48, (-rnd - np.float32(0.5)).astype(np.float32)), ("one_inf", 64, 48, inf1),
            ("mixed_sign", 64, 48, mixed), ("zero_max_sign", 7, 5, zeros_max),
            ("1x1", 1, 1, small[:1]), ("5x1", 5, 1, small[:5]), ("3x7", 3, 7, small)]


@pytest.mark.parametrize("name,W,H,img", _tone_cases(), ids=[c[0] for c in _tone_cases()])
def test_tone_and_gray8(gpu_ctx, name, W, H, img):
    ref = dr.display_ref(img, W, H)
    got = run_device(gpu_ctx, img, W, H)
    assert_same(got, ref, tag=name)
    if name == "zeros":
        assert np.isnan(got["tone"]).all() and not got["gray8"].any()
    if name in ("constant", "nan_first"):
        assert not got["gray8"].any()
    if name == "random":
        assert got["gray8"].min() == 0 and got["gray8"].max() == 255


def test_unaligned_base_pointers(gpu_ctx, oracle):
    """Every buffer one float (one byte for gray8) past its allocation: the
    vector loads and stores must fall back, and touch nothing outside."""
    rng = np.random.default_rng(29)
    W, H = 67, 13
    img = (rng.random(W * H, dtype=np.float32) * np.float32(2.0)).astype(np.float32)
    assert_same(run_device(gpu_ctx, img, W, H, offset=1), dr.display_ref(img, W, H), tag="no glare")
    assert_same(run_device(gpu_ctx, img, W, H, 1.01, offset=1), dr.display_ref(img, W, H, 1.01), tag="glare")


# ---- 5. whole chain ---------------------------------------------------------
def test_whole_chain_gui_cutoff(gpu_ctx, oracle):
    rng = np.random.default_rng(31)
    W, H = 97, 33
    img = _dim(rng, W * H)
    m = rng.random(W * H) < 0.03
    img[m] = (rng.random(int(m.sum()), dtype=np.float32) * 40 + np.float32(1.5)).astype(np.float32)
    ref = dr.display_ref(img, W, H, 1.01)
    assert_same(run_device(gpu_ctx, img, W, H, 1.01), ref)
    # the optional outputs left out: the context's scratch carries them
    assert_same(run_device(gpu_ctx, img, W, H, 1.01, want=()), ref, keys=("gray8",))


# ---- 6. stream order --------------------------------------------------------
def test_stream_order_after_async_render(gpu_ctx):
    """render_device_async then display_device on one torch stream, no wait
    between them: the display reads the finished plane."""
    import torch

    W, H = 32, 32
    gpu_ctx.upload_scene(scenes.make_scene_box())
    p = capi.make_params(W, H, 2, n_rays=16, depth_max=8)
    A = torch.zeros(4, H, W, dtype=torch.float32, device="cuda")
    B = torch.zeros(4, H, W, dtype=torch.float32, device="cuda")
    g8 = torch.zeros(W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gpu_ctx.render_device_async(p, *(A[i].data_ptr() for i in range(4)), s.cuda_stream)
        gpu_ctx.display_device(capi.make_display_params(W, H), A[0].data_ptr(), g8.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    got = g8.cpu().numpy()
    gpu_ctx.wait()
    gpu_ctx.render_device(p, *(B[i].data_ptr() for i in range(4)), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plane = B[0].cpu().numpy().reshape(-1)
    assert plane.max() > 0
    assert np.array_equal(got, dr.display_ref(plane, W, H)["gray8"])


# ---- 7. host buffers, argument errors --------------------------------------
def test_host_display_equals_device_and_rejects_bad_arguments(gpu_ctx, oracle):
    rng = np.random.default_rng(37)
    W, H = 53, 21
    img = (rng.random(W * H, dtype=np.float32) * np.float32(1.6)).astype(np.float32)
    for cutoff in (0.0, 1.01):
        assert_same(gpu_ctx.display(img, W, H, cutoff), run_device(gpu_ctx, img, W, H, cutoff), tag=cutoff)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    g8 = np.zeros(W * H, np.uint8)

    def rc(params, px=img.ctypes.data, out=g8.ctypes.data):
        return lib.ipt_display(h, C.byref(params), px, None, None, out)

    assert rc(capi.make_display_params(W, H), px=None) == capi.IPT_E_INVALID
    assert rc(capi.make_display_params(W, H), out=None) == capi.IPT_E_INVALID
    assert lib.ipt_display(h, None, img.ctypes.data, None, None, g8.ctypes.data) == capi.IPT_E_INVALID
    assert rc(capi.make_display_params(0, H)) == capi.IPT_E_INVALID
    assert rc(capi.make_display_params(W, -1)) == capi.IPT_E_INVALID
    assert rc(capi.make_display_params(W, H, -1.0)) == capi.IPT_E_INVALID
    assert rc(capi.make_display_params(W, H, float("nan"))) == capi.IPT_E_INVALID
    wide = np.zeros(4097, np.float32)
    wg = np.zeros(4097, np.uint8)
    assert rc(capi.make_display_params(4097, 1, 1.01), wide.ctypes.data, wg.ctypes.data) == capi.IPT_E_UNSUPPORTED
    assert rc(capi.make_display_params(1, 4097, 1.01), wide.ctypes.data, wg.ctypes.data) == capi.IPT_E_UNSUPPORTED
    assert rc(capi.make_display_params(4097, 1, 0.0), wide.ctypes.data, wg.ctypes.data) == capi.IPT_OK
    with pytest.raises(capi.IptError) as e:
        gpu_ctx.display(img, W, H, -2.0)
    assert e.value.code == capi.IPT_E_INVALID
    # the device call validates the same way (nothing is launched)
    dp = capi.make_display_params(W, H)
    assert lib.ipt_display_device(h, C.byref(dp), None, None, None, None, None) == capi.IPT_E_INVALID


# ---- 8. scratch regrowth ----------------------------------------------------
def test_scratch_regrowth(oracle):
    rng = np.random.default_rng(41)
    ctx = capi.Context(0)
    try:
        small = _dim(rng, 64 * 48)
        small[rng.choice(64 * 48, 40, replace=False)] = 5.0
        big = _dim(rng, 300 * 200)
        big[rng.choice(300 * 200, 300, replace=False)] = 9.0
        first = run_device(ctx, small, 64, 48, 1.01, want=())
        second = run_device(ctx, big, 300, 200, 1.01, want=())
        third = run_device(ctx, small, 64, 48, 1.01, want=())
        assert_same(first, dr.display_ref(small, 64, 48, 1.01), keys=("gray8",))
        assert_same(second, dr.display_ref(big, 300, 200, 1.01), keys=("gray8",))
        assert np.array_equal(first["gray8"], third["gray8"])
    finally:
        ctx.close()


# ---- 9. CLI -----------------------------------------------------------------
def test_cli_gpu_display_png_is_identical(tmp_path):
    exe = ge.build_host()
    args = [str(exe), "--scene", "box", "--spp", "2", "--width", "40", "--height", "24"]
    subprocess.run(args + ["--out", str(tmp_path / "cpu.png")], check=True, capture_output=True, timeout=120)
    subprocess.run(args + ["--gpu-display", "--out", str(tmp_path / "gpu.png")], check=True, capture_output=True,
                   timeout=120)
    a, b = (tmp_path / "cpu.png").read_bytes(), (tmp_path / "gpu.png").read_bytes()
    assert a == b
    assert read_png_gray8(tmp_path / "gpu.png").max() == 255
