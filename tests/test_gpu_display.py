"""Display pipeline on the GPU (ipt_display_device / ipt_display, ipt_post.hip):
glare -> tone map -> 8-bit on device buffers, bit for bit against the CPU
reference of tests/display_ref.py (oracle glare pinned to the reference's
gui.cpp, numpy float32 folds, host libm powf). Device buffers are torch
tensors; every comparison is on bit patterns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import display_cases as dc
import display_ref as dr
from ipt_amd import capi, scenes
from test_display_cpu import read_png_gray8

pytestmark = pytest.mark.gpu

ONE = 0x3f800000
P = float(dr.GAMMA)
EXHAUSTIVE = os.environ.get("IPT_EXHAUSTIVE") == "1"


def run_device(ctx, px, W, H, cutoff=0.0, stream=None, offset=0, want=("processed", "tone")):
    """ipt_display_device on torch tensors; `offset` floats / bytes of slack in
    front of every buffer (unaligned base pointers)."""
    import torch

    n = W * H
    src = torch.zeros(n + offset, dtype=torch.float32, device="cuda")
    src[offset:] = torch.from_numpy(np.array(px, np.float32).reshape(-1)).cuda()  # (a copy: px may be read-only)
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


def queue_device(ctx, src, g8, W, H, cutoff, stream):
    """ipt_display_device on `stream` with NULL processed / tone (the context's
    scratch carries them); queues only, no synchronisation of any kind."""
    ctx.display_device(capi.make_display_params(W, H, cutoff), src.data_ptr(), g8.data_ptr(), None, None,
                       stream.cuda_stream)


def assert_same(got, ref, keys=("processed", "tone", "gray8"), tag=None):
    for k in keys:
        a, b = (got[k], ref[k]) if k == "gray8" else (dr.bits(got[k]), dr.bits(ref[k]))
        bad = a != b
        assert not bad.any(), (tag, k, int(bad.sum()), np.flatnonzero(bad)[:5], a[bad][:5], b[bad][:5])


# ---- 1. powf ---------------------------------------------------------------
def _assert_powf(gpu_ctx, x, y):
    a, b = dr.bits(gpu_ctx.powf_device(x, y)), dr.bits(capi.powf_host(x, y))
    bad = a != b
    assert not bad.any(), (y, dr.bits(x)[bad][:5], a[bad][:5], b[bad][:5])


def _powf_sweep(gpu_ctx, stride):
    """Every stride-th float of [0, 1] in chunks of 2^24 inputs, then the
    windows around 0, the smallest normal and 1, for y = 1/2.2 and 0.6."""
    pats = []
    for c in (0, 0x00800000, ONE):
        pats.append(np.arange(max(c - 64, 0), c + 65, dtype=np.uint64))
    pats.append(np.array([0x80000000, 0x7f800000, 0x7fc00000], np.uint64))
    edges = np.concatenate(pats).astype(np.uint32).view(np.float32)
    chunk = (1 << 24) * stride
    for y in (P, 0.6):
        for s in range(0, ONE + 1, chunk):
            x = np.arange(s, min(ONE + 1, s + chunk), stride, dtype=np.uint64).astype(np.uint32).view(np.float32)
            _assert_powf(gpu_ctx, x, y)
        _assert_powf(gpu_ctx, edges, y)
    return edges


def test_powf_device_equals_host(gpu_ctx):
    """The device's powf_ against the library's host build of the same source
    (equal to libm on all of [0, 1], tests/test_display_cpu.py): every 61st
    float of [0, 1], 17.5 M inputs, the sweep of tests/test_math_exhaustive.py."""
    edges = _powf_sweep(gpu_ctx, 61)
    with pytest.raises(capi.IptError):
        gpu_ctx.powf_device(edges, 2.0)


if EXHAUSTIVE:  # IPT_EXHAUSTIVE=1, as in tests/test_math_exhaustive.py
    @pytest.mark.slow
    def test_powf_device_equals_host_exhaustive(gpu_ctx):
        """All 1 065 353 217 floats of [0, 1], both exponents."""
        _powf_sweep(gpu_ctx, 1)


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


@pytest.mark.parametrize("W,H", dc.SCAN_SHAPES, ids=[f"{W}x{H}" for W, H in dc.SCAN_SHAPES])
def test_compaction_above_256_blocks(gpu_ctx, oracle, W, H):
    """bright_scan_kernel at and past one block per scan thread (256, 257, 260
    and 400 blocks): 300 distinct bright values on either side of the scan
    threads' boundaries, the image unsaturated so that a reordered, dropped or
    duplicated record changes the float sums (conditions in dc.scan_ref)."""
    ref = dc.scan_ref(W, H)
    img, pos = dc.scan_case(W, H)
    nblk, per, used = dc.scan_geometry(W * H)
    assert (per == 1 and used == 256) if (W, H) == (512, 512) else (per == 2 and used < 256 and nblk > 256)
    assert int((img > dc.SCAN_CUTOFF).sum()) == len(pos) == dc.SCAN_BRIGHT
    assert_same(run_device(gpu_ctx, img, W, H, dc.SCAN_CUTOFF), ref, tag=(W, H))
    if (W, H) == (640, 640):  # once more through the context's scratch buffers
        assert_same(run_device(gpu_ctx, img, W, H, dc.SCAN_CUTOFF, want=()), ref, keys=("gray8",), tag="scratch")


@pytest.mark.parametrize("cx,cy", dc.FAR_CORNERS, ids=["top_left", "bottom_right"])
def test_far_halo_display(gpu_ctx, oracle, cx, cy):
    """glare_kernel's s >= 2^24 branch (the device's f64 root) through
    ipt_display_device: 4096 x 512 zeros and one bright corner, so that every
    output pixel is the halo term itself (601 pixels differ between the two
    radius formulas, tests/test_display_cpu.py). The scan runs at per = 8."""
    ref = dc.far_ref(cx, cy)
    assert int(np.count_nonzero(ref["processed"])) == dc.FAR_W * dc.FAR_H
    assert_same(run_device(gpu_ctx, dc.far_image(cx, cy), dc.FAR_W, dc.FAR_H, dc.FAR_CUTOFF), ref, tag=(cx, cy))


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
            ("1x1", 1, 1, small[:1]), ("5x1", 5, 1, small[:5]), ("3x7", 3, 7, small)] + dc.denormal_tone_cases()


_DENORMAL_CASES = {c[0] for c in dc.denormal_tone_cases()}


@pytest.mark.parametrize("name,W,H,img", _tone_cases(), ids=[c[0] for c in _tone_cases()])
def test_tone_and_gray8(gpu_ctx, name, W, H, img):
    ref = dr.display_ref(img, W, H)
    if name in _DENORMAL_CASES:  # subnormal mx, subnormal quotients, a span of a few ulps: stated there
        dc.check_denormal_tone_case(name, img, ref)
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


def test_two_streams_share_the_scratch(oracle):
    """Two display calls on two streams with no host wait between them: the
    second must run behind the first (hipStreamWaitEvent on the context's
    event), because both use the context's scalars, bright list and
    processed / tone scratch. L (256 x 256, 2000 bright pixels: a glare kernel
    of 1.3e8 terms) and S (64 x 48, 40 bright) alternate over four pairs, after
    a warm-up that grows the scratch so that no call takes the allocating path,
    which waits on the host.

    An ordering test is probabilistic: it cannot prove that the wait is there,
    it only fails with good likelihood when it is missing (the long call is then
    still running when the short one rewrites the shared scalars and list)."""
    import torch

    cases = dc.stream_cases()
    refs = {k: dc.stream_ref(k) for k in cases}
    ctx = capi.Context(0)
    try:
        src = {k: torch.from_numpy(np.array(img)).cuda() for k, (W, H, img) in cases.items()}
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        (WL, HL, _), out = cases["L"], []
        warm = torch.zeros(WL * HL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        queue_device(ctx, src["L"], warm, WL, HL, dc.STREAM_CUTOFF, s1)
        ctx.wait()
        for first, second in (("L", "S"), ("S", "L"), ("L", "S"), ("S", "L")):
            pair = [(key, torch.full((cases[key][0] * cases[key][1],), 9, dtype=torch.uint8, device="cuda"))
                    for key in (first, second)]
            torch.cuda.synchronize()
            for (key, g8), stream in zip(pair, (s1, s2)):
                W, H, _ = cases[key]
                queue_device(ctx, src[key], g8, W, H, dc.STREAM_CUTOFF, stream)
            ctx.wait()
            torch.cuda.synchronize()
            out += pair
        assert np.array_equal(warm.cpu().numpy(), refs["L"]["gray8"])
        for i, (key, g8) in enumerate(out):
            got = g8.cpu().numpy()
            bad = got != refs[key]["gray8"]
            assert not bad.any(), (i, key, int(bad.sum()), np.flatnonzero(bad)[:5])
    finally:
        ctx.close()


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
