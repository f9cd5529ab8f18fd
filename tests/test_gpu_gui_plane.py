"""IPT_FLAG_GUI_PLANE on the GPU: the Gui's render plane (gui.cpp:165-182), the
one the reference program renders into, displays and saves, bit for bit
against its numpy restatement (tests/gui_cases.py; tests/test_gui_plane_cpu.py
ties that to the oracle).

new_path_setup writes the codes relative to the Gui's nominal row H-1-iy,
accumulate_kernel<kPlaneGui> replays them: one nominal source row per
destination row (no doubled row 0), a drift branch over source rows H-2-yi ..
H-yi, and ipt_shard_plan's candidates under the same map. The frames are the
drift frames (hundreds of drifted samples per pass along x and y) and the
renders that hold what the two planes differ in: a top clamp (source row 0,
raw row H, brought back to H-1) and a bottom sample (source row H-1 into row
1). Radiance is the oracle's: the same (x, y) gives the same camera ray
whatever plane receives it. Tree: n_rays 4, depth_max 3."""
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import display_ref as dr
import drift_cases as dc
import gui_cases as gc
import oracle_binding as ob
from ipt_amd import capi, scenes

pytestmark = pytest.mark.gpu

bits = dc.bits
KEYS = tuple(k for k, _ in dc.PLANE_KEYS)
FLAG = gc.FLAG

# (W, H, spp, spp_offset)
WHOLE = ((60000, 3, 2, 0), (60000, 3, 9, 0), (3, 60000, 2, 0), (65536, 2, 2, 0), (2, 65536, 9, 136),
         (640, 640, 1, 25), (640, 640, 1, 56))
DEGENERATE = ((1, 1, 9, 0), (1, 7, 9, 0), (7, 1, 9, 0), (2, 2, 9, 0), (5, 17, 9, 0))
TALLEST = (2, 65536, 9, 136)


def _id(k):
    return "%dx%dx%d@%d" % k


def _assert_plane_equal(img, ref, keys=KEYS, what=""):
    for k in keys:
        bad = bits(img[k]) != bits(ref[k])
        assert not bad.any(), (what, k, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())


def _box(ctx):
    ctx.upload_scene(scenes.make_scene_box())


def _params(W, H, spp, off=0, flags=FLAG, **kw):
    return dc.params(W, H, spp, spp_offset=off, flags=flags, **kw)


@pytest.mark.parametrize("key", WHOLE + DEGENERATE, ids=_id)
def test_whole_frames_bit_exact(gpu_ctx, oracle, key):
    """ipt_render_values' values and codes, ipt_render's plane and the drifted
    counter (the counting instance), each against the restatement."""
    W, H, spp, off = key
    _box(gpu_ctx)
    ov, _, _ = dc.oracle_samples(W, H, spp, off)
    codes = gc.codes(W, H, spp, off)
    p = _params(W, H, spp, off, FLAG | capi.IPT_FLAG_COUNTERS)
    gpu_ctx.reset_counters()
    gv, gcodes = gpu_ctx.render_values(p)
    assert np.array_equal(gcodes, codes), int((gcodes != codes).sum())
    assert np.array_equal(bits(gv), bits(ov)), int((bits(gv) != bits(ov)).sum())
    assert gpu_ctx.counters()["drifted"] == int((codes != 0x05).sum())
    if key in gc.HIST:
        assert dc.histogram(gcodes) == gc.HIST[key]
    img = dc.plane(W, H)
    gpu_ctx.reset_counters()
    gpu_ctx.render(p, img)
    _assert_plane_equal(img, gc.gui_plane(W, H, spp, off))
    assert gpu_ctx.counters()["drifted"] == int((codes != 0x05).sum())


def test_top_clamp_with_radiance(gpu_ctx, oracle):
    """The top clamp whose sample carries radiance (smallpt's room; the box
    scene's lower edge is dark): without the min() its pixel would lose it."""
    name, W, H, spp, off = gc.TOP_CLAMP_NONZERO
    desc = getattr(scenes, "make_scene_" + name)()
    ov, _ = ob.render_values(desc, _params(W, H, spp, off, 0))
    codes = gc.codes(W, H, spp, off)
    top, _ = gc.edge_masks(W, H, spp, off)
    assert top.sum() == 1 and (ov[top] > 0).all()
    gpu_ctx.upload_scene(desc)
    gv, gcodes = gpu_ctx.render_values(_params(W, H, spp, off))
    assert np.array_equal(gcodes, codes) and np.array_equal(bits(gv), bits(ov))
    img = dc.plane(W, H)
    gpu_ctx.render(_params(W, H, spp, off), img)
    _assert_plane_equal(img, gc.replay(ov, codes))


# ---- device buffers -----------------------------------------------------------
def _to_device(img, keys=KEYS):
    dev = torch.device("cuda", 0)
    return {k: torch.from_numpy(img[k].view(np.int32) if k == "counters" else img[k]).to(dev) for k in keys}


def _ptrs(t):
    return (t["pixels"].data_ptr(), t["counters"].data_ptr(), t["sums"].data_ptr() if "sums" in t else None,
            t["pixel_max"].data_ptr() if "pixel_max" in t else None)


def _to_host(t):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if k == "counters" else v.cpu().numpy()) for k, v in t.items()}


SUBSETS = (KEYS, ("pixels", "counters", "pixel_max"), ("pixels", "counters", "sums"), ("pixels", "counters"))


@pytest.mark.parametrize("key", [(60000, 3, 9, 0), TALLEST], ids=_id)
def test_render_device_and_async(gpu_ctx, oracle, key):
    """ipt_render_device, and two queued ipt_render_device_async calls (five
    passes, then four) against the one call's plane; with and without sums
    and pixel_max."""
    W, H, spp, off = key
    _box(gpu_ctx)
    ref = gc.gui_plane(W, H, spp, off)
    for keys in SUBSETS:
        t = _to_device(dc.plane(W, H), keys)
        gpu_ctx.render_device(_params(W, H, spp, off), *_ptrs(t))
        _assert_plane_equal(_to_host(t), ref, keys, what="render_device " + "+".join(keys))
    for keys in (KEYS, ("pixels", "counters")):
        t = _to_device(dc.plane(W, H), keys)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            gpu_ctx.render_device_async(_params(W, H, 5, off), *_ptrs(t), s.cuda_stream)
            gpu_ctx.render_device_async(_params(W, H, spp - 5, off + 5), *_ptrs(t), s.cuda_stream)
        s.synchronize()
        gpu_ctx.wait()
        _assert_plane_equal(_to_host(t), ref, keys, what="render_device_async " + "+".join(keys))


# ---- shards -------------------------------------------------------------------
def _render_shards(ctx, key, tile, n_shards, flags=FLAG):
    W, H, spp, off = key
    out = dc.plane(W, H)
    covered = np.zeros(H, np.int32)
    for s in range(n_shards):
        part = dc.plane(W, H)
        p = _params(W, H, spp, off, flags, tile_rows=tile, n_shards=n_shards, shard_id=s)
        owned, _ = capi.shard_plan(p)
        covered += owned
        ctx.render(p, part)
        mask = np.repeat(owned, W)
        for k in KEYS:
            assert not part[k][~mask].any(), f"shard {s} wrote outside its rows"
            out[k][mask] = part[k][mask]
    assert (covered == 1).all()
    return out


@pytest.mark.parametrize("tile,n_shards", [(1, 2), (1, 3), (16, 8)])
def test_sharded_bit_exact(gpu_ctx, oracle, tile, n_shards):
    """Passes 136..144 of the tallest frame, assembled: the bottom samples
    (source row H-1 into row 1) and 2690 dy = +1 drifts cross owners under
    one-row tiles; each shard traces the Gui plan's candidate rows."""
    _box(gpu_ctx)
    W, H, spp, off = TALLEST
    if tile == 1:
        _, yi, _ = gc.destinations(gc.codes(W, H, spp, off))
        _, bottom = gc.edge_masks(W, H, spp, off)
        yn = np.broadcast_to(gc.nominal_rows(H), yi.shape)
        assert (dc.shard_of(yi[bottom], tile, n_shards) != dc.shard_of(yn[bottom], tile, n_shards)).all()
    _assert_plane_equal(_render_shards(gpu_ctx, TALLEST, tile, n_shards), gc.gui_plane(W, H, spp, off))


# ---- preloaded plane ------------------------------------------------------------
def test_preloaded_plane_bit_exact(gpu_ctx, oracle):
    """The replay continues existing state (drift_cases.preload's kinds on the
    drifted destinations) under the Gui map, host and device buffers."""
    W, H, spp = 60000, 3, 9
    _box(gpu_ctx)
    ov, _, _ = dc.oracle_samples(W, H, spp)
    codes = gc.codes(W, H, spp)
    _, yi, xi = gc.destinations(codes)
    d = codes != 0x05
    pre, _ = dc.preload(W, H, spp, yi[d] * W + xi[d])
    ref = gc.replay(ov, codes, img=dc.copy_plane(pre))
    assert (bits(ref["pixels"]) != bits(pre["pixels"])).any()
    img = dc.copy_plane(pre)
    gpu_ctx.render(_params(W, H, spp), img)
    _assert_plane_equal(img, ref, what="ipt_render")
    for keys in (KEYS, ("pixels", "counters")):
        t = _to_device(pre, keys)
        gpu_ctx.render_device(_params(W, H, spp), *_ptrs(t))
        _assert_plane_equal(_to_host(t), ref, keys, what="ipt_render_device " + "+".join(keys))


# ---- without the flag -------------------------------------------------------------
def test_without_the_flag_nothing_changes(gpu_ctx, oracle):
    """A guard: the same calls without the flag, on a context that has just
    rendered the Gui plane of the same shape and shard plan, still give the
    oracle's GridRenderPlane."""
    _box(gpu_ctx)
    for key in ((60000, 3, 9, 0), TALLEST):
        W, H, spp, off = key
        ov, oc, _ = dc.oracle_samples(W, H, spp, off)
        ref = dc.oracle_plane(W, H, spp, off)
        gpu_ctx.render(_params(W, H, spp, off), dc.plane(W, H))
        gv, gcodes = gpu_ctx.render_values(_params(W, H, spp, off, 0))
        assert np.array_equal(gcodes, oc) and np.array_equal(bits(gv), bits(ov))
        img = dc.plane(W, H)
        gpu_ctx.render(_params(W, H, spp, off, 0), img)
        _assert_plane_equal(img, ref, what="ipt_render")
        t = _to_device(dc.plane(W, H))
        gpu_ctx.render_device(_params(W, H, spp, off, 0), *_ptrs(t))
        _assert_plane_equal(_to_host(t), ref, what="ipt_render_device")
    _render_shards(gpu_ctx, TALLEST, 16, 8)
    _assert_plane_equal(_render_shards(gpu_ctx, TALLEST, 16, 8, flags=0), dc.oracle_plane(*TALLEST), what="shards")


# ---- the reference program's loop ---------------------------------------------------
@pytest.mark.parametrize("cutoff", [0.0, 1.01])
def test_render_then_display_on_one_stream(gpu_ctx, oracle, cutoff):
    """render(GUI_PLANE) into device buffers, then ipt_display_device on the
    same stream with no host wait between: gray8 is the CPU display of the
    restated plane (Gui::updateDisplay with the glare, Gui::save without)."""
    W, H, spp = 64, 64, 4
    _box(gpu_ctx)
    ref = gc.gui_plane(W, H, spp)
    assert ref["pixels"].max() > 0
    t = _to_device(dc.plane(W, H))
    g8 = torch.zeros(W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gpu_ctx.render_device_async(_params(W, H, spp), *_ptrs(t), s.cuda_stream)
        gpu_ctx.display_device(capi.make_display_params(W, H, cutoff), t["pixels"].data_ptr(), g8.data_ptr(),
                               stream=s.cuda_stream)
    s.synchronize()
    gpu_ctx.wait()
    _assert_plane_equal(_to_host(t), ref)
    assert np.array_equal(g8.cpu().numpy(), dr.display_ref(ref["pixels"], W, H, cutoff)["gray8"])


# ---- host layer ---------------------------------------------------------------------
@pytest.mark.parametrize("devices", ["0", "0,0,0"])
def test_cli_gui_plane(oracle, tmp_path, devices):
    """ipt_render --gui-plane (GuiRenderPlane through GpuRenderer /
    MultiGpuRenderer, two progressive batches) with --gpu-display, --pfm and
    --counts: the restated plane, and its display as the PNG's bytes."""
    from test_display_cpu import read_png_gray8

    exe = ge.build_host()
    W, H, spp = 40, 24, 2
    r = subprocess.run([str(exe), "--scene", "box", "--gui-plane", "--gpu-display", "--width", str(W), "--height",
                        str(H), "--spp", str(spp), "--passes", "2", "--n-rays", str(dc.N_RAYS), "--depth",
                        str(dc.DEPTH_MAX), "--devices", devices, "--tile-rows", "5", "--out", str(tmp_path / "o.png"),
                        "--pfm", str(tmp_path / "o.pfm"), "--counts", str(tmp_path / "o.u32")],
                       check=True, capture_output=True, text=True, timeout=120)
    assert '"plane": "gui"' in r.stdout
    ref = gc.gui_plane(W, H, 2 * spp)
    raw = (tmp_path / "o.pfm").read_bytes()
    px = np.frombuffer(raw[-4 * W * H:], np.float32).reshape(H, W)[::-1].reshape(-1)  # PFM rows: bottom to top
    assert np.array_equal(bits(px), bits(ref["pixels"]))
    assert np.array_equal(np.fromfile(tmp_path / "o.u32", np.uint32), ref["counters"])
    assert np.array_equal(read_png_gray8(tmp_path / "o.png").reshape(-1), dr.display_ref(ref["pixels"], W, H)["gray8"])
