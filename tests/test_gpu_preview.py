"""The preview estimator on the GPU (IPT_FLAG_PREVIEW, ipt_preview_values):
preview_kernel bit for bit against the reference restatement
(tests/native/preview_ref.cpp, pinned without a GPU by tests/test_preview_cpu.py)
on every geometry kind, the linear / BVH / grid sphere paths and every light
mode, then the flag through every render call, plane, shard plan, queued mix
with the full estimator, the display chain and the C++ CLI. Frames are 37 x 23
or smaller, 2 passes from spp_offset 3, unless a test says otherwise."""
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import display_ref as dr
import drift_cases as dc
import gui_cases as gc
import oracle_binding as ob
import preview_cases as pc
import preview_ref
from ipt_amd import capi, scenes

pytestmark = pytest.mark.gpu

bits = dc.bits
KEYS = tuple(k for k, _ in dc.PLANE_KEYS)
PREVIEW, GUI, COUNT = capi.IPT_FLAG_PREVIEW, capi.IPT_FLAG_GUI_PLANE, capi.IPT_FLAG_COUNTERS


def _assert_plane_equal(img, ref, keys=KEYS, what=""):
    for k in keys:
        bad = bits(img[k]) != bits(ref[k])
        assert not bad.any(), (what, k, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())


def _to_device(img, keys=KEYS):
    dev = torch.device("cuda", 0)
    return {k: torch.from_numpy(img[k].view(np.int32) if k == "counters" else img[k]).to(dev) for k in keys}


def _ptrs(t):
    return (t["pixels"].data_ptr(), t["counters"].data_ptr(), t["sums"].data_ptr() if "sums" in t else None,
            t["pixel_max"].data_ptr() if "pixel_max" in t else None)


def _to_host(t):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if k == "counters" else v.cpu().numpy()) for k, v in t.items()}


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_parity(gpu_ctx, oracle, name):
    """values, codes and kinds bit-identical, hits numerically equal, counters
    equal; the flag is not set (ipt_preview_values implies the preview)."""
    rv, rc, rk, rh, rcnt = pc.reference(name)
    pc.check_branches(name, rk)
    assert not np.isnan(rh).any()
    gpu_ctx.upload_scene(pc.scene(name))
    gpu_ctx.reset_counters()
    gv, gcodes, gk, gh = gpu_ctx.preview_values(pc.params(name, COUNT))
    cnt = gpu_ctx.counters()
    assert np.array_equal(gcodes, rc), int((gcodes != rc).sum())
    assert np.array_equal(gk, rk), (int((gk != rk).sum()), np.argwhere(gk != rk)[:4].tolist())
    assert np.array_equal(bits(gv), bits(rv)), (int((bits(gv) != bits(rv)).sum()), np.argwhere(gv != rv)[:4].tolist())
    assert np.array_equal(gh, rh), np.argwhere(gh != rh)[:4].tolist()  # (+-0 alike)
    for k in preview_ref.EVENT_COUNTERS:
        assert cnt[k] == rcnt[k], (k, cnt[k], rcnt[k])
    for k in preview_ref.ZERO_COUNTERS:
        assert cnt[k] == 0, (k, cnt[k])
    # what the kernel ran: every light is tested by the scan, fewer by the light BVH
    n_lights = len(pc.scene(name)["lights"])
    assert 0 < cnt["light_tests"] <= rcnt["light_traces"]
    # (built for more than 16 AreaLights; where it is not, the scan runs)
    if n_lights <= 16:
        assert cnt["light_nodes"] == 0
    assert cnt["light_nodes"] > 0 or cnt["light_tests"] == rcnt["light_traces"]
    # the outputs are optional, and the plain instance gives the same samples
    v2, c2, k2, h2 = gpu_ctx.preview_values(pc.params(name), kinds=False, hits=False)
    assert k2 is None and h2 is None and np.array_equal(bits(v2), bits(rv)) and np.array_equal(c2, rc)
    assert gpu_ctx.counters() == cnt  # (no IPT_FLAG_COUNTERS: nothing is counted)


def test_render_values_with_and_without_the_flag(gpu_ctx, oracle):
    rv, rc, _, _, _ = pc.reference("box/up")
    desc = pc.scene("box/up")
    gpu_ctx.upload_scene(desc)
    gv, gcodes = gpu_ctx.render_values(pc.params("box/up", PREVIEW))
    assert np.array_equal(bits(gv), bits(rv)) and np.array_equal(gcodes, rc)
    # n_rays and depth_max are not read
    gv, gcodes = gpu_ctx.render_values(pc.params("box/up", PREVIEW, n_rays=-5, depth_max=99))
    assert np.array_equal(bits(gv), bits(rv)) and np.array_equal(gcodes, rc)
    pv = gpu_ctx.preview_values(pc.params("box/up", n_rays=-5, depth_max=99))
    assert np.array_equal(bits(pv[0]), bits(rv))
    # without the flag: the full estimator, unchanged
    p = pc.params("box/up", n_rays=dc.N_RAYS, depth_max=dc.DEPTH_MAX)
    ov, oc = ob.render_values(desc, p)
    gv, gcodes = gpu_ctx.render_values(p)
    assert np.array_equal(bits(gv), bits(ov)) and np.array_equal(gcodes, oc)
    assert not np.array_equal(bits(ov), bits(rv))
    with pytest.raises(capi.IptError) as e:
        gpu_ctx.render_values(pc.params("box/up", n_rays=-5))
    assert e.value.code == capi.IPT_E_UNSUPPORTED


@pytest.mark.parametrize("flags", [0, GUI], ids=["grid", "gui"])
def test_planes_nine_passes(gpu_ctx, oracle, flags):
    """ipt_render and ipt_render_device at 9 passes (the replay's unrolled
    eight plus one), both planes; then two calls with increasing spp_offset."""
    name, spp = "box/up", 9
    rv, rc, _, _, _ = pc.reference(name, flags, spp)
    ref = gc.replay(rv, rc) if flags & GUI else ob.accumulate(rv, rc)
    assert ref["pixels"].max() == 1.0
    gpu_ctx.upload_scene(pc.scene(name))
    img = dc.plane(pc.W, pc.H)
    gpu_ctx.render(pc.params(name, PREVIEW | flags, spp), img)
    _assert_plane_equal(img, ref, what="ipt_render")
    t = _to_device(dc.plane(pc.W, pc.H))
    gpu_ctx.render_device(pc.params(name, PREVIEW | flags, spp), *_ptrs(t))
    _assert_plane_equal(_to_host(t), ref, what="ipt_render_device")
    img = dc.plane(pc.W, pc.H)
    gpu_ctx.render(pc.params(name, PREVIEW | flags, 5), img)
    gpu_ctx.render(pc.params(name, PREVIEW | flags, spp - 5, pc.OFFSET + 5), img)
    _assert_plane_equal(img, ref, what="two calls")


@pytest.mark.parametrize("tile,n_shards", [(4, 3), (1, 2)])
def test_sharded(gpu_ctx, oracle, tile, n_shards):
    name, spp = "box/up", 9
    rv, rc, _, _, _ = pc.reference(name, 0, spp)
    ref = ob.accumulate(rv, rc)
    gpu_ctx.upload_scene(pc.scene(name))
    out = dc.plane(pc.W, pc.H)
    covered = np.zeros(pc.H, np.int32)
    for s in range(n_shards):
        part = dc.plane(pc.W, pc.H)
        p = pc.params(name, PREVIEW, spp, tile_rows=tile, n_shards=n_shards, shard_id=s)
        owned, _ = capi.shard_plan(p)
        covered += owned
        gpu_ctx.render(p, part)
        mask = np.repeat(owned, pc.W)
        for k in KEYS:
            assert not part[k][~mask].any(), f"shard {s} wrote outside its rows"
            out[k][mask] = part[k][mask]
    assert (covered == 1).all()
    _assert_plane_equal(out, ref)


def _mixed_calls(name):
    """full -> preview -> full, two passes each, and the plane they leave: the
    oracle's samples of the full calls and the reference preview's of the
    middle one, replayed on the host in call order."""
    full = dict(n_rays=dc.N_RAYS, depth_max=dc.DEPTH_MAX)
    calls = [pc.params(name, 0, 2, 0, **full), pc.params(name, PREVIEW, 2, 2), pc.params(name, 0, 2, 4, **full)]
    rv, rc, _, _, _ = pc.reference(name, 0, 2, 2)
    assert (rv == 1.0).any()
    img = None
    for p in calls:
        v, c = (rv, rc) if p.flags & PREVIEW else ob.render_values(pc.scene(name), p)
        img = ob.accumulate(v, c, img)
    return calls, img


def _queue(ctx, calls):
    t = _to_device(dc.plane(pc.W, pc.H))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for p in calls:
            ctx.render_device_async(p, *_ptrs(t), s.cuda_stream)
    s.synchronize()
    ctx.wait()
    return _to_host(t)


def test_mixed_queued_passes(gpu_ctx, oracle):
    """full pass -> preview pass -> full pass queued into one plane on one
    stream equal the same three synchronous calls, bit for bit, and the host
    replay of their samples."""
    name = "box/up"
    gpu_ctx.upload_scene(pc.scene(name))
    calls, ref = _mixed_calls(name)
    sync = _to_device(dc.plane(pc.W, pc.H))
    for p in calls:
        gpu_ctx.render_device(p, *_ptrs(sync))
    sync = _to_host(sync)
    _assert_plane_equal(_queue(gpu_ctx, calls), sync, what="queued vs synchronous")
    _assert_plane_equal(sync, ref, what="synchronous vs host replay")


@pytest.mark.parametrize("gate", ["pool", "IPT_NO_TAIL_OVERLAP"])
def test_chunked_launches(oracle, monkeypatch, gate):
    """One pass per launch (IPT_TEST_CHUNK_UNITS): preview launches alternate
    the work slots, ungated, and a full launch after a preview one gates on
    the slot's last full launch (its drained pool, or its end event)."""
    monkeypatch.setenv("IPT_TEST_CHUNK_UNITS", "1")
    if gate != "pool":
        monkeypatch.setenv(gate, "1")
    ctx = capi.Context(0)
    try:
        name, spp = "box/up", 9
        rv, rc, rk, rh, _ = pc.reference(name, 0, spp)
        ctx.upload_scene(pc.scene(name))
        gv, gcodes, gk, gh = ctx.preview_values(pc.params(name, 0, spp))
        assert np.array_equal(bits(gv), bits(rv)) and np.array_equal(gcodes, rc)
        assert np.array_equal(gk, rk) and np.array_equal(gh, rh)
        img = dc.plane(pc.W, pc.H)
        ctx.render(pc.params(name, PREVIEW, spp), img)
        _assert_plane_equal(img, ob.accumulate(rv, rc), what="ipt_render")
        calls, ref = _mixed_calls(name)
        _assert_plane_equal(_queue(ctx, calls), ref, what="queued mix")
    finally:
        ctx.close()


@pytest.mark.parametrize("cutoff", [0.0, 1.01])
def test_preview_then_display_on_one_stream(gpu_ctx, oracle, cutoff):
    """The interactive frame: render(PREVIEW | GUI_PLANE, 1 spp) into device
    buffers, then ipt_display_device on the same stream with no host wait."""
    name = "box/up"
    rv, rc, _, _, _ = pc.reference(name, GUI, 1)
    ref = gc.replay(rv, rc)
    gpu_ctx.upload_scene(pc.scene(name))
    t = _to_device(dc.plane(pc.W, pc.H))
    g8 = torch.zeros(pc.W * pc.H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gpu_ctx.render_device_async(pc.params(name, PREVIEW | GUI, 1), *_ptrs(t), s.cuda_stream)
        gpu_ctx.display_device(capi.make_display_params(pc.W, pc.H, cutoff), t["pixels"].data_ptr(), g8.data_ptr(),
                               stream=s.cuda_stream)
    s.synchronize()
    gpu_ctx.wait()
    _assert_plane_equal(_to_host(t), ref)
    assert np.array_equal(g8.cpu().numpy(), dr.display_ref(ref["pixels"], pc.W, pc.H, cutoff)["gray8"])


def test_cli_preview(oracle, tmp_path):
    """ipt_render --preview --gui-plane: the reference plane and its display."""
    from test_display_cpu import read_png_gray8

    exe = ge.build_host()
    W, H, spp = 40, 24, 2
    r = subprocess.run([str(exe), "--scene", "box", "--preview", "--gui-plane", "--gpu-display", "--width", str(W),
                        "--height", str(H), "--spp", str(spp), "--devices", "0,0", "--tile-rows", "5",
                        "--out", str(tmp_path / "o.png"), "--pfm", str(tmp_path / "o.pfm")],
                       check=True, capture_output=True, text=True, timeout=120)
    assert '"plane": "gui"' in r.stdout
    rv, rc, rk, _, _ = preview_ref.render(scenes.make_scene_box(), capi.make_params(W, H, spp, flags=GUI))
    assert ((rk & 3) == preview_ref.OUTCOME_SURFACE).any()
    ref = gc.replay(rv, rc)
    raw = (tmp_path / "o.pfm").read_bytes()
    px = np.frombuffer(raw[-4 * W * H:], np.float32).reshape(H, W)[::-1].reshape(-1)  # PFM rows: bottom to top
    assert np.array_equal(bits(px), bits(ref["pixels"]))
    assert np.array_equal(read_png_gray8(tmp_path / "o.png").reshape(-1), dr.display_ref(ref["pixels"], W, H)["gray8"])
