"""Temporal reprojection on the device against tests/reproject_cases.py's
numpy restatement, bit for bit on the three planes and the stats: rendered
planes and guides at two cameras on both row maps, every camera move,
synthetic guides, poisoned planes, the history cap and the normal bound, the
argument rules, the host form, and the loop render -> guides -> new camera ->
guides -> reproject -> adapt -> masked render -> denoise -> display queued with
no host wait, stage by stage. tests/test_reproject_cpu.py pins, without a
GPU, that the restatement is the resampling meant. The definition's exact
comparisons (pixel boundaries, thresholds, the cap, denormals, misaligned
planes) are tests/test_gpu_reproject_edges.py's."""
import numpy as np
import pytest
import torch

import adaptive_cases as ac
import denoise_cases as dn
import display_ref
import drift_cases as dc
import gui_cases as gc
import reproject_cases as rc
from ipt_amd import capi, scenes
from reproject_gpu import DEV, STATS_JUNK, _check, _equal, _h, _reproject, _t

pytestmark = pytest.mark.gpu

F = np.float32


# ---- rendered planes -------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", rc.FRAMES + rc.TINY_FRAMES + (rc.BLOCK_FRAME,), ids=lambda f: "%dx%d" % f)
def test_rendered_frames(gpu_ctx, oracle, frame, plane):
    """131 x 67 and 300 x 75 take more than one workgroup and are no multiple
    of the block; on the tiny frames most taps leave the frame."""
    W, H = frame
    case = rc.rendered_case("box", "shift", W, H, plane)
    ref = _check(gpu_ctx, case, W, H, plane, (frame, plane))
    if W * H > 100:
        assert ref[3][0] > W * H // 4 and ref[3][1] > 0 and ref[3][2] > 0


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("scene_move", [("box", m) for m in rc.BOX_MOVES] + [("square", m) for m in rc.SQUARE_MOVES],
                         ids=lambda sm: "%s-%s" % sm)
def test_cameras(gpu_ctx, oracle, scene_move, plane):
    """The same camera, a shift, a turn, a camera with the hits behind it, a
    shift that leaves part of the frame without history; the square scene's
    camera direction has length 2."""
    scene, move = scene_move
    W, H = 64, 48
    case = rc.rendered_case(scene, move, W, H, plane)
    ref = _check(gpu_ctx, case, W, H, plane, (scene, move, plane))
    if move == "same":
        assert ref[3][1] == 0 and ref[3][0] > 0
    if move == "behind":
        assert 10 * ref[3][0] < ref[3][1] and ref[3][1] > W * H // 2
    if move == "far":
        assert ref[3][0] > 100 and ref[3][1] > ref[3][0]


@pytest.mark.parametrize("normal_min", (-1.0, 0.9, float("inf")))
@pytest.mark.parametrize("max_count", (2, 16, 1 << 24))
def test_cap_and_normal_bound(gpu_ctx, oracle, max_count, normal_min):
    """On the rendered box planes and on the poisoned crease planes, whose
    counters reach 2^24 + 1, 2^31 and 2^32 - 1."""
    W, H = 37, 23
    ref = _check(gpu_ctx, rc.rendered_case("box", "shift", W, H), W, H, max_count=max_count, normal_min=normal_min)
    assert (ref[3][0] == 0) == (normal_min == float("inf"))
    assert ref[1].max() <= max_count
    W, H = 67, 35
    _check(gpu_ctx, rc.poisoned(rc.synthetic_case("crease", W, H), W, H), W, H, max_count=max_count,
           normal_min=normal_min)


# ---- synthetic guides and poison -------------------------------------------------------------
@pytest.mark.parametrize("poison", (False, True))
@pytest.mark.parametrize("guides", ("crease", "step"))
def test_synthetic(gpu_ctx, guides, poison):
    W, H = 67, 35
    case = rc.synthetic_case(guides, W, H)
    if poison:
        case = rc.poisoned(case, W, H)
    for plane in ac.PLANES:
        ref = _check(gpu_ctx, case, W, H, plane, (guides, poison, plane))
        assert ref[3][0] > W * H // 2
        if poison:
            assert np.isfinite(ref[0]).all() and np.isfinite(ref[2]).all() and ref[3][2] > 0


@pytest.mark.parametrize("plane", ac.PLANES)
def test_poisoned_rendered_planes(gpu_ctx, oracle, plane):
    """NaN and infinite pixels and m2, counters 0, 1, 2, 2^24 + 1, 2^31 and
    2^32 - 1, kinds 0, 2, 3, 0x81, 0xfd, 0xff and guide positions and normals
    that are no numbers, in both guide planes."""
    W, H = 131, 67
    clean = rc.rendered_case("box", "turn", W, H, plane)
    case = rc.poisoned(clean, W, H)
    ref = _check(gpu_ctx, case, W, H, plane, plane)
    assert rc.differ(rc.reproject(*clean[:5], W, H, clean[5], plane), ref) != (0, 0, 0)


def test_stats_may_be_null(gpu_ctx, oracle):
    W, H = 37, 23
    case = rc.rendered_case("box", "shift", W, H)
    got = _reproject(gpu_ctx, case, W, H, stats=False)
    assert got[3] is None
    _equal(got, rc.reproject(*case[:5], W, H, case[5]))


# ---- the loop in stream order ----------------------------------------------------------------
ADAPT = dict(min_count=4, rel_tol=0.25, abs_tol=1e-3)


def _restated_chain(W, H, plane, move):
    """Every stage of the loop from the restatements."""
    gui = plane == rc.GUI
    case = rc.rendered_case("box", move, W, H, plane)
    rep = rc.reproject(*case[:5], W, H, case[5], plane)
    mask, astats = ac.adapt(rep[0], rep[1], rep[2], W, H, gui=gui, **ADAPT)
    import oracle_binding
    p = capi.make_params(W, H, rc.RENDER_SPP, spp_offset=rc.RENDER_SPP, **rc.RENDER)
    vals, codes = (np.asarray(a) for a in oracle_binding.render_values(scenes.make_scene_box(), p))
    if gui:
        codes = gc.codes(W, H, rc.RENDER_SPP, rc.RENDER_SPP)
    img = dc.plane(W, H)
    img["pixels"][:], img["counters"][:] = rep[0], rep[1]
    m2 = rep[2].copy()
    ac.replay(vals, codes, mask.reshape(H, W), plane, img=img, m2=m2)
    out, _ = dn.denoise(img["pixels"], img["counters"], m2, case[4], W, H)
    return dict(prev=case, rep=rep, mask=mask, astats=astats, img=img, m2=m2, out=out,
                gray8=display_ref.display_ref(out, W, H)["gray8"])


def _chain(ctx, W, H, plane, move, streams):
    """The loop queued with no host wait in the test: stage k runs on
    streams[k % len(streams)]. Between two post-process calls (reproject ->
    adapt, denoise -> display) the library orders the streams itself; where a
    render or a guide pass is the producer or the consumer the next stream
    waits for the previous one on the device."""
    n = W * H
    flags = ac.FLAG[plane]
    prev = {k: _t(v) for k, v in dc.plane(W, H).items()}
    cur = {k: _t(v) for k, v in dc.plane(W, H).items()}
    pm2, cm2 = torch.zeros(n, dtype=torch.float32, device=DEV), torch.zeros(n, dtype=torch.float32, device=DEV)
    pg, cg = (torch.zeros(n * 32, dtype=torch.uint8, device=DEV) for _ in range(2))
    rstats, astats = (torch.full((4,), STATS_JUNK, dtype=torch.int32, device=DEV) for _ in range(2))
    mask = torch.full((n,), 0x77, dtype=torch.uint8, device=DEV)
    out = torch.zeros(n, dtype=torch.float32, device=DEV)
    g8 = torch.zeros(n, dtype=torch.uint8, device=DEV)
    snap = {k: torch.zeros_like(v) for k, v in (("px", cur["pixels"]), ("cn", cur["counters"]), ("m2", cm2))}
    prev_cam = rc.box_prev_camera(move)
    ctx.upload_scene(rc.scene_desc("box", move))
    torch.cuda.synchronize()
    k = [0]
    last = [None]

    def stream(after_render=False):
        s = streams[k[0] % len(streams)]
        k[0] += 1
        if after_render and last[0] is not None and last[0] is not s:
            s.wait_stream(last[0])
        last[0] = s
        return s

    p = capi.make_params(W, H, rc.RENDER_SPP, flags=flags, **rc.RENDER)
    g1 = capi.make_params(W, H, 1, flags=flags)
    s = stream()
    ctx.render_masked_device_async(p, prev["pixels"].data_ptr(), prev["counters"].data_ptr(), prev["sums"].data_ptr(),
                                   prev["pixel_max"].data_ptr(), mask_ptr=None, m2_ptr=pm2.data_ptr(),
                                   stream=s.cuda_stream)
    s = stream(after_render=True)
    ctx.guides_device(g1, pg.data_ptr(), s.cuda_stream)
    ctx.upload_scene(scenes.make_scene_box())  # the new camera (the library waits for what it has queued)
    s = stream()
    ctx.guides_device(g1, cg.data_ptr(), s.cuda_stream)
    s = stream(after_render=True)  # (the guide pass is queued as a render is)
    ctx.reproject_device(capi.make_reproject_params(W, H, prev_cam, flags=flags), prev["pixels"].data_ptr(),
                         prev["counters"].data_ptr(), pm2.data_ptr(), pg.data_ptr(), cg.data_ptr(),
                         cur["pixels"].data_ptr(), cur["counters"].data_ptr(), cm2.data_ptr(), rstats.data_ptr(),
                         s.cuda_stream)
    s = stream()  # post-process call after post-process call: the library's own event orders the streams
    ctx.adapt_device(capi.make_adapt_params(W, H, flags=flags, **ADAPT), cur["pixels"].data_ptr(),
                     cur["counters"].data_ptr(), cm2.data_ptr(), mask.data_ptr(), astats.data_ptr(), s.cuda_stream)
    with torch.cuda.stream(s):  # (the reprojected planes, before the render continues them)
        snap["px"].copy_(cur["pixels"]), snap["cn"].copy_(cur["counters"]), snap["m2"].copy_(cm2)
    s = stream(after_render=True)  # (behind the copies too)
    p2 = capi.make_params(W, H, rc.RENDER_SPP, spp_offset=rc.RENDER_SPP, flags=flags, **rc.RENDER)
    ctx.render_masked_device_async(p2, cur["pixels"].data_ptr(), cur["counters"].data_ptr(), cur["sums"].data_ptr(),
                                   cur["pixel_max"].data_ptr(), mask_ptr=mask.data_ptr(), m2_ptr=cm2.data_ptr(),
                                   stream=s.cuda_stream)
    s = stream(after_render=True)
    ctx.denoise_device(capi.make_denoise_params(W, H), cur["pixels"].data_ptr(), cur["counters"].data_ptr(),
                       cm2.data_ptr(), cg.data_ptr(), out.data_ptr(), None, s.cuda_stream)
    s = stream()
    ctx.display_device(capi.make_display_params(W, H), out.data_ptr(), g8.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    ctx.wait()
    torch.cuda.synchronize()
    return dict(prev=(_h(prev["pixels"]), _h(prev["counters"]), _h(pm2)),
                pg=pg.cpu().numpy().view(capi.GuideRecord), cg=cg.cpu().numpy().view(capi.GuideRecord),
                rep=(_h(snap["px"]), _h(snap["cn"]), _h(snap["m2"]), _h(rstats)), mask=mask.cpu().numpy(),
                astats=_h(astats), img=(_h(cur["pixels"]), _h(cur["counters"]), _h(cm2)), out=_h(out),
                gray8=g8.cpu().numpy())


@pytest.mark.parametrize("plane", ac.PLANES)
def test_loop_in_stream_order(oracle, plane):
    """One stream, then two streams taking the stages in turn: every stage
    equals the restated chain. The masked render continues the reprojected
    mean, counter and m2 as it continues any preloaded plane."""
    W, H, move = 64, 48, "shift"
    ref = _restated_chain(W, H, plane, move)
    assert 0 < ref["astats"][0] < ref["rep"][3][0] + ref["rep"][3][1] and ref["rep"][3][1] > 0
    ctx = capi.Context(0)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for streams in ((s1,), (s1, s2)):
            got = _chain(ctx, W, H, plane, move, streams)
            what = (plane, len(streams))
            for k, name in enumerate(("pixels", "counters", "m2")):
                assert np.array_equal(dc.bits(got["prev"][k]), dc.bits(ref["prev"][k])), (what, "previous", name)
            assert np.array_equal(got["pg"].view(np.uint8), np.ascontiguousarray(ref["prev"][3]).view(np.uint8).reshape(-1))
            assert np.array_equal(got["cg"].view(np.uint8), np.ascontiguousarray(ref["prev"][4]).view(np.uint8).reshape(-1))
            _equal(got["rep"], ref["rep"], (what, "reproject"))
            assert np.array_equal(got["mask"], ref["mask"]) and got["astats"].tolist() == ref["astats"].tolist()
            assert np.array_equal(dc.bits(got["img"][0]), dc.bits(ref["img"]["pixels"])), (what, "continued pixels")
            assert np.array_equal(got["img"][1], ref["img"]["counters"]), (what, "continued counters")
            assert np.array_equal(dc.bits(got["img"][2]), dc.bits(ref["m2"])), (what, "continued m2")
            assert dn.same(got["out"], ref["out"]).all(), (what, "denoise")
            assert np.array_equal(got["gray8"], ref["gray8"]), (what, "display")
    finally:
        ctx.close()


# ---- errors ----------------------------------------------------------------------------------
def test_errors_leave_the_outputs(gpu_ctx, oracle):
    W, H = 13, 11
    n = W * H
    case = rc.rendered_case("box", "shift", W, H)
    buf = torch.full((n * 24 + 4,), 3.5, dtype=torch.float32, device=DEV)  # one allocation: overlaps are views of it
    base = buf.data_ptr()
    # planes 0..2, guides at 3 and 11 (8 planes' worth each), outputs at 19..21, stats behind them
    px, cn, mm, pg, cg, opx, ocn, om2, st = (base + 4 * n * k for k in (0, 1, 2, 3, 11, 19, 20, 21, 22))
    buf[0:n] = _t(case[0])
    buf[n:2 * n] = _t(case[1]).view(torch.float32)
    before = buf.cpu().numpy().copy()
    good = (px, cn, mm, pg, cg, opx, ocn, om2, st)

    def call(code, ptrs=good, w=W, h=H, flags=0, **kw):
        rp = capi.make_reproject_params(w, h, case[5], flags=flags, **kw)
        with pytest.raises(capi.IptError) as e:
            gpu_ctx.reproject_device(rp, *ptrs)
        assert e.value.code == code, (kw, ptrs)

    for kw in (dict(sigma_z=0.0), dict(sigma_z=-1.0), dict(sigma_z=float("nan")), dict(normal_min=float("nan")),
               dict(max_count=0), dict(max_count=1), dict(max_count=(1 << 24) + 1), dict(max_count=0xffffffff)):
        call(capi.IPT_E_INVALID, **kw)
    call(capi.IPT_E_INVALID, w=0)
    call(capi.IPT_E_INVALID, h=-1)
    call(capi.IPT_E_UNSUPPORTED, w=65536, h=32769)
    for flags in (capi.IPT_FLAG_COUNTERS, capi.IPT_FLAG_PREVIEW, capi.IPT_FLAG_COMPACT,
                  capi.IPT_FLAG_GUI_PLANE | capi.IPT_FLAG_PREVIEW, 1 << 31):
        call(capi.IPT_E_UNSUPPORTED, flags=flags)
    for k in range(8):  # each mandatory pointer NULL
        ptrs = list(good)
        ptrs[k] = None
        call(capi.IPT_E_INVALID, tuple(ptrs))
    last = 4 * (n - 1)
    ins = ((px, 4 * n), (cn, 4 * n), (mm, 4 * n), (pg, 32 * n), (cg, 32 * n))
    for o in range(5, 9):  # every output against every input, from the input's first and from its last dword
        for ip, ibytes in ins:
            for at in (ip, ip + ibytes - 4):
                ptrs = list(good)
                ptrs[o] = at
                call(capi.IPT_E_INVALID, tuple(ptrs))
    for a, b in ((5, 6), (5, 7), (6, 7)):  # the outputs against each other, whole and by one dword
        for shift in (0, last):
            ptrs = list(good)
            ptrs[b] = good[a] + shift
            call(capi.IPT_E_INVALID, tuple(ptrs))
    for o in (5, 6, 7):  # the stats inside an output plane
        ptrs = list(good)
        ptrs[8] = good[o] + last
        call(capi.IPT_E_INVALID, tuple(ptrs))
    gpu_ctx.wait()
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), before.view(np.uint32))
    # adjacent buffers are no overlap; the values that bound the ranges are accepted
    for kw in (dict(max_count=2), dict(max_count=1 << 24), dict(normal_min=float("inf")), dict(normal_min=-float("inf")),
               dict(sigma_z=float("inf"))):
        gpu_ctx.reproject_device(capi.make_reproject_params(W, H, case[5], **kw), *good)
    gpu_ctx.wait()
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert np.array_equal(after[:19 * n].view(np.uint32), before[:19 * n].view(np.uint32))
    assert np.array_equal(after[22 * n + 4:].view(np.uint32), before[22 * n + 4:].view(np.uint32))


# ---- host form -------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ac.PLANES)
def test_host_form_equals_device_form(gpu_ctx, oracle, plane):
    W, H = 64, 48
    case = rc.rendered_case("box", "turn", W, H, plane)
    rp = capi.make_reproject_params(W, H, case[5], flags=ac.FLAG[plane])
    px, cn, m2, st = gpu_ctx.reproject(rp, *case[:5])
    ref = rc.reproject(*case[:5], W, H, case[5], plane)
    _equal((px, cn, m2, np.array([st["reused"], st["disoccluded"], st["not_surface"], 0], np.uint32)), ref, plane)
    dev = _reproject(gpu_ctx, case, W, H, plane)
    assert np.array_equal(dc.bits(px), dc.bits(dev[0])) and np.array_equal(cn, dev[1])
    with pytest.raises(capi.IptError) as e:
        gpu_ctx.reproject(capi.make_reproject_params(W, H, case[5], max_count=1), *case[:5])
    assert e.value.code == capi.IPT_E_INVALID
