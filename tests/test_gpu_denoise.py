"""The denoiser on the device against tests/denoise_cases.py's numpy
restatement, bit for bit: the guide plane (ipt_guides_device), the filter
(ipt_denoise_device, ipt_denoise) in both tap-loop forms, its participation
edges, the chain render -> guides -> denoise -> display in stream order, and
the argument rules. tests/test_denoise_cpu.py pins, without a GPU, that the
restatement is the filter meant, on which frames a tap leaves its lattice tile
and which planes leave the windows of the range-free division and root."""
import functools

import numpy as np
import pytest
import torch

import adaptive_cases as ac
import denoise_cases as dn
import drift_cases as dc
import preview_cases as pc
from ipt_amd import capi, scenes

pytestmark = pytest.mark.gpu

F = np.float32
DEV = torch.device("cuda", 0)
FORMS = (None, "direct", "tiled")  # IPT_DENOISE_FORM: the library's choice, then each form forced


def _t(a):
    a = np.array(a, order="C")  # (a writable copy: the cases' arrays are read-only)
    if a.dtype == capi.GuideRecord:
        a = a.reshape(-1).view(np.uint8)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def _h(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _same(got, ref, what=""):
    bad = ~dn.same(got, ref)
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())


def _bits(got, ref, what=""):
    bad = dc.bits(np.asarray(got, F)) != dc.bits(np.asarray(ref, F))
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())


def _guides(ctx, p, stream=None):
    g = torch.full((p.width * p.height * 32,), 0xa5, dtype=torch.uint8, device=DEV)
    ctx.guides_device(p, g.data_ptr(), stream)
    ctx.wait()
    torch.cuda.synchronize()
    return g.cpu().numpy().view(capi.GuideRecord).reshape(p.height, p.width)


def _guides_equal(got, ref, what=""):
    a, b = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(ref).view(np.uint8)
    assert np.array_equal(a, b), (what, np.flatnonzero((a != b).reshape(-1, 32).any(1))[:8].tolist())


def _denoise(ctx, dp, px, cn, m2, g, var=True, form=None, monkeypatch=None):
    """ipt_denoise_device on device copies; (out, var or None) on the host."""
    n = dp.width * dp.height
    tp, tc, tm, tg = _t(np.asarray(px, F)), _t(np.asarray(cn, np.uint32)), _t(np.asarray(m2, F)), _t(g)
    out = torch.full((n,), 777.0, dtype=torch.float32, device=DEV)
    vo = torch.full((n,), 777.0, dtype=torch.float32, device=DEV) if var else None
    if monkeypatch is not None:
        if form is None:
            monkeypatch.delenv("IPT_DENOISE_FORM", raising=False)
        else:
            monkeypatch.setenv("IPT_DENOISE_FORM", form)
    ctx.denoise_device(dp, tp.data_ptr(), tc.data_ptr(), tm.data_ptr(), tg.data_ptr(), out.data_ptr(),
                       vo.data_ptr() if var else None)
    ctx.wait()
    torch.cuda.synchronize()
    return _h(out), (_h(vo) if var else None)


def _check_filter(ctx, monkeypatch, W, H, px, cn, m2, g, what="", ref=None, **kw):
    """Every form against the restatement (ref: its planes, where a test
    shares them), colour and variance."""
    ro, rv = ref if ref is not None else dn.denoise(px, cn, m2, g, W, H, **kw)
    dp = capi.make_denoise_params(W, H, **kw)
    for form in FORMS:
        out, var = _denoise(ctx, dp, px, cn, m2, g, form=form, monkeypatch=monkeypatch)
        _same(out, ro, (what, form, "out"))
        _same(var, rv, (what, form, "var"))
    return ro, rv


def _render(ctx, W, H, plane=dn.GRID, spp=dn.RENDER_SPP):
    """4 passes of the box scene through ipt_render_masked_device with m2."""
    ctx.upload_scene(scenes.make_scene_box())
    p = capi.make_params(W, H, spp, flags=ac.FLAG[plane], **dn.RENDER)
    t = {k: _t(v) for k, v in dc.plane(W, H).items()}
    tm2 = _t(np.zeros(W * H, F))
    ctx.render_masked_device(p, t["pixels"].data_ptr(), t["counters"].data_ptr(), t["sums"].data_ptr(),
                             t["pixel_max"].data_ptr(), mask_ptr=None, m2_ptr=tm2.data_ptr())
    torch.cuda.synchronize()
    return _h(t["pixels"]), _h(t["counters"]), _h(tm2)


# ---- guides ------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", ((37, 23), (13, 11), (1, 1), (1, 7), (7, 1), (2, 3)), ids=lambda f: "%dx%d" % f)
def test_guides_box(gpu_ctx, oracle, frame, plane):
    W, H = frame
    gpu_ctx.upload_scene(scenes.make_scene_box())
    ref = dn.box_guides(W, H, plane)
    got = _guides(gpu_ctx, capi.make_params(W, H, 1, flags=ac.FLAG[plane]))
    _guides_equal(got, ref, (frame, plane))
    if plane == dn.GRID and H >= 2:
        assert (got["kind"][H - 1] == 0xff).all() and not got["pos"][H - 1].any()
    if W * H > 100:
        assert ((got["kind"] & 3) == 1).sum() > W * H // 4
    # n_rays, depth_max and IPT_FLAG_PREVIEW change nothing
    p = capi.make_params(W, H, 1, n_rays=0, depth_max=0, flags=ac.FLAG[plane] | capi.IPT_FLAG_PREVIEW)
    _guides_equal(_guides(gpu_ctx, p), ref, (frame, plane, "preview flag"))


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("case", ("floor", "box/up", "spheres3000/up"))
def test_guides_scenes(gpu_ctx, oracle, case, plane):
    """Misses (the floor), a visible light (kind 2: the light's position, a
    zero normal) and a sphere list, from pass 3."""
    W, H = 37, 23
    desc = pc.with_camera(scenes.make_scene_spheres(3000), pc.UP) if case.startswith("spheres") else pc.scene(case)
    ref = dn.scene_guides(desc, W, H, plane, spp_offset=3)
    o = ref["kind"][ref["kind"] != 0xff] & 3
    assert (o == 1).any()
    if case == "floor":
        assert (o == 0).any()
    if case == "box/up":
        light = (ref["kind"] != 0xff) & ((ref["kind"] & 3) == 2)
        assert light.any() and not ref["normal"][light].any() and ref["pos"][light].any()
    gpu_ctx.upload_scene(desc)
    got = _guides(gpu_ctx, capi.make_params(W, H, 1, spp_offset=3, flags=ac.FLAG[plane]))
    _guides_equal(got, ref, (case, plane))
    assert not np.array_equal(ref.view(np.uint8), dn.scene_guides(desc, W, H, plane, spp_offset=0).view(np.uint8))


def test_guides_errors_leave_the_plane(gpu_ctx, oracle):
    W, H = 13, 11
    gpu_ctx.upload_scene(scenes.make_scene_box())
    g = torch.full((W * H * 32,), 0xa5, dtype=torch.uint8, device=DEV)
    bad = ((capi.make_params(W, H, 2), capi.IPT_E_INVALID), (capi.make_params(W, H, 0), capi.IPT_E_INVALID),
           (capi.make_params(W, H, 1, tile_rows=4, n_shards=2), capi.IPT_E_UNSUPPORTED),
           (capi.make_params(W, H, 1, flags=capi.IPT_FLAG_COUNTERS), capi.IPT_E_UNSUPPORTED),
           (capi.make_params(W, H, 1, flags=capi.IPT_FLAG_COMPACT), capi.IPT_E_UNSUPPORTED),
           (capi.make_params(0, H, 1), capi.IPT_E_INVALID))
    for p, code in bad:
        with pytest.raises(capi.IptError) as e:
            gpu_ctx.guides_device(p, g.data_ptr())
        assert e.value.code == code
    with pytest.raises(capi.IptError) as e:
        gpu_ctx.guides_device(capi.make_params(W, H, 1), None)
    assert e.value.code == capi.IPT_E_INVALID
    gpu_ctx.wait()
    torch.cuda.synchronize()
    assert (g.cpu().numpy() == 0xa5).all()


# ---- the filter on rendered planes ---------------------------------------------------------
@pytest.mark.parametrize("iterations", (1, 3, 6))
@pytest.mark.parametrize("frame", dn.FRAMES + ((13, 11),) + dn.TINY_FRAMES, ids=lambda f: "%dx%d" % f)
def test_filter_rendered(gpu_ctx, oracle, monkeypatch, frame, iterations):
    """131 x 67 is wider and taller than a tile and a multiple of neither tile
    size; on 13 x 11 and 37 x 23 iteration 6's step 32 leaves the centre tap
    alone; on the tiny frames most or all taps are out of frame."""
    W, H = frame
    px, cn, m2 = _render(gpu_ctx, W, H)
    img, rm2 = dn.box_plane(W, H)
    _bits(px, img["pixels"], "pixels")
    _bits(m2, rm2, "m2")
    g = _guides(gpu_ctx, capi.make_params(W, H, 1))
    _guides_equal(g, dn.box_guides(W, H))
    ro, _ = _check_filter(gpu_ctx, monkeypatch, W, H, px, cn, m2, g, frame, iterations=iterations)
    if W * H > 100:
        assert not np.array_equal(ro, px)


@pytest.mark.parametrize("normal_pow", (0, 2, 7))
def test_filter_normal_pow(gpu_ctx, oracle, monkeypatch, normal_pow):
    W, H = 37, 23
    img, m2 = dn.box_plane(W, H)
    _check_filter(gpu_ctx, monkeypatch, W, H, img["pixels"], img["counters"], m2, dn.box_guides(W, H),
                  iterations=3, normal_pow=normal_pow, sigma_l=8.0, sigma_z=0.05)


def test_filter_gui_plane(gpu_ctx, oracle, monkeypatch):
    W, H = 37, 23
    px, cn, m2 = _render(gpu_ctx, W, H, dn.GUI)
    img, rm2 = dn.box_plane(W, H, plane=dn.GUI)
    _bits(px, img["pixels"], "pixels")
    _bits(m2, rm2, "m2")
    g = _guides(gpu_ctx, capi.make_params(W, H, 1, flags=ac.FLAG[dn.GUI]))
    _guides_equal(g, dn.box_guides(W, H, dn.GUI))
    _check_filter(gpu_ctx, monkeypatch, W, H, px, cn, m2, g, iterations=4)


# ---- participation edges -------------------------------------------------------------------
def test_starved_pixels_among_participating_ones(gpu_ctx, oracle, monkeypatch):
    """One unmasked pass, then one under the half mask: half the pixels have
    c = 1 and take no part."""
    W, H = 37, 23
    gpu_ctx.upload_scene(scenes.make_scene_box())
    mask = ac.half_mask(W, H)
    t = {k: _t(v) for k, v in dc.plane(W, H).items()}
    tm2, tmask = _t(np.zeros(W * H, F)), _t(mask.reshape(-1))
    for s, m in ((0, None), (1, tmask)):
        p = capi.make_params(W, H, 1, spp_offset=s, **dn.RENDER)
        gpu_ctx.render_masked_device(p, t["pixels"].data_ptr(), t["counters"].data_ptr(), t["sums"].data_ptr(),
                                     t["pixel_max"].data_ptr(), mask_ptr=None if m is None else m.data_ptr(),
                                     m2_ptr=tm2.data_ptr())
    torch.cuda.synchronize()
    px, cn, m2 = _h(t["pixels"]), _h(t["counters"]), _h(tm2)
    g = dn.box_guides(W, H)
    part = dn.participation(px, cn, m2, g.reshape(-1))
    assert (cn < 2).sum() > 100 and part.sum() > 100
    ro, rv = _check_filter(gpu_ctx, monkeypatch, W, H, px, cn, m2, g, iterations=3)
    _bits(ro[~part], px[~part], "copied")
    assert (rv[cn < 2] == 0).all()


def test_poisoned_pixels_are_copied_and_poison_nothing(gpu_ctx, oracle, monkeypatch):
    """NaN, +inf, negative and -0.0 pixels, inf and NaN m2, on and next to
    participating pixels: the non-finite ones are copied bit for bit (the NaN's
    payload included) and no neighbour becomes non-finite."""
    W, H = 37, 23
    img, m2 = dn.box_plane(W, H)
    px, cn, m2 = img["pixels"].copy(), img["counters"].copy(), m2.copy()
    g = dn.box_guides(W, H)
    part0 = dn.participation(px, cn, m2, g.reshape(-1))
    idx = np.flatnonzero(part0.reshape(H, W)[2:H - 3, 2:W - 2].reshape(-1))
    sel = [int(i) for i in idx[np.linspace(0, idx.size - 1, 7).astype(int)]]
    at = [(2 + i // (W - 4)) * W + 2 + i % (W - 4) for i in sel]
    px[at[0]] = np.uint32(0x7fc12345).view(F)
    px[at[1]] = F(np.inf)
    px[at[2]] = F(-0.25)
    px[at[3]] = F(-0.0)
    m2[at[4]] = F(np.inf)
    m2[at[5]] = np.uint32(0xffc00001).view(F)
    m2[at[6]] = F(-1e-3)
    part = dn.participation(px, cn, m2, g.reshape(-1))
    out_of = [at[0], at[1], at[4], at[5]]
    assert not part[out_of].any() and part[[at[2], at[3], at[6]]].all()
    ro, rv = _check_filter(gpu_ctx, monkeypatch, W, H, px, cn, m2, g, iterations=3)
    dp = capi.make_denoise_params(W, H, iterations=3)
    out, var = _denoise(gpu_ctx, dp, px, cn, m2, g)
    assert np.array_equal(dc.bits(out[out_of]), dc.bits(px[out_of]))
    _same(var[out_of], dn.var0_of(cn, m2)[out_of], "var0 of the copied pixels")
    others = np.ones(W * H, bool)
    others[out_of] = False
    assert np.isfinite(out[others]).all()


# ---- synthetic guides ------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("guides", ("crease", "step"))
def test_filter_synthetic(gpu_ctx, oracle, monkeypatch, guides, iterations):
    W, H = 67, 35
    g = dn.crease_guides(W, H) if guides == "crease" else dn.step_guides(W, H)
    px, cn, m2 = dn.random_plane(W, H, iterations)
    ro, rv = _check_filter(gpu_ctx, monkeypatch, W, H, px, cn, m2, g, (guides, iterations), iterations=iterations,
                           sigma_l=6.0)
    dp = capi.make_denoise_params(W, H, iterations=iterations, sigma_l=6.0)
    for form in FORMS[1:]:
        out, var = _denoise(gpu_ctx, dp, px, cn, m2, g, var=False, form=form, monkeypatch=monkeypatch)
        assert var is None
        _same(out, ro, (guides, iterations, form, "var_out NULL"))
    assert not np.array_equal(ro, px)


def test_depth_step_stops_the_filter(gpu_ctx, oracle, monkeypatch):
    """dn.two_level_plane on dn.step_guides: the kernels give the restatement's
    plane, which test_denoise_cpu.py shows to keep the colour edge exactly."""
    W, H = 67, 35
    px, cn, m2 = dn.two_level_plane(W, H)
    ro, _ = _check_filter(gpu_ctx, monkeypatch, W, H, px, cn, m2, dn.step_guides(W, H), iterations=4, sigma_l=1000.0)
    _bits(ro, px, "the edge is kept")


# ---- lattice tiles ---------------------------------------------------------------------------
# The tiled form's taps leave their workgroup's 32 x 8 lattice tile along x
# where W > 32 s and along y where H > 8 s: on 300 x 75 at steps 4 and 8, on
# 1061 x 9 along x and on 9 x 277 along y up to step 32, on 1061 x 277 both
# (tests/test_denoise_cpu.py pins how many pixels a dropped halo tap changes).
SEAM_ITERATIONS = {(300, 75): 4, (1061, 9): 6, (9, 277): 6, (1061, 277): 6}


@functools.lru_cache(maxsize=None)
def _seam_case(W, H, guides="crease"):
    """(pixels, counters, m2, guides, keywords, the restatement's planes), read-only."""
    px, cn, m2 = dn.random_plane(W, H, 6)
    g = dn.crease_guides(W, H) if guides == "crease" else dn.step_guides(W, H)
    kw = dict(iterations=SEAM_ITERATIONS[W, H], sigma_l=6.0)
    ref = dn.denoise(px, cn, m2, g, W, H, **kw)
    for a in (px, cn, m2, g) + ref:
        a.setflags(write=False)
    return px, cn, m2, g, kw, ref


@pytest.mark.parametrize("frame", dn.SEAM_FRAMES, ids=lambda f: "%dx%d" % f)
def test_filter_across_lattice_tiles(gpu_ctx, oracle, monkeypatch, frame):
    W, H = frame
    px, cn, m2, g, kw, ref = _seam_case(W, H)
    _check_filter(gpu_ctx, monkeypatch, W, H, px, cn, m2, g, frame, ref=ref, **kw)
    assert not np.array_equal(ref[0], px)


def test_filter_across_lattice_tiles_on_a_depth_step_and_without_var(gpu_ctx, oracle, monkeypatch):
    W, H = 300, 75
    px, cn, m2, g, kw, ref = _seam_case(W, H, "step")
    _check_filter(gpu_ctx, monkeypatch, W, H, px, cn, m2, g, "step", ref=ref, **kw)
    assert not np.array_equal(ref[0], px)
    px, cn, m2, g, kw, ref = _seam_case(W, H)
    dp = capi.make_denoise_params(W, H, **kw)
    for form in FORMS:
        out, var = _denoise(gpu_ctx, dp, px, cn, m2, g, var=False, form=form, monkeypatch=monkeypatch)
        assert var is None
        _same(out, ref[0], (form, "var_out NULL"))


def test_filter_rendered_across_a_tile_at_step_8(gpu_ctx, oracle, monkeypatch):
    """The box scene on 300 x 75 through the chain, 4 iterations: the shipped
    form's last tiled step, 8, with ten tile columns per residue."""
    W, H = 300, 75
    px, cn, m2 = _render(gpu_ctx, W, H)
    img, rm2 = dn.box_plane(W, H)
    _bits(px, img["pixels"], "pixels")
    _bits(m2, rm2, "m2")
    g = _guides(gpu_ctx, capi.make_params(W, H, 1))
    _guides_equal(g, dn.box_guides(W, H))
    ro, _ = _check_filter(gpu_ctx, monkeypatch, W, H, px, cn, m2, g, "box 300x75", iterations=4)
    assert not np.array_equal(ro, px)


def test_small_frame_queued_behind_a_large_one(oracle):
    """1061 x 277 and then 37 x 23 on one context with no wait between the
    calls: the small frame's second record plane lies where the large frame's
    does, 345 small frames into the scratch, not behind its own first one."""
    ctx = capi.Context(0)
    try:
        W, H = 1061, 277
        px, cn, m2, g, kw, ref = _seam_case(W, H)
        w, h = 37, 23
        spx, scn, sm2 = dn.random_plane(w, h, 6)
        sg = dn.crease_guides(w, h)
        big = [_t(a) for a in (px, cn, m2, g)]
        small = [_t(a) for a in (spx, scn, sm2, sg)]
        outs = [torch.full((n,), 777.0, dtype=torch.float32, device=DEV) for n in (W * H, W * H, w * h, w * h)]
        torch.cuda.synchronize()
        ctx.denoise_device(capi.make_denoise_params(W, H, **kw), *(t.data_ptr() for t in big), outs[0].data_ptr(),
                           outs[1].data_ptr())
        ctx.denoise_device(capi.make_denoise_params(w, h, iterations=5, sigma_l=6.0), *(t.data_ptr() for t in small),
                           outs[2].data_ptr(), outs[3].data_ptr())
        ctx.wait()
        torch.cuda.synchronize()
        _same(_h(outs[0]), ref[0], "large out")
        _same(_h(outs[1]), ref[1], "large var")
        ro, rv = dn.denoise(spx, scn, sm2, sg, w, h, iterations=5, sigma_l=6.0)
        _same(_h(outs[2]), ro, "small out")
        _same(_h(outs[3]), rv, "small var")
    finally:
        ctx.close()


# ---- values outside the in-range window --------------------------------------------------------
@pytest.mark.parametrize("name", dn.EDGE_CASES)
def test_filter_edge_planes(gpu_ctx, oracle, monkeypatch, name):
    """Operands outside [2^-40, 2^41) (division) and [2^-96, 2^126) (root),
    denormal operands and results, counters past 2^24 and 2^31, sv / 0
    (tests/test_denoise_cpu.py pins the census of each plane)."""
    W, H = 67, 35
    px, cn, m2, g, kw = dn.edge_case(name)
    ro, rv = _check_filter(gpu_ctx, monkeypatch, W, H, px, cn, m2, g, name, **kw)
    assert not np.array_equal(ro, px)


@pytest.mark.parametrize("name", ("counters_mix", "colour_e-64", "world_e-45"))
def test_filter_edge_planes_in_halos(gpu_ctx, oracle, monkeypatch, name):
    W, H = 300, 75
    px, cn, m2, g, kw = dn.edge_case(name, W, H)
    ro, rv = _check_filter(gpu_ctx, monkeypatch, W, H, px, cn, m2, g, name, **dict(kw, iterations=4))
    assert not np.array_equal(ro, px)


@pytest.mark.parametrize("infinite_normals", (False, True))
def test_guides_that_are_no_numbers(gpu_ctx, oracle, monkeypatch, infinite_normals):
    """NaN and infinite guide components on participating pixels and kinds of
    every kind & 3: a NaN-guided pixel keeps its colour, nothing beyond the
    filter's reach differs from the clean run, and without an infinite normal
    every colour is finite (with one, the restatement's NaNs, bit for bit)."""
    W, H, it = 67, 35, 3
    kw = dict(iterations=it, sigma_l=6.0)
    px, cn, m2 = dn.random_plane(W, H, dn.EDGE_SEED)
    g0 = dn.crease_guides(W, H)
    g, where, kinds = dn.poisoned_guides(g0, dn.participation(px, cn, m2, g0.reshape(-1)), infinite_normals)
    _check_filter(gpu_ctx, monkeypatch, W, H, px, cn, m2, g, "poisoned guides", **kw)
    dp = capi.make_denoise_params(W, H, **kw)
    clean, clean_var = _denoise(gpu_ctx, dp, px, cn, m2, g0)
    out, var = _denoise(gpu_ctx, dp, px, cn, m2, g)
    kept = [where[k] for k in ("pos_nan", "pos_snan", "normal_nan", "pos_inf")]
    _bits(out[kept], px[kept], "NaN-guided pixels keep their colour")
    off = [i for i, k in kinds.items() if (k & 3) != 1]
    _bits(out[off], px[off], "copied")
    r = 2 * (2 ** it - 1)
    far = ~dn.reach(W, H, list(where.values()) + list(kinds), r)
    assert far.sum() >= 18
    _bits(out[far], clean[far], "beyond the reach")
    _bits(var[far], clean_var[far], "beyond the reach, var")
    assert not np.array_equal(out, clean)
    if infinite_normals:
        inf_at = [where["normal_pinf"], where["normal_ninf"]]
        assert np.isnan(out[inf_at]).all() and np.isfinite(out[~dn.reach(W, H, inf_at, r)]).all()
    else:
        assert np.isfinite(out).all()


# ---- stream order ----------------------------------------------------------------------------
def _chain(ctx, W, H, stream, staged):
    """masked render -> guides -> denoise -> display on `stream`; staged: a
    host wait after every call. Returns (gray8, out) on the host."""
    n = W * H
    t = {k: _t(v) for k, v in dc.plane(W, H).items()}
    tm2 = torch.zeros(n, dtype=torch.float32, device=DEV)
    tg = torch.zeros(n * 32, dtype=torch.uint8, device=DEV)
    out = torch.zeros(n, dtype=torch.float32, device=DEV)
    g8 = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    h = stream.cuda_stream
    p = capi.make_params(W, H, dn.RENDER_SPP, **dn.RENDER)

    def step():
        if staged:
            ctx.wait()
            torch.cuda.synchronize()

    with torch.cuda.stream(stream):
        ctx.render_masked_device_async(p, t["pixels"].data_ptr(), t["counters"].data_ptr(), t["sums"].data_ptr(),
                                       t["pixel_max"].data_ptr(), mask_ptr=None, m2_ptr=tm2.data_ptr(), stream=h)
        step()
        ctx.guides_device(capi.make_params(W, H, 1), tg.data_ptr(), h)
        step()
        ctx.denoise_device(capi.make_denoise_params(W, H), t["pixels"].data_ptr(), t["counters"].data_ptr(),
                           tm2.data_ptr(), tg.data_ptr(), out.data_ptr(), None, h)
        step()
        ctx.display_device(capi.make_display_params(W, H), out.data_ptr(), g8.data_ptr(), stream=h)
    stream.synchronize()
    res = g8.cpu().numpy(), out.cpu().numpy()
    ctx.wait()
    return res


def test_chain_in_stream_order(oracle):
    """No host wait between the four calls, on one stream and then on a second
    one (the filter's scratch is the context's: the second stream's call waits
    on the first's event), two frame sizes alternating so that the scratch
    regrows: every frame equals the staged chain and the restatement."""
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(scenes.make_scene_box())
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        frames = ((37, 23), (64, 48))
        staged = {f: _chain(ctx, *f, s1, True) for f in frames}
        for f in frames:
            img, m2 = dn.box_plane(*f)
            ro, _ = dn.denoise(img["pixels"], img["counters"], m2, dn.box_guides(*f), *f)
            _same(staged[f][1], ro, ("staged", f))
            assert staged[f][0].max() == 255
        for s in (s1, s2, s1, s2):
            for f in frames:
                g8, out = _chain(ctx, *f, s, False)
                _same(out, staged[f][1], ("queued", f))
                assert np.array_equal(g8, staged[f][0])
        # two streams with no host wait between their calls
        W, H = frames[1]
        img, m2 = dn.box_plane(W, H)
        g = dn.box_guides(W, H)
        tp, tc, tm, tg = _t(img["pixels"]), _t(img["counters"]), _t(m2), _t(g)
        outs = [torch.zeros(W * H, dtype=torch.float32, device=DEV) for _ in range(4)]
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            ctx.denoise_device(capi.make_denoise_params(W, H, iterations=1 + k), tp.data_ptr(), tc.data_ptr(),
                               tm.data_ptr(), tg.data_ptr(), o.data_ptr(), None, (s1, s2)[k & 1].cuda_stream)
        ctx.wait()
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            _same(o.cpu().numpy(), dn.denoise(img["pixels"], img["counters"], m2, g, W, H, iterations=1 + k)[0], k)
    finally:
        ctx.close()


# ---- errors ----------------------------------------------------------------------------------
def test_errors_leave_the_outputs(gpu_ctx, oracle):
    W, H = 13, 11
    n = W * H
    img, m2 = dn.box_plane(W, H)
    buf = torch.full((n * 16,), 3.5, dtype=torch.float32, device=DEV)  # one allocation: overlaps are views of it
    base = buf.data_ptr()
    px, cn, mm, gd, out, var = (base + 4 * n * k for k in (0, 1, 2, 3, 11, 12))  # guides: 8 planes' worth
    buf[0:n] = _t(img["pixels"])
    before = buf.cpu().numpy().copy()
    ok = dict(iterations=3, sigma_l=4.0, normal_pow=2, sigma_z=0.1)

    def call(code, ptrs=None, w=W, h=H, **kw):
        dp = capi.make_denoise_params(w, h, **dict(ok, **kw))
        with pytest.raises(capi.IptError) as e:
            gpu_ctx.denoise_device(dp, *(ptrs or (px, cn, mm, gd, out, var)))
        assert e.value.code == code, (kw, ptrs)

    for kw in (dict(iterations=0), dict(iterations=7), dict(normal_pow=-1), dict(normal_pow=8), dict(sigma_l=0.0),
               dict(sigma_l=-1.0), dict(sigma_l=float("nan")), dict(sigma_z=0.0), dict(sigma_z=float("nan"))):
        call(capi.IPT_E_INVALID, **kw)
    call(capi.IPT_E_INVALID, w=0)
    call(capi.IPT_E_INVALID, h=-1)
    call(capi.IPT_E_UNSUPPORTED, w=65536, h=32769)
    for k in range(5):  # each mandatory pointer NULL
        ptrs = [px, cn, mm, gd, out, var]
        ptrs[k] = None
        call(capi.IPT_E_INVALID, tuple(ptrs))
    last = 4 * (n - 1)
    for ptrs in ((px, cn, mm, gd, px, var), (px, cn, mm, gd, px + last, var), (px, cn, mm, gd, cn, var),
                 (px, cn, mm, gd, mm - last, var), (px, cn, mm, gd, gd + 32 * n - 4, var),
                 (px, cn, mm, gd, out, px), (px, cn, mm, gd, out, cn + last), (px, cn, mm, gd, out, mm),
                 (px, cn, mm, gd, out, gd), (px, cn, mm, gd, out, out), (px, cn, mm, gd, out, out + last)):
        call(capi.IPT_E_INVALID, ptrs)
    gpu_ctx.wait()
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), before.view(np.uint32))
    # adjacent buffers are no overlap
    gpu_ctx.denoise_device(capi.make_denoise_params(W, H, **ok), px, cn, mm, gd, out, var)
    gpu_ctx.wait()


# ---- host form -------------------------------------------------------------------------------
@pytest.mark.parametrize("var", (True, False))
def test_host_form_equals_device_form(gpu_ctx, oracle, var):
    W, H = 64, 48
    img, m2 = dn.box_plane(W, H)
    g = dn.box_guides(W, H)
    dp = capi.make_denoise_params(W, H)
    out, vo = gpu_ctx.denoise(dp, img["pixels"], img["counters"], m2, g, var=var)
    dout, dvo = _denoise(gpu_ctx, dp, img["pixels"], img["counters"], m2, g, var=var)
    _bits(out, dout)
    ro, rv = dn.denoise(img["pixels"], img["counters"], m2, g, W, H)
    _same(out, ro)
    if var:
        _bits(vo, dvo)
        _same(vo, rv)
    else:
        assert vo is None and dvo is None
    with pytest.raises(capi.IptError) as e:
        gpu_ctx.denoise(capi.make_denoise_params(W, H, iterations=9), img["pixels"], img["counters"], m2, g)
    assert e.value.code == capi.IPT_E_INVALID


def test_host_guides_equal_device_guides(gpu_ctx, oracle):
    W, H = 37, 23
    gpu_ctx.upload_scene(scenes.make_scene_box())
    for plane in ac.PLANES:
        p = capi.make_params(W, H, 1, spp_offset=2, flags=ac.FLAG[plane])
        _guides_equal(gpu_ctx.guides(p), _guides(gpu_ctx, p), plane)
        _guides_equal(gpu_ctx.guides(p), dn.box_guides(W, H, plane, 2), plane)


def test_pass_times_probe(oracle, monkeypatch):
    """ipt_denoise_pass_ms: nothing without IPT_DENOISE_PROFILE=1, a time for
    the prepare pass and each iteration with it; the outputs are the same."""
    W, H = 64, 48
    img, m2 = dn.box_plane(W, H)
    g = dn.box_guides(W, H)
    dp = capi.make_denoise_params(W, H, iterations=3)
    ctx = capi.Context(0)
    try:
        monkeypatch.delenv("IPT_DENOISE_PROFILE", raising=False)
        plain, _ = _denoise(ctx, dp, img["pixels"], img["counters"], m2, g)
        with pytest.raises(capi.IptError) as e:
            ctx.denoise_pass_ms()
        assert e.value.code == capi.IPT_E_INVALID
        monkeypatch.setenv("IPT_DENOISE_PROFILE", "1")
        timed, _ = _denoise(ctx, dp, img["pixels"], img["counters"], m2, g)
        ms = ctx.denoise_pass_ms()
        assert all(x > 0 for x in ms[:4]) and ms[4:] == [0.0, 0.0, 0.0]
        _bits(timed, plain)
    finally:
        ctx.close()
