"""Adaptive sampling on the device against tests/adaptive_cases.py's numpy
restatement: masked renders (ipt_render_masked_device[_async]) with their
second-moment plane, the next mask (ipt_adapt_device) and the loop, device-
resident and through ipt_render_adaptive. Planes, m2 and masks are compared
bit for bit; tests/test_adaptive_cpu.py pins, without a GPU, that the cases
hold what this file relies on."""
import numpy as np
import pytest
import torch

import adaptive_cases as ac
import drift_cases as dc
import gui_cases as gc
import preview_cases as pc
import preview_ref
from ipt_amd import capi, scenes

pytestmark = pytest.mark.gpu

bits = dc.bits
KEYS = tuple(k for k, _ in dc.PLANE_KEYS)
BARE = ("pixels", "counters")
DEV = torch.device("cuda", 0)


def _box(ctx):
    ctx.upload_scene(scenes.make_scene_box())


def _t(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).to(DEV)


def _h(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _to_device(img, keys=KEYS):
    return {k: _t(img[k]) for k in keys}


def _to_host(t):
    return {k: _h(v) for k, v in t.items()}


def _ptrs(t):
    return (t["pixels"].data_ptr(), t["counters"].data_ptr(), t["sums"].data_ptr() if "sums" in t else None,
            t["pixel_max"].data_ptr() if "pixel_max" in t else None)


def _assert_plane_equal(img, ref, keys=KEYS, what=""):
    for k in keys:
        bad = bits(img[k]) != bits(ref[k])
        assert not bad.any(), (what, k, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())


def _assert_bits(a, b, what=""):
    bad = bits(a) != bits(b)
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())


def _assert_bits_nan(a, b, what=""):
    """Bit for bit, except that a NaN equals a NaN. For m2 over a preloaded
    plane alone: on a NaN pixel (v - p_old) * (v - p_new) multiplies two NaNs,
    and which operand's sign and payload the product carries is the
    processor's choice (x86 keeps the first operand's, the GPU need not), as
    drift_cases.preload notes for generated NaNs. From a zeroed plane no NaN
    arises and m2 is compared bit for bit."""
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (what, "NaN positions", np.flatnonzero(na != nb)[:8].tolist())
    _assert_bits(np.where(na, np.float32(0), a), np.where(nb, np.float32(0), b), what)


def _masked(ctx, p, mask, img=None, m2=None, keys=KEYS, with_m2=True, sync=True, stream=None):
    """One masked render into a device copy of img / m2 (zeros if None);
    returns (plane, m2 or None) on the host."""
    W, H = p.width, p.height
    t = _to_device(dc.plane(W, H) if img is None else img, keys)
    tm2 = _t(np.zeros(W * H, np.float32) if m2 is None else m2) if with_m2 else None
    tmask = None if mask is None else _t(np.ascontiguousarray(mask, np.uint8).reshape(-1))
    call = ctx.render_masked_device if sync else ctx.render_masked_device_async
    call(p, *_ptrs(t), mask_ptr=None if tmask is None else tmask.data_ptr(),
         m2_ptr=None if tm2 is None else tm2.data_ptr(), stream=stream)
    if not sync:
        ctx.wait()
    torch.cuda.synchronize()
    return _to_host(t), (None if tm2 is None else _h(tm2))


def _params(W, H, spp, plane, **kw):
    kw["flags"] = kw.get("flags", 0) | ac.FLAG[plane]
    return dc.params(W, H, spp, **kw)


def _samples(W, H, spp, plane, spp_offset=0):
    return dc.oracle_samples(W, H, spp, spp_offset)[0], ac.codes_of(W, H, spp, plane, spp_offset)


# ---- explicit masks ----------------------------------------------------------------------
SMALL_FRAMES = ((1, 1, 9), (2, 2, 9), (5, 4, 9), (13, 11, 9), (257, 5, 9))


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", SMALL_FRAMES + ac.HALF_FRAMES, ids=lambda f: "%dx%dx%d" % f)
def test_explicit_mask(gpu_ctx, oracle, frame, plane):
    """The seeded half mask: plane, m2 and the counting instance's paths and
    drifted against the masked replay; then without sums / pixel_max and
    without m2. On the drift frames drifted samples cross between active and
    masked pixels both ways (test_adaptive_cpu.py pins how many)."""
    W, H, spp = frame
    _box(gpu_ctx)
    v, c = _samples(W, H, spp, plane)
    mask = ac.half_mask(W, H)
    if W * H == 1:
        mask[:] = 1  # (the one-pixel frame: an active pixel; its masked twin is the all-zero corner)
    ref, rm2 = ac.replay(v, c, mask, plane)
    gpu_ctx.reset_counters()
    got, m2 = _masked(gpu_ctx, _params(W, H, spp, plane, flags=capi.IPT_FLAG_COUNTERS), mask)
    _assert_plane_equal(got, ref, what="all arrays")
    _assert_bits(m2, rm2, "m2")
    paths, drifted = ac.counts(c, mask, plane)
    cnt = gpu_ctx.counters()
    assert (cnt["paths"], cnt["drifted"]) == (paths, drifted)
    p = _params(W, H, spp, plane)
    got, m2 = _masked(gpu_ctx, p, mask, keys=BARE)
    _assert_plane_equal(got, ref, BARE, what="no sums / pixel_max")
    _assert_bits(m2, rm2, "m2, no sums / pixel_max")
    got, m2 = _masked(gpu_ctx, p, mask, with_m2=False)
    assert m2 is None
    _assert_plane_equal(got, ref, what="m2 NULL")
    got, _ = _masked(gpu_ctx, p, mask, keys=("pixels", "counters", "sums"), with_m2=False)
    _assert_plane_equal(got, ref, ("pixels", "counters", "sums"), what="m2 and pixel_max NULL")


# ---- mask corners ------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ac.PLANES)
def test_all_zero_mask_leaves_a_preloaded_plane(gpu_ctx, oracle, plane):
    W, H, spp = 13, 11, 9
    _box(gpu_ctx)
    pre, _ = dc.preload(W, H, spp)
    pm2 = np.random.default_rng(3).random(W * H, dtype=np.float32)
    gpu_ctx.reset_counters()
    got, m2 = _masked(gpu_ctx, _params(W, H, spp, plane, flags=capi.IPT_FLAG_COUNTERS), np.zeros((H, W), np.uint8),
                      img=pre, m2=pm2)
    _assert_plane_equal(got, pre, what="all-zero mask")
    _assert_bits(m2, pm2, "m2")
    cnt = gpu_ctx.counters()
    assert cnt["paths"] == 0 and cnt["drifted"] == 0 and cnt["traced_rays"] == 0
    got, _ = _masked(gpu_ctx, _params(1, 1, 9, plane), np.zeros((1, 1), np.uint8))
    assert not got["counters"].any() and not bits(got["pixels"]).any()


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", ((13, 11, 9), (4099, 61, 2)), ids=lambda f: "%dx%dx%d" % f)
def test_all_ones_and_null_mask_equal_the_unmasked_render(gpu_ctx, oracle, frame, plane):
    """Bit for bit ipt_render_device's plane, into a preloaded plane too; m2
    against the restatement."""
    W, H, spp = frame
    _box(gpu_ctx)
    p = _params(W, H, spp, plane)
    v, c = _samples(W, H, spp, plane)
    pre, _ = dc.preload(W, H, spp)
    for img in (None, pre):
        t = _to_device(dc.plane(W, H) if img is None else img)
        gpu_ctx.render_device(p, *_ptrs(t))
        torch.cuda.synchronize()
        plain = _to_host(t)
        _, rm2 = ac.replay(v, c, None, plane, img=None if img is None else dc.copy_plane(img))
        for mask in (np.ones((H, W), np.uint8), np.full((H, W), 0xff, np.uint8), None):
            got, m2 = _masked(gpu_ctx, p, mask, img=img)
            _assert_plane_equal(got, plain, what="mask %s" % (None if mask is None else int(mask[0, 0])))
            (_assert_bits if img is None else _assert_bits_nan)(m2, rm2, "m2")
            assert img is None or np.isnan(rm2).any()
    got, m2 = _masked(gpu_ctx, p, None, with_m2=False)  # neither: the unmasked launches themselves
    _assert_plane_equal(got, dc.oracle_plane(W, H, spp) if plane == ac.GRID else gc.gui_plane(W, H, spp))


def test_grid_row0_mask_renders_both_folded_source_rows(gpu_ctx, oracle):
    """Under the Grid map mask[0][ix] governs source rows H-2 and H-1 alike:
    with row 0 alone active, row 0 gets two samples per pass and nothing else
    gets any."""
    W, H, spp = 13, 11, 9
    _box(gpu_ctx)
    mask = np.zeros((H, W), np.uint8)
    mask[0] = 1
    v, c = _samples(W, H, spp, ac.GRID)
    assert (c[:, H - 2:] == 0x05).all()
    ref, rm2 = ac.replay(v, c, mask, ac.GRID)
    gpu_ctx.reset_counters()
    got, m2 = _masked(gpu_ctx, _params(W, H, spp, ac.GRID, flags=capi.IPT_FLAG_COUNTERS), mask)
    _assert_plane_equal(got, ref)
    _assert_bits(m2, rm2, "m2")
    cn = got["counters"].reshape(H, W)
    assert (cn[0] == 2 * spp).all() and not cn[1:].any()
    assert gpu_ctx.counters()["paths"] == 2 * spp * W
    # the same mask under the Gui map: row 0 is source row H-1's alone
    ref, _ = ac.replay(v, ac.codes_of(W, H, spp, ac.GUI), mask, ac.GUI)
    got, _ = _masked(gpu_ctx, _params(W, H, spp, ac.GUI), mask)
    _assert_plane_equal(got, ref)
    assert (got["counters"].reshape(H, W)[0] == spp).all()


def test_overlapping_buffers_are_refused(gpu_ctx, oracle):
    W, H = 13, 11
    _box(gpu_ctx)
    p = dc.params(W, H, 1)
    t = _to_device(dc.plane(W, H))
    mask = _t(np.ones(W * H, np.uint8))
    m2 = _t(np.zeros(W * H + 4, np.float32))
    before = _to_host(t)
    for kw in (dict(mask_ptr=mask.data_ptr(), m2_ptr=t["sums"].data_ptr()),
               dict(mask_ptr=t["pixels"].data_ptr() + 8, m2_ptr=m2.data_ptr()),
               dict(mask_ptr=m2.data_ptr() + 16, m2_ptr=m2.data_ptr()),
               dict(mask_ptr=None, m2_ptr=t["counters"].data_ptr() + 4 * (W * H - 1))):
        with pytest.raises(capi.IptError) as e:
            gpu_ctx.render_masked_device_async(p, *_ptrs(t), **kw)
        assert e.value.code == capi.IPT_E_INVALID
    gpu_ctx.wait()
    torch.cuda.synchronize()
    _assert_plane_equal(_to_host(t), before, what="nothing was launched")


# ---- launch paths ------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ac.PLANES)
def test_chunked_launches(oracle, monkeypatch, plane):
    """IPT_TEST_CHUNK_UNITS in a fresh context: three launches of three passes,
    then one pass per launch -- every launch reads the mask and rebuilds its
    flags, the two work-slot streams each take the call's one wait."""
    W, H, spp = 13, 11, 9
    v, c = _samples(W, H, spp, plane)
    mask = ac.half_mask(W, H)
    ref, rm2 = ac.replay(v, c, mask, plane)
    for units in (3 * W * H, 1):
        monkeypatch.setenv("IPT_TEST_CHUNK_UNITS", str(units))
        ctx = capi.Context(0)
        try:
            _box(ctx)
            got, m2 = _masked(ctx, _params(W, H, spp, plane), mask)
            _assert_plane_equal(got, ref, what="chunk units %d" % units)
            _assert_bits(m2, rm2, "m2, chunk units %d" % units)
        finally:
            ctx.close()


@pytest.mark.parametrize("plane", ac.PLANES)
def test_queued_calls(gpu_ctx, oracle, plane):
    """Two queued masked calls (5 + 4 passes) equal one call; a masked call
    queued between unmasked ones on one stream is ordered with both (its mask
    is written on that stream just before, and overwritten just after)."""
    W, H, spp = 13, 11, 9
    _box(gpu_ctx)
    v, c = _samples(W, H, spp, plane)
    mask = ac.half_mask(W, H)
    ref, rm2 = ac.replay(v, c, mask, plane)
    s = torch.cuda.Stream(DEV)
    t, tm2, tmask = _to_device(dc.plane(W, H)), _t(np.zeros(W * H, np.float32)), _t(mask.reshape(-1))
    with torch.cuda.stream(s):
        for n, off in ((5, 0), (4, 5)):
            gpu_ctx.render_masked_device_async(_params(W, H, n, plane, spp_offset=off), *_ptrs(t),
                                               mask_ptr=tmask.data_ptr(), m2_ptr=tm2.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    gpu_ctx.wait()
    _assert_plane_equal(_to_host(t), ref, what="5 + 4 passes")
    _assert_bits(_h(tm2), rm2, "m2, 5 + 4 passes")
    # unmasked 3, masked 3, unmasked 3
    ref = dc.plane(W, H)
    rm2 = np.zeros(W * H, np.float32)
    ac.replay(v[:3], c[:3], None, plane, ref, np.zeros(W * H, np.float32))
    ac.replay(v[3:6], c[3:6], mask, plane, ref, rm2)
    ac.replay(v[6:], c[6:], None, plane, ref, np.zeros(W * H, np.float32))
    t, tm2 = _to_device(dc.plane(W, H)), _t(np.zeros(W * H, np.float32))
    tmask = torch.zeros(W * H, dtype=torch.uint8, device=DEV)
    src = _t(mask.reshape(-1))
    with torch.cuda.stream(s):
        gpu_ctx.render_device_async(_params(W, H, 3, plane), *_ptrs(t), stream=s.cuda_stream)
        tmask.copy_(src)  # the mask is produced on the stream, before the call
        gpu_ctx.render_masked_device_async(_params(W, H, 3, plane, spp_offset=3), *_ptrs(t),
                                           mask_ptr=tmask.data_ptr(), m2_ptr=tm2.data_ptr(), stream=s.cuda_stream)
        tmask.zero_()     # and overwritten after it
        gpu_ctx.render_device_async(_params(W, H, 3, plane, spp_offset=6), *_ptrs(t), stream=s.cuda_stream)
    s.synchronize()
    gpu_ctx.wait()
    _assert_plane_equal(_to_host(t), ref, what="unmasked, masked, unmasked")
    _assert_bits(_h(tm2), rm2, "m2 of the masked call")


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("tile,n_shards", ((1, 3), (16, 2)))
def test_sharded_masked_render(gpu_ctx, oracle, tile, n_shards, plane):
    """The mask is the whole frame for every shard; the shards' owned rows,
    assembled, are the unsharded masked plane and m2."""
    W, H, spp = 3, 60000, 2
    _box(gpu_ctx)
    v, c = _samples(W, H, spp, plane)
    mask = ac.half_mask(W, H)
    ref, rm2 = ac.replay(v, c, mask, plane)
    out, om2 = dc.plane(W, H), np.zeros(W * H, np.float32)
    covered = np.zeros(H, np.int32)
    for s in range(n_shards):
        p = _params(W, H, spp, plane, tile_rows=tile, n_shards=n_shards, shard_id=s)
        owned, _ = capi.shard_plan(p)
        covered += owned
        part, pm2 = _masked(gpu_ctx, p, mask)
        rows = np.repeat(owned, W)
        for k in KEYS:
            assert not part[k][~rows].any(), f"shard {s} wrote outside its rows"
            out[k][rows] = part[k][rows]
        assert not pm2[~rows].any()
        om2[rows] = pm2[rows]
    assert (covered == 1).all()
    _assert_plane_equal(out, ref)
    _assert_bits(om2, rm2, "m2")


@pytest.mark.parametrize("plane", ac.PLANES)
def test_masked_preview(gpu_ctx, plane):
    """IPT_FLAG_PREVIEW reads the mask through the same new_path_setup."""
    W, H, spp = 13, 11, 9
    desc = pc.with_camera(scenes.make_scene_box(), pc.UP)
    flags = capi.IPT_FLAG_PREVIEW | ac.FLAG[plane]
    v, c, kinds, _, _ = preview_ref.render(desc, capi.make_params(W, H, spp, flags=flags))
    assert len(np.unique(kinds & 3)) == 3  # miss, surface and light samples
    mask = ac.half_mask(W, H)
    ref, rm2 = ac.replay(v, c, mask, plane)
    gpu_ctx.upload_scene(desc)
    gpu_ctx.reset_counters()
    got, m2 = _masked(gpu_ctx, capi.make_params(W, H, spp, flags=flags | capi.IPT_FLAG_COUNTERS), mask)
    _assert_plane_equal(got, ref)
    _assert_bits(m2, rm2, "m2")
    assert gpu_ctx.counters()["paths"] == ac.counts(c, mask, plane)[0]


# ---- ipt_adapt_device --------------------------------------------------------------------
MIN_COUNT = 8


def _crafted(W, H, seed):
    """Planes whose pixels run through every pairing of the listed counters,
    second moments and means (5 * 8 * 6 = 240 < 257 pixels), then seeded."""
    n = W * H
    cn = np.array([0, 1, MIN_COUNT - 1, MIN_COUNT, 2 ** 24 + 1], np.uint32)
    m2 = np.array([0.0, -1.0, np.inf, np.nan, 1e-3, 3.0, 1e30, 2.0 ** -140], np.float32)
    px = np.array([-0.5, np.nan, 0.0, 0.25, np.inf, 1e-20], np.float32)
    j = np.arange(n)
    rng = np.random.default_rng(seed)
    k = np.where(j < 240, j, rng.integers(0, 240, n))
    pixels, counters, mom = px[(k // 40) % 6].copy(), cn[k % 5].copy(), m2[(k // 5) % 8].copy()
    late = j >= 240  # seeded: counters around min_count, m2 around the threshold
    counters[late] = rng.integers(0, 3 * MIN_COUNT, int(late.sum())).astype(np.uint32)
    pixels[late] = rng.random(int(late.sum()), dtype=np.float32)
    mom[late] = (rng.random(int(late.sum()), dtype=np.float32) * np.float32(8.0)).astype(np.float32)
    return pixels, counters, mom


def _adapt(ctx, ap, pixels, counters, m2, stats=True, stream=None):
    tp, tc, tm = _t(pixels), _t(counters), _t(m2)
    tmask = torch.full((pixels.size,), 0x55, dtype=torch.uint8, device=DEV)
    tstats = torch.full((4,), 0x55555555, dtype=torch.int32, device=DEV)
    ctx.adapt_device(ap, tp.data_ptr(), tc.data_ptr(), tm.data_ptr(), tmask.data_ptr(),
                     tstats.data_ptr() if stats else None, stream)
    ctx.wait()
    torch.cuda.synchronize()
    return _h(tmask), _h(tstats)


@pytest.mark.parametrize("gui", (False, True), ids=("grid", "gui"))
@pytest.mark.parametrize("frame", ((257, 3), (513, 2), (257, 1), (1, 1), (1, 300), (13, 11)), ids=lambda f: "%dx%d" % f)
def test_adapt_device_crafted_planes(gpu_ctx, frame, gui):
    """Counters 0, 1, min_count - 1, min_count and 2^24 + 1; m2 0, negative,
    infinite, NaN and subnormal; pixels negative, NaN and infinite; row H-1 of
    the Grid map with H = 1 (live) and H >= 2 (nobody's); 257 and 513 columns
    (a row crossing the 256-thread blocks)."""
    W, H = frame
    pixels, counters, m2 = _crafted(W, H, seed=W * 1000 + H)
    flags = capi.IPT_FLAG_GUI_PLANE if gui else 0
    for rel, ab in ((0.25, 1e-3), (0.0, 0.0), (1e30, 1e30)):
        ap = capi.make_adapt_params(W, H, MIN_COUNT, rel, ab, flags)
        rmask, rstats = ac.adapt(pixels, counters, m2, W, H, MIN_COUNT, rel, ab, gui)
        mask, stats = _adapt(gpu_ctx, ap, pixels, counters, m2)
        assert np.array_equal(mask, rmask), np.flatnonzero(mask != rmask)[:8].tolist()
        assert stats.tolist() == rstats.tolist()
        if W * H >= 240 and (gui or H == 1) and rel == 0.25:
            assert rstats[0] > rstats[1] > 0 and rstats[2] > 0 and rstats[0] < W * H
    mask, stats = _adapt(gpu_ctx, ap, pixels, counters, m2, stats=False)
    assert np.array_equal(mask, rmask) and (stats == 0x55555555).all()


def test_adapt_device_refuses_before_writing(gpu_ctx):
    W, H = 13, 11
    pixels, counters, m2 = _crafted(W, H, seed=1)
    good = dict(min_count=MIN_COUNT, rel_tol=0.25, abs_tol=1e-3, flags=0)
    cases = [(dict(good, min_count=1), capi.IPT_E_INVALID), (dict(good, min_count=0), capi.IPT_E_INVALID),
             (dict(good, rel_tol=-1.0), capi.IPT_E_INVALID), (dict(good, abs_tol=-1e-9), capi.IPT_E_INVALID),
             (dict(good, rel_tol=float("nan")), capi.IPT_E_INVALID), (dict(good, abs_tol=float("nan")), capi.IPT_E_INVALID),
             (dict(good, flags=capi.IPT_FLAG_COUNTERS), capi.IPT_E_UNSUPPORTED),
             (dict(good, flags=capi.IPT_FLAG_GUI_PLANE | capi.IPT_FLAG_PREVIEW), capi.IPT_E_UNSUPPORTED)]
    tp, tc, tm = _t(pixels), _t(counters), _t(m2)
    tmask = torch.full((W * H,), 0x55, dtype=torch.uint8, device=DEV)
    tstats = torch.full((4,), 0x55555555, dtype=torch.int32, device=DEV)
    ptrs = [tp.data_ptr(), tc.data_ptr(), tm.data_ptr(), tmask.data_ptr(), tstats.data_ptr()]
    for kw, code in cases:
        with pytest.raises(capi.IptError) as e:
            gpu_ctx.adapt_device(capi.make_adapt_params(W, H, **kw), *ptrs)
        assert e.value.code == code, kw
    ap = capi.make_adapt_params(W, H, **good)
    for hole in range(4):  # a NULL that is not optional
        with pytest.raises(capi.IptError) as e:
            gpu_ctx.adapt_device(ap, *[None if i == hole else q for i, q in enumerate(ptrs)])
        assert e.value.code == capi.IPT_E_INVALID
    for w, h in ((0, H), (W, -1)):
        with pytest.raises(capi.IptError) as e:
            gpu_ctx.adapt_device(capi.make_adapt_params(w, h, **good), *ptrs)
        assert e.value.code == capi.IPT_E_INVALID
    with pytest.raises(capi.IptError) as e:  # the mask inside an input
        gpu_ctx.adapt_device(ap, ptrs[0], ptrs[1], ptrs[2], ptrs[2] + 4, ptrs[4])
    assert e.value.code == capi.IPT_E_INVALID
    gpu_ctx.wait()
    torch.cuda.synchronize()
    assert (_h(tmask) == 0x55).all() and (_h(tstats) == 0x55555555).all()
    assert np.array_equal(bits(_h(tm)), bits(m2))


# ---- the loop ----------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", ac.LOOP_FRAMES, ids=lambda f: "%dx%d" % f)
def test_loop_device_resident(gpu_ctx, oracle, frame, plane):
    """render_masked -> adapt, ten rounds queued on one stream with no host
    wait in between (each round's state is cloned on the stream), against the
    numpy loop round for round: plane, m2, mask, stats."""
    W, H = frame
    _box(gpu_ctx)
    v, c = _samples(W, H, ac.LOOP_SPP, plane)
    rounds, used = ac.loop(v, c, plane, ac.LOOP_ROUND, **ac.LOOP_ADAPT)
    assert used == ac.LOOP_SPP
    ap = capi.make_adapt_params(W, H, flags=ac.FLAG[plane], **ac.LOOP_ADAPT)
    s = torch.cuda.Stream(DEV)
    t, tm2 = _to_device(dc.plane(W, H)), _t(np.zeros(W * H, np.float32))
    tmask = torch.zeros(W * H, dtype=torch.uint8, device=DEV)
    tstats = torch.zeros(4, dtype=torch.int32, device=DEV)
    snaps = []
    with torch.cuda.stream(s):
        for r in range(len(rounds)):
            gpu_ctx.render_masked_device_async(
                _params(W, H, ac.LOOP_ROUND, plane, spp_offset=r * ac.LOOP_ROUND), *_ptrs(t),
                mask_ptr=tmask.data_ptr() if r else None, m2_ptr=tm2.data_ptr(), stream=s.cuda_stream)
            gpu_ctx.adapt_device(ap, t["pixels"].data_ptr(), t["counters"].data_ptr(), tm2.data_ptr(),
                                 tmask.data_ptr(), tstats.data_ptr(), s.cuda_stream)
            snaps.append(({k: x.clone() for k, x in t.items()}, tm2.clone(), tmask.clone(), tstats.clone()))
    s.synchronize()
    gpu_ctx.wait()
    for r, ((img, m2, mask, stats), (gi, gm2, gmask, gstats)) in enumerate(zip(rounds, snaps)):
        _assert_plane_equal(_to_host(gi), img, what="round %d" % r)
        _assert_bits(_h(gm2), m2, "m2, round %d" % r)
        assert np.array_equal(_h(gmask), mask), r
        assert _h(gstats).tolist() == stats.tolist(), r


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", ac.LOOP_FRAMES, ids=lambda f: "%dx%d" % f)
def test_render_adaptive(gpu_ctx, oracle, frame, plane):
    """ipt_render_adaptive with a cap of 4k passes ends where the numpy loop's
    round k does (plane, m2, mask, stats, passes used); with a tolerance that
    everything meets it stops after the first round past min_count."""
    W, H = frame
    _box(gpu_ctx)
    v, c = _samples(W, H, ac.LOOP_SPP, plane)
    rounds, _ = ac.loop(v, c, plane, ac.LOOP_ROUND, **ac.LOOP_ADAPT)
    ap = capi.make_adapt_params(W, H, flags=ac.FLAG[plane], **ac.LOOP_ADAPT)
    for k, (img, m2, mask, stats) in enumerate(rounds, 1):
        got, gm2, gmask = dc.plane(W, H), np.zeros(W * H, np.float32), np.zeros(W * H, np.uint8)
        st = gpu_ctx.render_adaptive(_params(W, H, k * ac.LOOP_ROUND, plane), ap, ac.LOOP_ROUND, got, gm2, gmask)
        _assert_plane_equal(got, img, what="cap %d passes" % (4 * k))
        _assert_bits(gm2, m2, "m2")
        assert np.array_equal(gmask, mask)
        assert [st["active"], st["starved"], st["nan"], st["passes"]] == stats.tolist()[:3] + [k * ac.LOOP_ROUND]
    loose = dict(ac.LOOP_ADAPT, rel_tol=1e9)
    ref, used = ac.loop(v, c, plane, ac.LOOP_ROUND, **loose)
    assert used == 8 and ref[-1][3][0] == 0
    got = {k: x for k, x in dc.plane(W, H).items() if k in BARE}
    st = gpu_ctx.render_adaptive(_params(W, H, ac.LOOP_SPP, plane), capi.make_adapt_params(W, H, flags=ac.FLAG[plane], **loose),
                                 ac.LOOP_ROUND, got)
    assert st == {"active": 0, "starved": 0, "nan": 0, "passes": 8}
    _assert_plane_equal(got, ref[-1][0], BARE, what="early stop, no sums / pixel_max / m2 / mask")
    with pytest.raises(capi.IptError) as e:
        gpu_ctx.render_adaptive(_params(W, H, 8, plane, tile_rows=1, n_shards=2), ap, 4, dc.plane(W, H))
    assert e.value.code == capi.IPT_E_UNSUPPORTED
    with pytest.raises(capi.IptError) as e:
        gpu_ctx.render_adaptive(_params(W, H, 8, plane), ap, 0, dc.plane(W, H))
    assert e.value.code == capi.IPT_E_INVALID
