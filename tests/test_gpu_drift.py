"""accumulate_kernel's drift branch against the oracle, on frames that reach it.

A jittered sample whose (float)(i + u) rounds across an integer lands one
pixel off its nominal destination; new_path_setup flags both pixels and the
replay serves them by its second branch: up to four candidate source rows,
three columns, nine codes, the 0xfe halo samples of other shards skipped, the
rays added in render_sample's raster order so that the running mean comes out
bit-identical. The rate is about i * 2^-24 per sample, so no frame of the
other fast tests holds a drifted sample. The frames here (tests/drift_cases.py)
are 60000 and 65536 pixels long and two or three wide: hundreds of drifted
samples per pass, along x (dx = -1 and +1) and along y (dy = -1 and +1), at
the rows where the nominal mapping folds (source rows H-2 and H-1 into row 0,
row H-1 fed by drift alone), cut by one-row shard tiles, replayed into
preloaded planes, and in the 2048^2 passes that hold the one diagonal code the
default seed produces. tests/test_drift_cpu.py pins, without a GPU, that the
frames hold what this file relies on.

Everything is compared bit for bit with ob.render_values (samples, codes,
counters) and ob.accumulate (the plane)."""
import numpy as np
import pytest
import torch

import drift_cases as dc
import oracle_binding as ob
from ipt_amd import capi, scenes

pytestmark = pytest.mark.gpu

bits = dc.bits
KEYS = tuple(k for k, _ in dc.PLANE_KEYS)


def _frame_id(v):
    return "%dx%d" % v if isinstance(v, tuple) else str(v)


def _assert_plane_equal(img, ref, keys=KEYS, what=""):
    for k in keys:
        bad = bits(img[k]) != bits(ref[k])
        assert not bad.any(), (what, k, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())


def _box(ctx):
    desc = scenes.make_scene_box()
    ctx.upload_scene(desc)
    return desc


def _check_frame(ctx, W, H, spp, count, **tree):
    """Samples, codes, plane (and the drifted counter of the counting
    instance) of one whole-frame render against the oracle."""
    _box(ctx)
    ov, oc, ocnt = dc.oracle_samples(W, H, spp, **tree)
    p = dc.params(W, H, spp, flags=capi.IPT_FLAG_COUNTERS if count else 0, **tree)
    gv, gc = ctx.render_values(p)
    assert np.array_equal(gc, oc), int((gc != oc).sum())
    assert np.array_equal(bits(gv), bits(ov)), int((bits(gv) != bits(ov)).sum())
    img = dc.plane(W, H)
    ctx.reset_counters()
    ctx.render(p, img)
    _assert_plane_equal(img, dc.oracle_plane(W, H, spp, **tree))
    if count:
        assert ctx.counters()["drifted"] == ocnt["drifted"] > 0
    return gv, gc


@pytest.mark.parametrize("spp", dc.SPPS)
@pytest.mark.parametrize("frame", dc.FRAMES, ids=_frame_id)
def test_drift_frames_bit_exact(gpu_ctx, oracle, frame, spp):
    """Nine passes go through the unrolled eight and the remainder of the
    nominal branch beside the drift branch, with the counting instance."""
    _check_frame(gpu_ctx, *frame, spp, count=spp == 9)


def test_max_height_frame_bit_exact(gpu_ctx, oracle):
    """H = 65536, validate()'s limit: the one frame with as many rows as the
    replay's launch can be asked for."""
    _check_frame(gpu_ctx, *dc.MAX_HEIGHT, 2, count=True)


def _to_device(img, dev, keys=KEYS):
    return {k: torch.from_numpy(img[k].view(np.int32) if k == "counters" else img[k]).to(dev) for k in keys}


def _render_device(ctx, p, t):
    ctx.render_device(p, t["pixels"].data_ptr(), t["counters"].data_ptr(),
                      t["sums"].data_ptr() if "sums" in t else None,
                      t["pixel_max"].data_ptr() if "pixel_max" in t else None)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if k == "counters" else v.cpu().numpy()) for k, v in t.items()}


@pytest.mark.parametrize("spp", dc.SPPS)
@pytest.mark.parametrize("frame", [dc.WIDE, dc.TALL], ids=_frame_id)
def test_drift_frames_render_device(gpu_ctx, oracle, frame, spp):
    """The same planes through ipt_render_device on torch tensors."""
    _box(gpu_ctx)
    dev = torch.device("cuda", 0)
    got = _render_device(gpu_ctx, dc.params(*frame, spp), _to_device(dc.plane(*frame), dev))
    _assert_plane_equal(got, dc.oracle_plane(*frame, spp))


@pytest.mark.parametrize("case", dc.DIAGONAL, ids=lambda c: "%#x-pass%d" % (c[0], c[3]))
def test_diagonal_drift_bit_exact(gpu_ctx, oracle, case):
    """dx = dy = +1 (0xa) and dx = -1, dy = +1 (0x8): one sample of a whole
    square pass each, with radiance."""
    code, n, seed, off, ix, iy, n_rays, depth_max, value = case
    gv, gc = _check_frame(gpu_ctx, n, n, 1, count=False, spp_offset=off, n_rays=n_rays, depth_max=depth_max,
                          seed=seed)
    assert gc[0, iy, ix] == code and float(gv[0, iy, ix]) == value


# ---- drift across shard boundaries -----------------------------------------
def _render_shards(ctx, frame, tile, n_shards, spp):
    """Every shard of the plan into a plane of its own; returns the assembled
    plane after checking that no shard wrote outside ipt_shard_plan's rows."""
    W, H = frame
    out = dc.plane(W, H)
    covered = np.zeros(H, np.int32)
    for s in range(n_shards):
        part = dc.plane(W, H)
        p = dc.params(W, H, spp, tile_rows=tile, n_shards=n_shards, shard_id=s)
        owned, _ = capi.shard_plan(p)
        covered += owned
        ctx.render(p, part)
        mask = np.repeat(owned, W)
        for k in KEYS:
            assert not part[k][~mask].any(), f"shard {s} wrote outside its rows"
            out[k][mask] = part[k][mask]
    assert (covered == 1).all()
    return out


@pytest.mark.parametrize("frame,tile,n_shards", [(f, t, n) for f, plans in dc.SHARD_PLANS.items() for t, n in plans],
                         ids=_frame_id)
def test_sharded_drift_bit_exact(gpu_ctx, oracle, frame, tile, n_shards):
    """A drifted sample whose destination row is another shard's is a 0xfe
    halo sample for the owner of its nominal row and a candidate-row sample
    for the owner of its destination; assembled, the shards' planes are the
    oracle's whole frame."""
    _box(gpu_ctx)
    spp = dc.SHARD_SPP[frame]
    got = _render_shards(gpu_ctx, frame, tile, n_shards, spp)
    _assert_plane_equal(got, dc.oracle_plane(*frame, spp))


def test_sharded_drift_chunked(oracle, monkeypatch):
    """One pass per launch: the drift flags are rebuilt by every launch, so
    each chunk's replay stands on its own."""
    monkeypatch.setenv("IPT_TEST_CHUNK_UNITS", "1")
    ctx = capi.Context(0)
    try:
        _box(ctx)
        got = _render_shards(ctx, dc.TALL, 1, 3, 4)
        _assert_plane_equal(got, dc.oracle_plane(*dc.TALL, 4))
    finally:
        ctx.close()


def test_sharded_drift_resident_host_plane(oracle):
    """Three contexts, one host plane, two progressive calls each: the rows a
    context keeps on its device between the calls, and the rows its neighbours
    wrote in between, add up to the oracle's four passes."""
    ctxs = [capi.Context(0) for _ in range(3)]
    try:
        for c in ctxs:
            _box(c)
        W, H = dc.TALL
        img = dc.plane(W, H)
        for off in (0, 2):
            for s, c in enumerate(ctxs):
                c.render(dc.params(W, H, 2, spp_offset=off, tile_rows=1, n_shards=3, shard_id=s), img)
        _assert_plane_equal(img, dc.oracle_plane(W, H, 4))
    finally:
        for c in ctxs:
            c.close()


# ---- replay into a preloaded plane -------------------------------------------
def _check_preloaded(ctx, frame, spp, hot_from_drift):
    W, H = frame
    _box(ctx)
    ov, oc, _ = dc.oracle_samples(W, H, spp)
    hot = None
    if hot_from_drift:
        _, yi, xi = dc.destinations(oc)
        d = oc != 0x05
        hot = yi[d] * W + xi[d]
    pre, _ = dc.preload(W, H, spp, hot)
    ref = ob.accumulate(ov, oc, img=dc.copy_plane(pre))
    p = dc.params(W, H, spp)
    img = dc.copy_plane(pre)
    ctx.render(p, img)
    _assert_plane_equal(img, ref, what="ipt_render")
    dev = torch.device("cuda", 0)
    _assert_plane_equal(_render_device(ctx, p, _to_device(pre, dev)), ref, what="ipt_render_device")
    # sums and pixel_max are optional: without either, the rest is the same
    for keys in (("pixels", "counters", "pixel_max"), ("pixels", "counters", "sums"), ("pixels", "counters")):
        got = _render_device(ctx, p, _to_device(pre, dev, keys))
        _assert_plane_equal(got, ref, keys, what="ipt_render_device " + "+".join(keys))
    return pre, ref


@pytest.mark.parametrize("spp", dc.SPPS)
def test_preloaded_wide_plane_bit_exact(gpu_ctx, oracle, spp):
    """add_ray on existing state -- counters around 2^24 and 2^31 and up to
    the last value that cannot wrap, negative, -0.0, subnormal, infinite and
    NaN pixels, pixel_max below, above and NaN, infinite sums -- with every
    kind on drifted destination pixels."""
    pre, ref = _check_preloaded(gpu_ctx, dc.WIDE, spp, hot_from_drift=True)
    assert (bits(ref["pixels"]) != bits(pre["pixels"])).any()


@pytest.mark.parametrize("spp", dc.SMALL_SPPS)
def test_preloaded_small_plane_bit_exact(gpu_ctx, oracle, spp):
    """The nominal branch's unrolled eight passes and its remainder (7, 8, 9,
    16, 17 passes) on the same kinds of existing state."""
    _check_preloaded(gpu_ctx, dc.SMALL, spp, hot_from_drift=False)
