"""The leaf rule of the product FIXED = K box instances: a
child pushed at depth K (one iteration, a childless ray) strictly behind the
lights' plane is worth exactly +0 whatever it draws, so the end-of-step
pre-skip takes its iteration whatever its pick word says (three draws, or one
for the fall-through) and the step's pop unwinds it: the child costs no step
of its own. The counting instances run the iteration (the oracle counts its
events).

Each case compares the product instance's samples and drift codes bit for bit
with the oracle's, and the counting instance's samples and its ten counters
with the oracle's, on 64 x 48 frames at 2 spp (tests/test_gpu_tree_votes.py's
frame).

Scenes
  default, far   sample_scenes[0] from its own camera and from the far camera;
  flipped        the light's normal flipped to +z (same square): the other half
                 of the box is "behind";
  above, below   the light plane beyond every surface, at z = +1.5 and z = -1.5
                 with the normal -z: every node is in front (no leaf is ever
                 elided), every node is behind (every leaf in the window is);
  wall_hi/lo     the plane exactly on the walls z = +1 and z = -1, a z that hit
                 points take: the test is strict, o.z == P.z must push. (A light
                 on a wall fails the host's range proof, so these launches take
                 the generic single-light instance, whose skip-ahead and
                 pre-skip use the same strict test on the same plane.)
  lights64       the 64-light lattice, exactly uniform on the draw's integer
                 (cdf_p2): the lattice instances' leaf rule is live, the
                 pick word's class is pick_p2w's last test;
  lights25       the 25-light lattice, not uniform (pick_of): the lattice
                 instances with the leaf rule off;
  lights16       the 16-light list: no fixed instance, must stay bit-exact.

Tree shapes: n_rays 16 at depth_max 8 and 6 (the K instance), at 5 and 4
(depth_max <= K + 1: the launch falls back), n_rays 8 and 32 (kFixedPow2). The
plane-position scenes run the K shapes and one fallback.

Plumbing, sample_scenes[0] at n_rays 16, depth_max 8: a sharded plan with
one-row tiles, a chunked launch, two queued launches, a masked render.
"""
import functools

import numpy as np
import pytest

import adaptive_cases as ac
import oracle_binding as ob
from ipt_amd import capi, scenes

pytestmark = pytest.mark.gpu

TEN = ("paths", "traced_rays", "surface_hits", "light_hits", "expanded_nodes",
       "iterations", "light_samples", "skipped", "light_traces", "drifted")
W, H, SPP = 64, 48, 2
MAIN = ("default", "far", "flipped", "lights64", "lights25", "lights16")
PLANES = ("above", "below", "wall_hi", "wall_lo")
K_SHAPES = [(16, 8), (16, 6)]
FALLBACK = [(16, 5), (16, 4)]
POW2 = [(8, 8), (32, 8)]
PLANE_KEYS = (("pixels", np.float32), ("counters", np.uint32), ("sums", np.float32), ("pixel_max", np.float32))
f32 = np.float32


def _light(z, normal_z=-1.0):
    """sample_scenes[0]'s 0.2 x 0.2 square at height z; with normal +z the corner
    moves so that the square stays where it was."""
    cx, cy, _ = scenes.box_light_corner()
    if normal_z > 0:
        cx = f32(cx + f32(0.2))
    return scenes.square_light((cx, cy, f32(z)), (0.0, 0.0, normal_z), (0.0, 0.2, 0.0), 1.0)


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "lights16":
        return scenes.make_scene_box_lights(4)
    if name == "lights25":
        return scenes.make_scene_box_lights(5)
    if name == "lights64":
        return scenes.make_scene_box_lights(8)
    desc = scenes.make_scene_box()
    if name == "far":
        pos = np.asarray((3.0, -6.0, 2.5), np.float32)
        desc["camera"] = scenes.simple_camera(pos, scenes.normalize(-pos))
    elif name == "flipped":
        desc["lights"] = [_light(scenes.box_light_corner()[2], +1.0)]
    elif name in ("above", "below", "wall_hi", "wall_lo"):
        desc["lights"] = [_light({"above": 1.5, "below": -1.5, "wall_hi": 1.0, "wall_lo": -1.0}[name])]
    return desc


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle(name, n_rays=16, depth_max=8):
    """Oracle samples, codes and counters of a whole frame, computed once per case."""
    p = capi.make_params(W, H, SPP, n_rays=n_rays, depth_max=depth_max)
    ov, oc, o = ob.render_values(_scene(name), p, 0, with_counters=True)
    ov.setflags(write=False)
    oc.setflags(write=False)
    return ov, oc, o


def _check(ctx, name, n_rays, depth_max):
    kw = dict(n_rays=n_rays, depth_max=depth_max)
    ctx.upload_scene(_scene(name))
    pv, pc = ctx.render_values(capi.make_params(W, H, SPP, **kw))
    ctx.reset_counters()
    cv, cc = ctx.render_values(capi.make_params(W, H, SPP, flags=capi.IPT_FLAG_COUNTERS, **kw))
    g = ctx.counters()
    ov, oc, o = _oracle(name, n_rays, depth_max)
    assert np.array_equal(pc, oc), "product drift codes differ from the oracle"
    assert np.array_equal(_bits(pv), _bits(ov)), (
        f"product: {int((_bits(pv) != _bits(ov)).sum())} of {pv.size} samples differ from the oracle")
    assert np.array_equal(cc, oc), "counting-instance drift codes differ"
    assert np.array_equal(_bits(cv), _bits(ov)), (
        f"counting instance: {int((_bits(cv) != _bits(ov)).sum())} of {pv.size} samples differ from the oracle")
    for k in TEN:
        assert g[k] == o[k], (name, k, g[k], o[k])
    return ov, o


@pytest.mark.parametrize("n_rays,depth_max", K_SHAPES + FALLBACK + POW2)
@pytest.mark.parametrize("name", MAIN)
def test_scenes_and_tree_shapes_match_oracle(gpu_ctx, oracle, name, n_rays, depth_max):
    ov, o = _check(gpu_ctx, name, n_rays, depth_max)
    assert o["surface_hits"] > 0 and o["expanded_nodes"] > 0 and o["light_hits"] > 0
    assert _bits(ov).any()


@pytest.mark.parametrize("n_rays,depth_max", K_SHAPES + FALLBACK[:1])
@pytest.mark.parametrize("name", PLANES)
def test_plane_positions_match_oracle(gpu_ctx, oracle, name, n_rays, depth_max):
    ov, o = _check(gpu_ctx, name, n_rays, depth_max)
    assert o["surface_hits"] > 0 and o["expanded_nodes"] > 0
    if name == "below":
        # every node is behind the plane: every light pick is skipped, nothing is lit
        assert o["light_hits"] == 0 and o["skipped"] >= o["light_samples"] > 0 and not _bits(ov).any()
    if name == "above":
        # every node is in front of the plane: no light pick is skipped
        assert o["skipped"] == 0 and o["light_samples"] > 0


def test_lattice_without_cdf_p2_first_in_a_fresh_context(oracle):
    """The lattice instances compare every next pick word with cdf[nl]'s
    threshold (the fall-through class), also where the leaf rule is off: in a
    context that has seen no other scene the threshold must be this scene's
    (a pre-skipped light pick is three draws, not one)."""
    ctx = capi.Context(0)
    try:
        _, o = _check(ctx, "lights25", 16, 8)
        assert o["skipped"] > 0
    finally:
        ctx.close()


def _image():
    return {k: np.zeros(W * H, dt) for k, dt in PLANE_KEYS}


def _assert_same(a, b, sel=slice(None), what=""):
    for k, _ in PLANE_KEYS:
        assert np.array_equal(_bits(a[k])[sel], _bits(b[k])[sel]), (what, k)


@functools.lru_cache(maxsize=None)
def _plane():
    ov, oc, _ = _oracle("default")
    return ob.accumulate(ov, oc)


def test_sharded_plan_with_one_row_tiles(gpu_ctx, oracle):
    gpu_ctx.upload_scene(_scene("default"))
    seen = np.zeros(W * H, bool)
    for shard in range(3):
        p = capi.make_params(W, H, SPP, n_rays=16, depth_max=8, tile_rows=1, n_shards=3, shard_id=shard)
        owned, _ = capi.shard_plan(p)
        mask = np.repeat(owned, W)
        img = _image()
        gpu_ctx.render(p, img)
        for k in img:
            assert not img[k][~mask].any(), "shard wrote outside its rows"
        _assert_same(img, _plane(), mask, "shard %d" % shard)
        seen |= mask
    assert seen.all()


def test_chunked_launch(oracle, monkeypatch):
    """IPT_TEST_CHUNK_UNITS (read at creation) splits the call into launches of one pass."""
    monkeypatch.setenv("IPT_TEST_CHUNK_UNITS", "3000")
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(_scene("default"))
        p = capi.make_params(W, H, SPP, n_rays=16, depth_max=8)
        gv, gc = ctx.render_values(p)
        ov, oc, _ = _oracle("default")
        assert np.array_equal(gc, oc) and np.array_equal(_bits(gv), _bits(ov))
        img = _image()
        ctx.render(p, img)
        _assert_same(img, _plane(), what="chunked")
    finally:
        ctx.close()


def _device_plane():
    import torch

    return torch.zeros(4, H, W, dtype=torch.float32, device="cuda")


def _ptrs(st):
    return st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr()


def _host(st):
    import torch

    torch.cuda.synchronize()
    a = st.cpu().numpy()
    return {"pixels": a[0].reshape(-1), "counters": a[1].view(np.uint32).reshape(-1),
            "sums": a[2].reshape(-1), "pixel_max": a[3].reshape(-1)}


def test_two_queued_launches(gpu_ctx, oracle):
    """Two queued one-pass calls leave the oracle's two-pass plane."""
    import torch

    gpu_ctx.upload_scene(_scene("default"))
    q = _device_plane()
    stream = torch.cuda.current_stream().cuda_stream
    for c in range(SPP):
        gpu_ctx.render_device_async(capi.make_params(W, H, 1, spp_offset=c, n_rays=16, depth_max=8), *_ptrs(q), stream)
    gpu_ctx.wait()
    _assert_same(_host(q), _plane(), what="queued")


def test_masked_render(gpu_ctx, oracle):
    """The seeded half mask: the plane and the second moment of the masked replay of the oracle's samples."""
    import torch

    gpu_ctx.upload_scene(_scene("default"))
    ov, oc, _ = _oracle("default")
    mask = ac.half_mask(W, H)
    ref, rm2 = ac.replay(ov, oc, mask, ac.GRID)
    t = _device_plane()
    m2 = torch.zeros(W * H, dtype=torch.float32, device="cuda")
    tm = torch.from_numpy(np.ascontiguousarray(mask).reshape(-1).copy()).to("cuda")
    gpu_ctx.render_masked_device(capi.make_params(W, H, SPP, n_rays=16, depth_max=8), *_ptrs(t),
                                 mask_ptr=tm.data_ptr(), m2_ptr=m2.data_ptr())
    _assert_same(_host(t), ref, what="masked")
    assert np.array_equal(_bits(m2.cpu().numpy()), _bits(rm2))
