"""The box planes' nearest-candidate form (ipt_path.h
trace_box_planes_nearest) and the hit point the box trace hands to resolve, in
the path kernel, against the oracle. The host half
(tests/test_box_planes_host.py) compares the function itself with the full
form on 2 x 20 M rays; here the callers of the box planes run inside their
steps: the box instance (sample_scenes[0]) with the nearest-candidate form and
the hit point handed to resolve, and the lattice-light and sphere-list
instances, which go through the same trace_geometry and keep the full form
(DESIGN.md 4.10).

Each case compares, as tests/test_gpu_step_unwind.py does, the product
instance's samples and drift codes bit for bit with the oracle's, the counting
instance's samples with both, and the ten event counters with the oracle's.

Cameras of the box scene (64x64, 2 spp, n_rays 16, depth 8):
  default   sample_scenes[0]'s own, outside the open (-y) side;
  inside    in the box, between the sphere and the open side: no camera ray
            crosses a plane's extension;
  far       far outside and off axis: much of the frame misses the box, and
            those camera rays' nearest candidate plane is crossed outside its
            bounds while the failing coordinate still moves inwards -- the
            full form runs behind its vote in waves whose other lanes iterate;
  diagonal  at (0.4, 0.4, -0.4) aimed along the box diagonal at the corner
            (1, 1, -1): the three facing planes' t nearly tie around the
            frame's centre;
  edge      next to the edge x = 1, z = -1, aimed along it: two planes nearly
            tie over the frame and many hit points lie within rounding of a
            bound.
"""
import functools

import numpy as np
import pytest

import oracle_binding as ob
from ipt_amd import capi, scenes

pytestmark = pytest.mark.gpu

TEN = ("paths", "traced_rays", "surface_hits", "light_hits", "expanded_nodes",
       "iterations", "light_samples", "skipped", "light_traces", "drifted")


def _cam(pos, look_at=None, direction=None):
    pos = np.asarray(pos, np.float32)
    if direction is None:
        direction = np.asarray(look_at, np.float32) - pos
    return scenes.simple_camera(pos, scenes.normalize(np.asarray(direction, np.float32)))


CAMERAS = {
    "default": None,
    "inside": lambda: _cam((0.0, -0.8, 0.3), look_at=(0.0, 1.0, -1.0)),
    "far": lambda: _cam((3.0, -6.0, 2.5), look_at=(0.0, 0.0, 0.0)),
    "diagonal": lambda: _cam((0.4, 0.4, -0.4), direction=(1.0, 1.0, -1.0)),
    "edge": lambda: _cam((0.95, -0.9, -0.95), direction=(0.0, 1.0, 0.0)),
}


def _scene(name):
    if name == "lights16":
        return scenes.make_scene_box_lights(4)  # 16 lights: the lattice instance
    if name == "spheres50":
        return scenes.make_scene_spheres(50, seed=3)
    desc = scenes.make_scene_box()
    if CAMERAS[name] is not None:
        desc["camera"] = CAMERAS[name]()
    return desc


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle(name, w, h, spp):
    """Oracle samples, codes and counters of a whole frame, computed once per case."""
    p = capi.make_params(w, h, spp, n_rays=16, depth_max=8)
    ov, oc, o = ob.render_values(_scene(name), p, 0, with_counters=True)
    ov.setflags(write=False)
    oc.setflags(write=False)
    return ov, oc, o


def _check(ctx, name, w, h, spp):
    ctx.upload_scene(_scene(name))
    kw = dict(n_rays=16, depth_max=8)
    pv, pc = ctx.render_values(capi.make_params(w, h, spp, **kw))
    ctx.reset_counters()
    cv, cc = ctx.render_values(capi.make_params(w, h, spp, flags=capi.IPT_FLAG_COUNTERS, **kw))
    g = ctx.counters()
    ov, oc, o = _oracle(name, w, h, spp)
    assert np.array_equal(pc, oc), "product drift codes differ from the oracle"
    assert np.array_equal(_bits(pv), _bits(ov)), (
        f"product: {int((_bits(pv) != _bits(ov)).sum())} of {pv.size} samples differ from the oracle")
    assert np.array_equal(cc, oc), "counting-instance drift codes differ"
    assert np.array_equal(_bits(cv), _bits(ov)), (
        f"counting instance: {int((_bits(cv) != _bits(ov)).sum())} of {pv.size} samples differ from the oracle")
    for k in TEN:
        assert g[k] == o[k], (name, k, g[k], o[k])
    return o


@pytest.mark.parametrize("camera", sorted(CAMERAS))
def test_box_matches_oracle(gpu_ctx, oracle, camera):
    _check(gpu_ctx, camera, 64, 64, 2)


def test_lattice_lights_match_oracle(gpu_ctx, oracle):
    """The 16-light lattice at 64x64: the lattice instance's box trace."""
    _check(gpu_ctx, "lights16", 64, 64, 2)


def test_sphere_list_matches_oracle(gpu_ctx, oracle):
    """50 listed spheres at 32x32: the sphere-list instances' walls."""
    _check(gpu_ctx, "spheres50", 32, 32, 2)


def test_two_shard_call_matches_oracle(gpu_ctx, oracle):
    """The default frame rendered as two shards (tile_rows 8): both shards'
    rows together are the oracle's whole-frame plane, from the product and
    from the counting instance."""
    w = h = 64
    gpu_ctx.upload_scene(_scene("default"))
    ov, oc, _ = _oracle("default", w, h, 2)
    ref = ob.accumulate(ov, oc)
    seen = np.zeros(w * h, bool)
    for shard in (0, 1):
        kw = dict(n_rays=16, depth_max=8, tile_rows=8, n_shards=2, shard_id=shard)
        p = capi.make_params(w, h, 2, **kw)
        owned, _ = capi.shard_plan(p)
        assert owned.any() and not owned.all()
        mask = np.repeat(owned, w)
        planes = []
        for flags in (0, capi.IPT_FLAG_COUNTERS):
            img = {k: np.zeros(w * h, dt) for k, dt in (("pixels", np.float32), ("counters", np.uint32),
                                                        ("sums", np.float32), ("pixel_max", np.float32))}
            gpu_ctx.render(capi.make_params(w, h, 2, flags=flags, **kw), img)
            planes.append(img)
        for k in planes[0]:
            assert not planes[0][k][~mask].any(), "shard wrote outside its rows"
            assert np.array_equal(_bits(planes[0][k])[mask], _bits(ref[k])[mask]), ("product", shard, k)
            assert np.array_equal(_bits(planes[1][k]), _bits(planes[0][k])), ("counting instance", shard, k)
        assert not (seen & mask).any()
        seen |= mask
    assert seen.all()
