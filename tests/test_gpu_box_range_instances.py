"""The box planes' range form as a parameter of the path kernel's box instances
(path_kernel's BOXIN): the in-range instance holds the
in-range trace alone, the generic instance the generic full-form trace alone,
and the launch picks one from the scene (box_inrange, set at upload) or from
IPT_BOX_GENERIC=1 in the environment of the context's creation. The
axis-aligned single light's in-range instance exists twice more (FIXED): with
the pop's power-of-two unwind and the skip-ahead's guard fixed, taken by
launches whose n_rays is a power of two and whose light has a skip-ahead
plane, and without, taken by the others.

Each case compares, as tests/test_gpu_box_planes.py does, the product
instance's samples and drift codes bit for bit with the oracle's, the counting
instance's samples with both, and the ten event counters with the oracle's.

  in range   the session's context: sample_scenes[0] with its own camera and
             with the far camera (the full form behind the nearest form's
             vote), the 16-light scene (a light list in LDS) and a 25-light
             lattice (the lattice instance, which keeps the full form);
  forced     a context created under IPT_BOX_GENERIC=1 renders the same
             scenes: the only way the generic forms run on rays that hit;
  selected   the camera at (0, -2^40, 0) looking along +y puts the scene out
             of range: every camera ray leaves the planes' t at infinity (the
             oracle: 8 192 paths, 8 192 traced rays, no surface hit, every
             sample 0), and the launch takes the generic instance by itself;
  trees      n_rays 12 at depth_max 4 is no power of two: the launch takes the
             instance that is not FIXED, on its dividing unwind; n_rays 1, the
             smallest power of two, takes the FIXED one with the smallest tree;
  no plane   a single axis-aligned light with P.z = 0 has no skip-ahead plane
             (|P.z| < 2^-32): the instance that is not FIXED, its guard false.
"""
import functools

import numpy as np
import pytest

import oracle_binding as ob
from ipt_amd import capi, scenes

pytestmark = pytest.mark.gpu

TEN = ("paths", "traced_rays", "surface_hits", "light_hits", "expanded_nodes",
       "iterations", "light_samples", "skipped", "light_traces", "drifted")

# name -> (width, height, spp)
CASES = {"default": (64, 64, 2), "far": (64, 64, 2), "lights16": (64, 64, 1), "lights25": (64, 64, 1)}


def _cam(pos, look_at=None, direction=None):
    pos = np.asarray(pos, np.float32)
    if direction is None:
        direction = np.asarray(look_at, np.float32) - pos
    return scenes.simple_camera(pos, scenes.normalize(np.asarray(direction, np.float32)))


def _scene(name):
    if name == "lights16":
        return scenes.make_scene_box_lights(4)
    if name == "lights25":
        return scenes.make_scene_box_lights(5)  # more than the LDS light list holds: the lattice instance
    desc = scenes.make_scene_box()
    if name == "far":
        desc["camera"] = _cam((3.0, -6.0, 2.5), look_at=(0.0, 0.0, 0.0))
    elif name == "pz0":
        desc["lights"] = [scenes.square_light((np.float32(0.1), np.float32(-0.9), np.float32(0.0)),
                                              (0.0, 0.0, -1.0), (0.0, 0.2, 0.0), 1.0)]
    elif name == "beyond":
        desc["camera"] = _cam((0.0, -(2.0 ** 40), 0.0), direction=(0.0, 1.0, 0.0))
    return desc


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle(name, w, h, spp, n_rays=16, depth_max=8):
    """Oracle samples, codes and counters of a whole frame, computed once per case."""
    kw = dict(n_rays=n_rays, depth_max=depth_max)
    ov, oc, o = ob.render_values(_scene(name), capi.make_params(w, h, spp, **kw), 0, with_counters=True)
    ov.setflags(write=False)
    oc.setflags(write=False)
    return ov, oc, o


def _check(ctx, name, w, h, spp, n_rays=16, depth_max=8):
    kw = dict(n_rays=n_rays, depth_max=depth_max)
    ctx.upload_scene(_scene(name))
    pv, pc = ctx.render_values(capi.make_params(w, h, spp, **kw))
    ctx.reset_counters()
    cv, cc = ctx.render_values(capi.make_params(w, h, spp, flags=capi.IPT_FLAG_COUNTERS, **kw))
    g = ctx.counters()
    ov, oc, o = _oracle(name, w, h, spp, n_rays, depth_max)
    assert np.array_equal(pc, oc), "product drift codes differ from the oracle"
    assert np.array_equal(_bits(pv), _bits(ov)), (
        f"product: {int((_bits(pv) != _bits(ov)).sum())} of {pv.size} samples differ from the oracle")
    assert np.array_equal(cc, oc), "counting-instance drift codes differ"
    assert np.array_equal(_bits(cv), _bits(ov)), (
        f"counting instance: {int((_bits(cv) != _bits(ov)).sum())} of {pv.size} samples differ from the oracle")
    for k in TEN:
        assert g[k] == o[k], (name, k, g[k], o[k])
    return ov, o


@pytest.fixture(scope="module")
def generic_ctx():
    """A context created under IPT_BOX_GENERIC=1 (read once, at creation)."""
    mp = pytest.MonkeyPatch()
    mp.setenv("IPT_BOX_GENERIC", "1")
    try:
        ctx = capi.Context(0)
    finally:
        mp.undo()
    yield ctx
    ctx.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_in_range_instance_matches_oracle(gpu_ctx, oracle, name):
    _, o = _check(gpu_ctx, name, *CASES[name])
    assert o["surface_hits"] > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_forced_generic_instance_matches_oracle(generic_ctx, oracle, name):
    """The generic instance on rays that hit: the same scenes, the same bits."""
    _, o = _check(generic_ctx, name, *CASES[name])
    assert o["surface_hits"] > 0


def test_override_is_read_at_creation(monkeypatch, oracle):
    """monkeypatch.setenv before capi.Context, as a caller would set it."""
    monkeypatch.setenv("IPT_BOX_GENERIC", "1")
    ctx = capi.Context(0)
    monkeypatch.delenv("IPT_BOX_GENERIC")
    try:
        _check(ctx, "default", *CASES["default"])
    finally:
        ctx.close()


def test_scene_beyond_range_takes_the_generic_instance(gpu_ctx, oracle):
    """Camera at (0, -2^40, 0) looking along +y: out of range, so the launch
    takes the generic instance without the override. No ray reaches a plane."""
    ov, o = _check(gpu_ctx, "beyond", 64, 64, 2)
    assert o["paths"] == 8192 and o["traced_rays"] == 8192 and o["surface_hits"] == 0
    assert not _bits(ov).any()


@pytest.mark.parametrize("n_rays", [12, 1])
def test_other_tree_shapes_match_oracle(gpu_ctx, oracle, n_rays):
    """n_rays 12: the instance whose unwind chooses its form per step, on its
    dividing form; n_rays 1: the FIXED instance, one child per node."""
    _, o = _check(gpu_ctx, "default", 32, 32, 2, n_rays=n_rays, depth_max=4)
    assert o["surface_hits"] > 0 and o["iterations"] > 0


def test_light_without_skip_ahead_plane_matches_oracle(gpu_ctx, oracle):
    """P.z = 0: the host finds no skip-ahead plane, so the launch takes the
    instance that reads the guard."""
    _, o = _check(gpu_ctx, "pz0", 32, 32, 2)
    assert o["light_samples"] > 0 and o["surface_hits"] > 0
