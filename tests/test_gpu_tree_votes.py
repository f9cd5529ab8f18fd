"""The tree shape as a parameter of the fixed box instances (path_kernel's
FIXED = K): a launch whose n_rays is 2^K for the compiled K
(4: n_rays 16) and whose depth_max exceeds K + 1 takes an instance that reads
neither n_rays, meta_shift nor depth_max in its step; every other launch takes
the instance it took before (select_path4, ipt_select.h).

Each case compares, as tests/test_gpu_box_range_instances.py does, the product
instance's samples and drift codes bit for bit with the oracle's, the counting
instance's samples with both, and the ten event counters with the oracle's, on
64 x 48 frames at 2 spp: sample_scenes[0] from its own camera and from the far
camera, the 16-light list (not a fixed instance: it must be unchanged) and a
25-light lattice.

  tree      n_rays 16 at depth_max 8 and 6: the FIXED = K instance;
  fallback  n_rays 16 at depth_max 5, 4 and 1: depth_max <= K + 1, so the depth
            cut is live and the launch must take the power-of-two instance
            (the oracle's traced rays fall with depth_max: asserted);
  other K   n_rays 8 and 32 at depth_max 8: powers of two that are not the
            compiled K (32 runs the 8-level instances);
  not fixed n_rays 12 (no power of two) and 1 (K = 0) at depth_max 8;
  wide      n_rays 256 (meta_shift 16) at depth_max 2, sample_scenes[0] only.
            (At depth_max 10 a 256-ray tree has about 1e11 iterations per
            path: neither the oracle nor one lane finishes a single path, so
            the wide meta word is exercised at the depth existing tests use,
            tests/test_gpu_deep_trees.py.)
  generic   the forced-generic instances (IPT_BOX_GENERIC=1) once.

No vote of the step was rewritten (none of the two that were
built cleared the A/B), so there is no rare-branch case of a new vote here.
"""
import functools

import numpy as np
import pytest

import oracle_binding as ob
from ipt_amd import capi, scenes

pytestmark = pytest.mark.gpu

TEN = ("paths", "traced_rays", "surface_hits", "light_hits", "expanded_nodes",
       "iterations", "light_samples", "skipped", "light_traces", "drifted")
W, H, SPP = 64, 48, 2
SCENES = ("default", "far", "lights16", "lights25")
TREE = [(16, 8), (16, 6)]
FALLBACK = [(16, 5), (16, 4), (16, 1)]
OTHER_K = [(8, 8), (32, 8)]
NOT_FIXED = [(12, 8), (1, 8)]


@functools.lru_cache(maxsize=None)
def _scene_cached(name):
    if name == "lights16":
        return scenes.make_scene_box_lights(4)
    if name == "lights25":
        return scenes.make_scene_box_lights(5)
    desc = scenes.make_scene_box()
    if name == "far":
        pos = np.asarray((3.0, -6.0, 2.5), np.float32)
        desc["camera"] = scenes.simple_camera(pos, scenes.normalize(-pos))
    return desc


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle(name, n_rays, depth_max):
    """Oracle samples, codes and counters of a whole frame, computed once per case."""
    p = capi.make_params(W, H, SPP, n_rays=n_rays, depth_max=depth_max)
    ov, oc, o = ob.render_values(_scene_cached(name), p, 0, with_counters=True)
    ov.setflags(write=False)
    oc.setflags(write=False)
    return ov, oc, o


def _check(ctx, name, n_rays, depth_max):
    kw = dict(n_rays=n_rays, depth_max=depth_max)
    ctx.upload_scene(_scene_cached(name))
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
    return o


@pytest.mark.parametrize("n_rays,depth_max", TREE)
@pytest.mark.parametrize("name", SCENES)
def test_tree_shape_instance_matches_oracle(gpu_ctx, oracle, name, n_rays, depth_max):
    """depth_max > K + 1: no ray is cut, so depth_max 8 and 6 render the same tree."""
    o = _check(gpu_ctx, name, n_rays, depth_max)
    assert o["surface_hits"] > 0 and o["expanded_nodes"] > 0
    assert o["traced_rays"] == _oracle(name, 16, 8)[2]["traced_rays"]


@pytest.mark.parametrize("n_rays,depth_max", FALLBACK)
@pytest.mark.parametrize("name", SCENES)
def test_depth_cut_falls_back_and_still_cuts(gpu_ctx, oracle, name, n_rays, depth_max):
    """depth_max <= K + 1: rays at depth_max are not traced (fewer traced rays
    than the uncut tree), which the tree-shape instance could not render."""
    o = _check(gpu_ctx, name, n_rays, depth_max)
    assert o["traced_rays"] < _oracle(name, 16, 8)[2]["traced_rays"]


@pytest.mark.parametrize("n_rays,depth_max", OTHER_K + NOT_FIXED)
@pytest.mark.parametrize("name", SCENES)
def test_other_tree_shapes_match_oracle(gpu_ctx, oracle, name, n_rays, depth_max):
    o = _check(gpu_ctx, name, n_rays, depth_max)
    assert o["surface_hits"] > 0 and o["iterations"] > 0


def test_wide_meta_word_matches_oracle(gpu_ctx, oracle):
    """n_rays 256: a power of two with meta_shift 16 (the compiled K has 8)."""
    o = _check(gpu_ctx, "default", 256, 2)
    assert o["expanded_nodes"] > 0


def test_forced_generic_instance_matches_oracle(oracle):
    """IPT_BOX_GENERIC=1 (read at creation): the generic instance, whatever the tree."""
    mp = pytest.MonkeyPatch()
    mp.setenv("IPT_BOX_GENERIC", "1")
    try:
        ctx = capi.Context(0)
    finally:
        mp.undo()
    try:
        _check(ctx, "default", 16, 8)
    finally:
        ctx.close()
