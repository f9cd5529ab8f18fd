"""The scene fact of the product FIXED = K box instances: no
draw word falls through the pick (cdf[nl] >= 1), checked per scene by the
host. With it the single-light and LDS-lattice product instances pick with one
32-bit compare, advance three draws per pre-skipped pick and select between
two directions. A scene without it takes kFixedPow2, the code as it was. (The
lattices with global records keep the general pick: test_gpu_instance_census's
box/a10big and box/a01big, whose weights leave fall-through words, render on
their FIXED = 4 instances bit for bit.)

Each case compares the product instance's samples and drift codes bit for bit
with the oracle's, the counting instance's samples and its ten counters with
the oracle's, and asserts the instance each launch took (ipt_last_instance:
MAXSUSP, COUNT, LMODE, GEOM, BOXIN, FIXED), on 64 x 48 frames at 2 spp
(tests/test_gpu_leaf_elide.py's frame). The scenes are fixed_facts_cases.py's;
tests/test_fixed_facts_host.py has the CPU half (the facts per scene, the
selector, and that the leaky frame meets a fall-through in the oracle).

Plumbing, sample_scenes[0] at n_rays 16, depth_max 8: a chunked launch, two
queued launches, a sharded plan with one-row tiles.
"""
import functools

import numpy as np
import pytest

import fixed_facts_cases as fc
import oracle_binding as ob
from ipt_amd import capi

pytestmark = pytest.mark.gpu

TEN = ("paths", "traced_rays", "surface_hits", "light_hits", "expanded_nodes",
       "iterations", "light_samples", "skipped", "light_traces", "drifted")
W, H, SPP = 64, 48, 2
SEED = 20241223
PLANE_KEYS = (("pixels", np.float32), ("counters", np.uint32), ("sums", np.float32), ("pixel_max", np.float32))
ONE_A10, LATTICE_LDS, LIST_LDS = 5, 9, 2  # kLightsOneA10, kLightsGridA10L, kLightsLds
TREE, POW2 = 4, -1                        # kTreeK, kFixedPow2

# (scene, n_rays, depth_max, RNG seed, LMODE, FIXED of the launch)
CASES = [
    ("default", 16, 8, SEED, ONE_A10, TREE),
    ("default", 16, 6, SEED, ONE_A10, TREE),
    ("default", 16, 5, SEED, ONE_A10, POW2),   # depth_max <= K + 1
    ("default", 8, 8, SEED, ONE_A10, POW2),
    ("default", 32, 8, SEED, ONE_A10, POW2),
    ("far", 16, 8, SEED, ONE_A10, TREE),
    ("flipped", 16, 8, SEED, ONE_A10, TREE),
    ("flipped", 16, 6, SEED, ONE_A10, TREE),
    ("tilted", 16, 8, SEED, ONE_A10, TREE),     # |n.z| one ulp below 1
    ("overpower", 16, 8, SEED, ONE_A10, TREE),  # power / area = +inf: resolve's finite test
    ("leaky25", 16, 8, fc.LEAKY_RNG_SEED, LATTICE_LDS, POW2),  # cdf[nl] < 1, a fall-through in the frame
    ("lights64", 16, 8, SEED, LATTICE_LDS, TREE),
    ("lights64", 16, 6, SEED, LATTICE_LDS, TREE),
    ("lights64", 8, 8, SEED, LATTICE_LDS, POW2),
    ("lights16", 16, 8, SEED, LIST_LDS, 0),
]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle(name, n_rays=16, depth_max=8, seed=SEED):
    """Oracle samples, codes and counters of a whole frame, computed once per case."""
    p = capi.make_params(W, H, SPP, n_rays=n_rays, depth_max=depth_max, seed=seed)
    ov, oc, o = ob.render_values(fc.scene(name), p, 0, with_counters=True)
    ov.setflags(write=False)
    oc.setflags(write=False)
    return ov, oc, o


@pytest.mark.parametrize("name,n_rays,depth_max,seed,lmode,fixed", CASES,
                         ids=["%s-%d-%d" % c[:3] for c in CASES])
def test_scene_matches_oracle_on_its_instance(gpu_ctx, oracle, name, n_rays, depth_max, seed, lmode, fixed):
    kw = dict(n_rays=n_rays, depth_max=depth_max, seed=seed)
    gpu_ctx.upload_scene(fc.scene(name))
    pv, pc = gpu_ctx.render_values(capi.make_params(W, H, SPP, **kw))
    inst = tuple(gpu_ctx.last_instance())
    # the stack's levels: the deepest pushed node (4 suspended levels, or the 8-level instances)
    susp = max(d for d in range(depth_max) if n_rays >> d)
    ms = 4 if susp <= 4 else 8
    assert inst == (ms, 0, lmode, 0, 1, fixed), inst
    gpu_ctx.reset_counters()
    cv, cc = gpu_ctx.render_values(capi.make_params(W, H, SPP, flags=capi.IPT_FLAG_COUNTERS, **kw))
    inst = tuple(gpu_ctx.last_instance())
    assert inst == (ms, 1, lmode, 0, 1, fixed), inst
    g = gpu_ctx.counters()
    ov, oc, o = _oracle(name, n_rays, depth_max, seed)
    assert np.array_equal(pc, oc), "product drift codes differ from the oracle"
    assert np.array_equal(_bits(pv), _bits(ov)), (
        f"product: {int((_bits(pv) != _bits(ov)).sum())} of {pv.size} samples differ from the oracle")
    assert np.array_equal(cc, oc), "counting-instance drift codes differ"
    assert np.array_equal(_bits(cv), _bits(ov)), (
        f"counting instance: {int((_bits(cv) != _bits(ov)).sum())} of {pv.size} samples differ from the oracle")
    for k in TEN:
        assert g[k] == o[k], (name, k, g[k], o[k])
    assert o["surface_hits"] > 0 and o["expanded_nodes"] > 0 and o["light_hits"] > 0 and o["skipped"] > 0
    assert _bits(ov).any()


def _image():
    return {k: np.zeros(W * H, dt) for k, dt in PLANE_KEYS}


def _assert_same(a, b, sel=slice(None), what=""):
    for k, _ in PLANE_KEYS:
        assert np.array_equal(_bits(a[k])[sel], _bits(b[k])[sel]), (what, k)


@functools.lru_cache(maxsize=None)
def _plane():
    ov, oc, _ = _oracle("default")
    return ob.accumulate(ov, oc)


def test_chunked_launch(oracle, monkeypatch):
    """IPT_TEST_CHUNK_UNITS (read at creation) splits the call into launches of one pass."""
    monkeypatch.setenv("IPT_TEST_CHUNK_UNITS", "3000")
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(fc.scene("default"))
        p = capi.make_params(W, H, SPP, n_rays=16, depth_max=8)
        gv, gc = ctx.render_values(p)
        assert tuple(ctx.last_instance()) == (4, 0, ONE_A10, 0, 1, TREE)
        ov, oc, _ = _oracle("default")
        assert np.array_equal(gc, oc) and np.array_equal(_bits(gv), _bits(ov))
        img = _image()
        ctx.render(p, img)
        _assert_same(img, _plane(), what="chunked")
    finally:
        ctx.close()


def test_two_queued_launches(gpu_ctx, oracle):
    """Two queued one-pass calls leave the oracle's two-pass plane."""
    import torch

    gpu_ctx.upload_scene(fc.scene("default"))
    q = torch.zeros(4, H, W, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for c in range(SPP):
        gpu_ctx.render_device_async(capi.make_params(W, H, 1, spp_offset=c, n_rays=16, depth_max=8),
                                    q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), q[3].data_ptr(), stream)
    gpu_ctx.wait()
    assert tuple(gpu_ctx.last_instance()) == (4, 0, ONE_A10, 0, 1, TREE)
    torch.cuda.synchronize()
    a = q.cpu().numpy()
    got = {"pixels": a[0].reshape(-1), "counters": a[1].view(np.uint32).reshape(-1),
           "sums": a[2].reshape(-1), "pixel_max": a[3].reshape(-1)}
    _assert_same(got, _plane(), what="queued")


def test_sharded_plan_with_one_row_tiles(gpu_ctx, oracle):
    gpu_ctx.upload_scene(fc.scene("default"))
    seen = np.zeros(W * H, bool)
    for shard in range(3):
        p = capi.make_params(W, H, SPP, n_rays=16, depth_max=8, tile_rows=1, n_shards=3, shard_id=shard)
        owned, _ = capi.shard_plan(p)
        mask = np.repeat(owned, W)
        img = _image()
        gpu_ctx.render(p, img)
        assert tuple(gpu_ctx.last_instance()) == (4, 0, ONE_A10, 0, 1, TREE)
        for k in img:
            assert not img[k][~mask].any(), "shard wrote outside its rows"
        _assert_same(img, _plane(), mask, "shard %d" % shard)
        seen |= mask
    assert seen.all()
