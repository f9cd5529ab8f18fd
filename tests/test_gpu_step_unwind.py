"""The step's bookkeeping -- pop / unwind, resolve / push, the prologue's
window -- against the oracle, on the trees where it takes every path.

Each case compares three things, as test_gpu_parity.py's
test_counters_match_oracle does: the product instance's samples and drift
codes bit for bit with the oracle's, the counting instance's samples
(IPT_FLAG_COUNTERS) bit for bit with both, and the ten event counters with the
oracle's counts.

Trees (n_rays, depth_max), on a 24x20 frame, 2 spp, spp_offset 5 (960 paths:
waves refill, the last wave is part-filled):
  (16, 8)  the workload's tree: nodes at depths 0..4, unwinds of 1..5 levels;
  (1, 8), (2, 8)  every node's last iteration, so a pop follows a push directly
           (depths 0 and 0..1);
  (17, 8)  not a power of two at any depth: res/n by division;
  (0, 8)   the camera ray only (no node, no pop);
and (64, 8) on a 4x4 frame at 1 spp (box scene): nodes at depths 0..6, the
8-level instance.

Which cases reach the unwind loop `l = tdepth - 3 > stop` (a pop that finishes
four or more levels at once: the node and at least three suspended ancestors
that were on their last iteration when they pushed) was established once on
the CPU with the oracle's iteration hook (scripts/unwind_stats.cpp, pops by
levels finished at once):
  box (16, 8):  1: 37141  2: 15634  3: 3817  4: 469  5: 29   -> loop entered 498 times
  box (17, 8):  1: 39482  2: 16627  3: 4049  4: 496  5: 34   -> 530 times
  box (2, 8):   1: 680    2: 291                              -> never
  box (1, 8):   1: 692                                        -> never
  box (0, 8):   no pop
  box (64, 8), 4x4: 1: 226127  2: 98195  3: 23501  4: 2821  5: 185  6: 9 -> 3015 times
  (the lattice scenes: within 1 % of the box's counts, 496 .. 529 times)
so the (16, 8) and (17, 8) cases of every scene run it (one or two trips), and
the (64, 8) case runs it for up to three trips.

One more call is sharded (tile_rows 4, n_shards 3, shard_id 1, the 24x20 box):
lanes then meet units that are not theirs.
"""
import functools

import numpy as np
import pytest

import oracle_binding as ob
from ipt_amd import capi, scenes

pytestmark = pytest.mark.gpu

TEN = ("paths", "traced_rays", "surface_hits", "light_hits", "expanded_nodes",
       "iterations", "light_samples", "skipped", "light_traces", "drifted")
SCENES = {"box": scenes.make_scene_box,
          "box_lights4": lambda: scenes.make_scene_box_lights(4),
          "box_lights16": lambda: scenes.make_scene_box_lights(16)}
W, H, SPP, OFF = 24, 20, 2, 5


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle(scene, w, h, spp, off, n_rays, depth_max):
    """Oracle samples, codes and counters of a whole frame, computed once per case."""
    p = capi.make_params(w, h, spp, spp_offset=off, n_rays=n_rays, depth_max=depth_max)
    ov, oc, o = ob.render_values(SCENES[scene](), p, 0, with_counters=True)
    ov.setflags(write=False)
    oc.setflags(write=False)
    return ov, oc, o


def _check(ctx, scene, w, h, spp, off, n_rays, depth_max):
    ctx.upload_scene(SCENES[scene]())
    kw = dict(spp_offset=off, n_rays=n_rays, depth_max=depth_max)
    pv, pc = ctx.render_values(capi.make_params(w, h, spp, **kw))
    ctx.reset_counters()
    cv, cc = ctx.render_values(capi.make_params(w, h, spp, flags=capi.IPT_FLAG_COUNTERS, **kw))
    g = ctx.counters()
    ov, oc, o = _oracle(scene, w, h, spp, off, n_rays, depth_max)
    assert np.array_equal(pc, oc), "product drift codes differ from the oracle"
    assert np.array_equal(_bits(pv), _bits(ov)), (
        f"product: {int((_bits(pv) != _bits(ov)).sum())} of {pv.size} samples differ from the oracle")
    assert np.array_equal(cc, pc) and np.array_equal(cc, oc), "counting-instance drift codes differ"
    assert np.array_equal(_bits(cv), _bits(pv)), (
        f"counting instance: {int((_bits(cv) != _bits(pv)).sum())} of {pv.size} samples differ from the product's")
    assert np.array_equal(_bits(cv), _bits(ov))
    for k in TEN:
        assert g[k] == o[k], (scene, n_rays, k, g[k], o[k])


@pytest.mark.parametrize("n_rays", [16, 1, 2, 17, 0])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_step_matches_oracle(gpu_ctx, oracle, scene, n_rays):
    """(16, 8) and (17, 8) reach the unwind loop past two levels (module docstring)."""
    _check(gpu_ctx, scene, W, H, SPP, OFF, n_rays, 8)


def test_eight_level_instance_matches_oracle(gpu_ctx, oracle):
    """(64, 8), 4x4 at 1 spp: nodes at depths 0..6, the unwind loop runs up to three trips."""
    _check(gpu_ctx, "box", 4, 4, 1, 0, 64, 8)


def _plane():
    return {k: np.zeros(W * H, dt) for k, dt in (("pixels", np.float32), ("counters", np.uint32),
                                                  ("sums", np.float32), ("pixel_max", np.float32))}


def test_sharded_call_matches_oracle(gpu_ctx, oracle):
    """Shard 1 of 3 (tile_rows 4) of the 24x20 box at (16, 8): the candidate
    rows hold units whose sample lands in another shard's row, which the lanes
    drop. The shard's rows of the plane are the oracle's whole-frame rows, from
    the product and from the counting instance; the counters are the oracle's
    per-path events summed over the samples that land in the shard's rows
    (`drifted` is counted by the ray generation over every candidate unit)."""
    desc = SCENES["box"]()
    gpu_ctx.upload_scene(desc)
    kw = dict(spp_offset=OFF, n_rays=16, depth_max=8, tile_rows=4, n_shards=3, shard_id=1)
    p = capi.make_params(W, H, SPP, **kw)
    owned, cand = capi.shard_plan(p)
    assert owned.any() and not owned.all()
    whole = capi.make_params(W, H, SPP, spp_offset=OFF, n_rays=16, depth_max=8)
    ov, oc, ev = ob.render_events(desc, whole)
    wv, wc, _ = _oracle("box", W, H, SPP, OFF, 16, 8)
    assert np.array_equal(_bits(ov), _bits(wv)) and np.array_equal(oc, wc)
    ref = ob.accumulate(ov, oc)
    mask = np.repeat(owned, W)

    part = _plane()
    gpu_ctx.render(p, part)
    gpu_ctx.reset_counters()
    cpart = _plane()
    gpu_ctx.render(capi.make_params(W, H, SPP, flags=capi.IPT_FLAG_COUNTERS, **kw), cpart)
    g = gpu_ctx.counters()
    for k in part:
        assert not part[k][~mask].any() and not cpart[k][~mask].any(), "shard wrote outside its rows"
        assert np.array_equal(_bits(part[k])[mask], _bits(ref[k])[mask]), ("product", k)
        assert np.array_equal(_bits(cpart[k]), _bits(part[k])), ("counting instance", k)

    # the samples this shard traces: those that land in one of its rows
    iy = np.arange(H)
    yn = np.maximum(H - 2 - iy, 0)[None, :, None]
    code = oc.astype(np.int32)
    assert not (code == 0xff).any()
    yi = yn + ((code >> 2) & 3) - 1
    mine = owned[yi]
    assert mine.any() and not mine[:, cand, :].all(), "no candidate unit lands outside the shard's rows"
    assert not mine[:, np.setdiff1d(iy, cand), :].any(), "a sample of the shard lies outside its candidate rows"
    expect = {"paths": int(mine.sum()), "drifted": int((code[:, cand, :] != 0x05).sum())}
    for k in TEN[1:9]:
        expect[k] = int(ev[..., ob.EVENT_NAMES.index(k)][mine].sum())
    for k in TEN:
        assert g[k] == expect[k], (k, g[k], expect[k])
