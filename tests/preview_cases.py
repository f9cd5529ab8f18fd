"""Scenes, cameras and pinned reference counts of the preview estimator's
tests (tests/test_preview_cpu.py without a GPU, tests/test_gpu_preview.py on
one).

With every scenes.py builder's own camera no sample of box, floor, corner,
fractal, box_lights or spheres sees a light (the box light faces down at
z = -0.15 and the camera sits above it), so the cases define cameras of their
own: UP looks up at the light from below, THRU looks at it through the r = 0.5
sphere, which then occludes it.

EXPECT pins, per case, the reference restatement's outcome histogram [miss,
surface, light] and the samples in which both si and li exist (won by the
surface / by the light) or the light is hit with no surface behind it, at the
case's frame, 2 passes from spp_offset 3, default seed. A case's non-zero
entries are the branches it is there to reach: the GPU tests assert them
against the reference before comparing, so a scene edit cannot silently empty
a branch."""
import functools

import numpy as np

import preview_ref
from ipt_amd import capi, scenes

f32 = np.float32
W, H, SPP, OFFSET = 37, 23, 2, 3


def look_at(position, target, up_hint=(0.0, 0.0, 1.0)):
    """SimpleCamera at `position` looking at `target` (sample_scenes.cpp's
    normalize(target - position))."""
    pos = np.array(position, f32)
    d = scenes.normalize((np.array(target, f32) - pos).astype(f32))
    return scenes.simple_camera(pos, d, up_hint)


UP = look_at((0.2, -0.8, -0.9), (0.2, -0.8, 1.0), (0.0, 1.0, 0.0))
THRU = look_at((-0.2, 0.8, -0.8), (0.2, -0.8, -0.15), (0.0, 0.0, 1.0))


def with_camera(desc, cam):
    return dict(desc, camera=cam) if cam is not None else desc


def tilted_light_scene():
    d = scenes.make_scene_box()
    light = dict(d["lights"][0], x_axis=[float(f32(v)) for v in (0.05, 0.2, 0.0)],
                 y_axis=[float(f32(v)) for v in (0.2, -0.05, 0.03)])
    return dict(d, lights=[light])


def round_lights_scene():
    d = scenes.make_scene_box()
    return dict(d, lights=d["lights"] + [scenes.sphere_light((0.5, -0.5, 0.6), 0.1),
                                         scenes.point_light((-0.5, -0.5, 0.5), 0.05), scenes.outer_light(5.0)])


# name -> (scene builder, camera or None for the builder's own, (W, H))
CASES = {
    "box/up": (scenes.make_scene_box, UP, (W, H)),
    "box/thru": (scenes.make_scene_box, THRU, (W, H)),
    "box_lights4/up": (lambda: scenes.make_scene_box_lights(4), UP, (W, H)),      # 16 lights
    "box_lights5/up": (lambda: scenes.make_scene_box_lights(5), UP, (W, H)),      # lattice of 25
    "box_lights16/up": (lambda: scenes.make_scene_box_lights(16), UP, (W, H)),    # lattice of 256
    "tilted/up": (tilted_light_scene, UP, (W, H)),                                # one general light
    "random17/up": (lambda: scenes.make_scene_random_lights(17), UP, (W, H)),     # light BVH
    "random17/thru": (lambda: scenes.make_scene_random_lights(17), THRU, (W, H)),
    "random64/up": (lambda: scenes.make_scene_random_lights(64), UP, (W, H)),
    "spheres10000/up": (lambda: scenes.make_scene_spheres(10000), UP, (W, H)),    # sphere grid
    "spheres10000/thru": (lambda: scenes.make_scene_spheres(10000), THRU, (W, H)),
    "spheres400/up": (lambda: scenes.make_scene_spheres(400), UP, (W, H)),
    "spheres50/up": (lambda: scenes.make_scene_spheres(50), UP, (W, H)),
    "spheres10/up": (lambda: scenes.make_scene_spheres(10), UP, (W, H)),          # linear list
    "round/stock": (round_lights_scene, None, (W, H)),
    "round/up": (round_lights_scene, UP, (W, H)),
    "floor": (scenes.make_scene_square_lit_by_square, look_at((0.0, -0.6, -0.98), (0.0, 0.0, -0.93)), (W, H)),
    "corner/lit": (scenes.make_scene_lit_corner, look_at((-0.9, -0.9, -0.9), (0.0, 0.0, 0.0)), (W, H)),
    "corner/stock": (scenes.make_scene_lit_corner, None, (W, H)),
    "fractal": (scenes.make_scene_fractal, look_at((0.0, -4.0, 0.0), (-5.5, 0.0, 0.0)), (W, H)),
    "smallpt": (scenes.make_scene_smallpt, look_at((50.0, 40.0, 81.6), (50.0, 81.6, 81.6)), (W, H)),
    # degenerate frames (257x1: a unit range crossing a 256-thread block)
    "box/up/1x1": (scenes.make_scene_box, UP, (1, 1)),
    "box/up/1x7": (scenes.make_scene_box, UP, (1, 7)),
    "box/up/7x1": (scenes.make_scene_box, UP, (7, 1)),
    "box/up/257x1": (scenes.make_scene_box, UP, (257, 1)),
    "box/up/64x5": (scenes.make_scene_box, UP, (64, 5)),
}

_BOX_UP = ([756, 823, 123], 0, 107, 16)
# name -> (outcomes [miss, surface, light], surface wins, light wins, light with no surface)
EXPECT = {
    "box/up": _BOX_UP,
    "box/thru": ([781, 921, 0], 8, 0, 0),
    "box_lights4/up": _BOX_UP,
    "box_lights5/up": _BOX_UP,
    "box_lights16/up": _BOX_UP,
    "tilted/up": ([739, 835, 128], 0, 95, 33),
    "random17/up": ([741, 812, 149], 7, 118, 31),
    "random17/thru": ([749, 921, 32], 64, 0, 32),
    "random64/up": ([741, 810, 151], 30, 120, 31),
    "spheres10000/up": ([351, 1340, 11], 112, 11, 0),
    "spheres10000/thru": ([15, 1687, 0], 8, 0, 0),
    "spheres400/up": ([704, 875, 123], 0, 107, 16),
    "spheres50/up": ([777, 802, 123], 0, 107, 16),
    "spheres10/up": ([790, 789, 123], 0, 107, 16),
    "round/stock": ([0, 1223, 479], 1223, 4, 475),
    "round/up": ([0, 796, 906], 796, 134, 772),
    "floor": ([1004, 692, 6], 0, 0, 6),
    "corner/lit": ([1323, 0, 379], 0, 0, 379),
    "corner/stock": ([1125, 577, 0], 0, 0, 0),
    "fractal": ([1547, 35, 120], 0, 0, 120),
    "smallpt": ([0, 1528, 174], 0, 174, 0),
}
# the degenerate frames' outcome histograms
EXPECT_OUTCOMES = {
    "box/up/1x1": [0, 2, 0],
    "box/up/1x7": [5, 8, 1],
    "box/up/7x1": [7, 6, 1],
    "box/up/257x1": [234, 248, 32],
    "box/up/64x5": [282, 313, 45],
}


def params(name, flags=0, spp=SPP, spp_offset=OFFSET, **kw):
    w, h = CASES[name][2]
    return capi.make_params(w, h, spp, spp_offset=spp_offset, flags=flags, **kw)


@functools.lru_cache(maxsize=None)
def scene(name):
    build, cam, _ = CASES[name]
    return with_camera(build(), cam)


@functools.lru_cache(maxsize=None)
def reference(name, flags=0, spp=SPP, spp_offset=OFFSET):
    """The reference restatement's (values, codes, kinds, hits, counters) of a
    case, computed once and read-only."""
    return preview_ref.render(scene(name), params(name, flags, spp, spp_offset))


def check_branches(name, kinds):
    """Every outcome and both-hit class EXPECT names for the case is present in
    the reference's kinds."""
    c = preview_ref.classes(kinds)
    if name in EXPECT:
        outcomes, sw, lw, la = EXPECT[name]
        for k in range(3):
            assert (c["outcomes"][k] > 0) == (outcomes[k] > 0), (name, c)
        assert (c["surface_wins"] > 0) == (sw > 0) and (c["light_wins"] > 0) == (lw > 0), (name, c)
        assert (c["light_alone"] > 0) == (la > 0), (name, c)
    elif name in EXPECT_OUTCOMES:
        for k in range(3):
            assert (c["outcomes"][k] > 0) == (EXPECT_OUTCOMES[name][k] > 0), (name, c)
    return c
