"""Scenes of the no-fall-through tests: tests/test_fixed_facts_host.py
asks the library's plan and selector about them without a GPU,
tests/test_gpu_fixed_facts.py renders them.

NO_FALLTHROUGH[name]: what plan_scene must find. In the single-light and
LDS-lattice instances a launch of n_rays 16 and depth_max > 5 takes FIXED = 4
(kTreeK) only with it, else kFixedPow2 (-1).

  default, far  sample_scenes[0] from its camera and from the far camera;
  flipped       its light's normal flipped to +z (the same square);
  tilted        a square whose sides' product rounds so that the normalized
                normal's n.z is one ulp below 1 (0x3f7fffff): still a
                skip-ahead plane and an axis-aligned light;
  overpower     the light's power / area overflows to +inf: the weights are
                the default's (0.5, 0.5), resolve's finite test decides;
  leaky25       the 25-light lattice with hashed powers whose running sum
                cdf[25] rounds below 1: fall-through words exist;
  lights64      the 64-light lattice (uniform on the draw's integer);
  lights256     bench.py's C5 scene;
  lights16      the 16-light list (no fixed instance at all).
"""
import functools

import numpy as np

from ipt_amd import scenes

f32 = np.float32
TILT_SIDE = 0.10040000081062317  # the first side 0.1 + i 1e-4 (float) whose normal has n.z = -0x3f7fffff
# the first powers' seed of 1 .. 299 that leaves 4 of the 2^24 draw values past
# cdf[25], and the first RNG seed with which the 64 x 48 x 2 frame meets one
# (found with the oracle; test_fixed_facts_host.py checks both)
LEAKY_SEED = 115
LEAKY_RNG_SEED = 5

NO_FALLTHROUGH = {
    "default": 1, "far": 1, "flipped": 1, "tilted": 1, "overpower": 1, "leaky25": 0, "lights64": 1, "lights256": 1,
}


def _light(normal_z=-1.0, side=0.2, power=1.0):
    cx, cy, cz = scenes.box_light_corner()
    if normal_z > 0:
        cx = f32(cx + f32(side))
    return scenes.square_light((cx, cy, cz), (0.0, 0.0, normal_z), (0.0, side, 0.0), power)


def leaky_lights(seed):
    """make_scene_box_lights(5) with powers (1 + hash) / 64 instead of 1/25."""
    desc = scenes.make_scene_box_lights(5)
    g = scenes.splitmix64(seed)
    lights = []
    for L in desc["lights"]:
        lights.append(dict(L, power=float(f32(f32(1.0 + (next(g) >> 40) * (1.0 / (1 << 24))) / f32(64.0)))))
    return dict(desc, lights=lights)


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "lights16":
        return scenes.make_scene_box_lights(4)
    if name == "lights64":
        return scenes.make_scene_box_lights(8)
    if name == "lights256":
        return scenes.make_scene_box_lights(16)
    if name == "leaky25":
        return leaky_lights(LEAKY_SEED)
    desc = scenes.make_scene_box()
    if name == "far":
        pos = np.asarray((3.0, -6.0, 2.5), np.float32)
        desc["camera"] = scenes.simple_camera(pos, scenes.normalize(-pos))
    elif name == "flipped":
        desc["lights"] = [_light(+1.0)]
    elif name == "tilted":
        desc["lights"] = [_light(-1.0, TILT_SIDE)]
    elif name == "overpower":
        desc["lights"] = [_light(-1.0, 0.2, 3.0e38)]
    elif name != "default":
        raise KeyError(name)
    return desc


def scene_text(desc):
    """The scene as tests/native/scene_plan_dump.cpp and fixed_facts_check.cpp read it."""
    def num(v):
        return repr(float(np.float32(v)))

    cam = desc["camera"]
    lines = [str(desc["geometry_kind"]),
             " ".join(num(v) for k in ("position", "direction", "right", "up") for v in cam[k]),
             str(len(desc["lights"]))]
    for L in desc["lights"]:
        vals = list(L["position"]) + list(L["x_axis"]) + list(L["y_axis"]) + [L["power"], L["type"]]
        lines.append(" ".join(num(v) for v in vals))
    spheres = desc.get("spheres", [])
    lines.append(str(len(spheres)))
    for c, r in spheres:
        lines.append(" ".join(num(v) for v in list(c) + [r]))
    return "\n".join(lines) + "\n"
