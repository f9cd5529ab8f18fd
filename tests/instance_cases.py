"""Which path_kernel instances a launch can take, and one small case for each.

path_kernel<MAXSUSP, COUNT, LMODE, GEOM, BOXIN, FIXED> (ipt_kernels.hip) is
compiled once for every combination the selector names (select_path ...
select_path4, ipt_amd/csrc/ipt_select.h): the list in profiles/path_instances.txt, written from a build
by scripts/path_instances.py. A key here is that tuple of six integers, as
ipt_last_instance returns it; a case key is the key without COUNT.

REACHABLE restates the selector over abstract launches. An abstract launch is

  susp      needed_susp(p): the depth of the deepest pushed node, 0 .. 8
            (validate() refuses more); select_path takes MAXSUSP 4 for
            susp <= 4 and 8 otherwise;
  count     IPT_FLAG_COUNTERS (mode_of);
  lights    the scene's light class, below;
  geom      geometry_kind, 0 .. 5 (select_path3; an unknown kind renders as 0);
  generic   box scenes only: the camera or the sphere list lies outside 2^39
            (box_inrange, set at the end of plan_scene) or the context
            was created under IPT_BOX_GENERIC=1 (select_path4);
  pow2      n_rays is a power of two (select_path4: nr != 0 && !(nr & (nr-1)));
  tree16    n_rays == 16 and depth_max > 5 (select_path4, kTreeK = 4);
  lds_ok    lattices only: IPT_LATTICE_LDS is not 0 and the records-in-LDS
            layout fits the device's LDS (select_path2, path_lds_bytes).

Light classes (select_path2, and plan_scene, ipt_scene_plan.h, which sets
any_round_light, light_axis and light_pattern):

  round     any sphere, point or outer light                     -> kLightsAny
  one       one area light, light_axis == 0                      -> kLightsOne
  one_a10   one area light, light_axis == 1                      -> kLightsOneA10
  one_a01   one area light, light_axis == 2                      -> kLightsOneA01
  few       0 or 2 .. 16 (kLdsLights) area lights                -> kLightsLds
  lat_a10   more than 16 area lights, light_pattern == 1         -> kLightsGridA10[L]
  lat_a01   more than 16 area lights, light_pattern == 2         -> kLightsGridA01[L]
  many      more than 16 area lights, no lattice                 -> kLightsGlobal

Which abstract launches exist (constraints(), each from the source):

  a. light_axis is cleared unless geometry_kind is IPT_GEOM_SPHERE_IN_BOX and
     light_ranges_box() proves the light's ranges ("if (out.light_axis &&
     !(s->geometry_kind == IPT_GEOM_SPHERE_IN_BOX && light_ranges_box(...)))
     out.light_axis = 0;" in plan_scene): one_a10 / one_a01 exist on
     geom 0 only.
  b. the lattice is built for geom 0 only ("use_lgrid = ... s->geometry_kind
     == IPT_GEOM_SPHERE_IN_BOX && light_grid_build(...)" in plan_scene,
     and select_path2 compares geometry_kind again): lat_* exist on geom 0
     only. The same lights on another geometry are `many`.
  c. light_ranges_box() needs dmax <= 2^8, with the camera inside dmax: a
     scene whose camera is out of range (2^39) has neither light_axis nor a
     lattice. The aligned classes reach BOXIN = false through
     IPT_BOX_GENERIC=1 only; the result is the same set of keys.
  d. the skip-ahead plane (sa_on) needs an area light with zero z components
     in its axes, a normal along z and 2^-32 <= |P.z| <= 2^32.
     axis_aligned_light() gives the first three, light_ranges_box() gives
     |P.z| >= 2^-8 and dmax <= 2^8: sa_on is 1 for every one_a10, one_a01 and
     lat_* scene. So FIXED depends on n_rays alone for them, and their
     FIXED = 0 in-range instances are reached by an n_rays that is no power
     of two (test_gpu_box_range_instances' "pz0" light, P.z = 0, fails
     axis_aligned_light's P != 0 and renders on kLightsOne).
  e. tree16 gives susp == 4 (16 >> 4 == 1, 16 >> 5 == 0): it exists at
     MAXSUSP 4 only, as the `if constexpr (MAXSUSP == kTreeK)` says.
  f. lds_ok is false at MAXSUSP 8: block_of() gives the records-in-LDS
     instances 1024 threads, so path_lds_bytes' stack term alone is
     8 levels x 6 fields (kStackFields) x 1024 x 4 B = 192 KiB, above the
     160 KiB of LDS (max_lds). At MAXSUSP 4 the stack is 96 KiB and the case
     lattices fit.

REACHABLE is select() over every abstract launch that satisfies a-f: 184 keys.
UNREACHABLE names the other 52 instantiated keys with the rule that excludes
each: 40 by (a), 12 by (f). test_instance_cases_cpu.py holds the two against
profiles/path_instances.txt.

CASES: for every reachable case key at least one (key, scene, params, context
kind); scene is a name resolved by scene(), params the keyword arguments of
capi.make_params, kind one of "default", "generic" (IPT_BOX_GENERIC=1),
"global" (IPT_LATTICE_LDS=0).

  geometries  box; floor; corner; smallpt; fractal; sph50 (the sphere BVH);
              sph400 (the sphere grid). The fractal is seen through a narrower
              camera aimed at the crevice between its two leftmost spheres
              (the sample scene's camera meets a sphere in 2 % of a 12 x 8
              frame, and no path of it bounces five times).
  light sets  own (the sample scene's single light; the fractal's is a sphere
              light, so its kLightsOne case has `single`, a square above);
              r4, r16 (kLightsLds) and r17, r64 (kLightsGlobal): the first n
              emitters of
              make_scene_random_lights(64, seed 7); round: the scene's own
              light plus the round-light mix of test_round_lights_bit_exact;
              r600: 600 emitters, a light BVH above kLdsLightNodesMax nodes
              (the walk in global memory). Every set is defined in the box's
              coordinates and mapped affinely into the geometry's extent
              (GEOM_MAP): a rotation that brings the box's "up" (z) to the
              geometry's, a scale per axis and an offset; round lights scale
              their radius by the largest of the three.
  lattices    a10sq, a01sq: 5 x 5 square cells; a10re, a01re: 3 x 7 cells of
              0.06 x 0.025 with cell (1, 3) empty (20 lights), the A10 one
              with both axes negative, the A01 one with y negative (a light
              facing down has n.z = -x.y * y.x < 0 for A10 and x.x * y.y < 0
              for A01). a10big, a01big: 17 x 18 cells, too many records for
              the LDS at 1024 threads: global records without an override.
  trees       n_rays 12 (FIXED 0), 8 (kFixedPow2), 16 at depth_max 6 (kTreeK);
              MAXSUSP 8: n_rays 32, or 33 where FIXED must be 0, depth_max 6.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

from ipt_amd import capi, scenes

f32 = np.float32

# path_kernel's LMODE (ipt_kparams.h's kLights* enum) and FIXED
ONE, LDS, GLOBAL, ANY, ONE_A10, ONE_A01, GRID_A10, GRID_A01, GRID_A10L, GRID_A01L = range(1, 11)
FIXED_POW2, TREE_K = -1, 4
BOX = capi.IPT_GEOM_SPHERE_IN_BOX
GEOMS = tuple(range(6))
LIGHT_CLASSES = ("round", "one", "one_a10", "one_a01", "few", "lat_a10", "lat_a01", "many")


def select(susp, count, lights, geom, generic, pow2, tree16, lds_ok):
    """select_path ... select_path4 (ipt_select.h) on an abstract launch: the instance key."""
    maxsusp = 4 if susp <= 4 else 8                                    # select_path
    if lights == "round":                                              # select_path2
        lmode = ANY
    elif lights in ("one", "one_a10", "one_a01"):
        lmode = {"one": ONE, "one_a10": ONE_A10, "one_a01": ONE_A01}[lights]
    elif lights == "few":
        lmode = LDS
    elif lights in ("lat_a10", "lat_a01") and geom == BOX:
        a10 = lights == "lat_a10"
        lmode = (GRID_A10L if a10 else GRID_A01L) if lds_ok else (GRID_A10 if a10 else GRID_A01)
    else:
        lmode = GLOBAL
    if geom == BOX and not generic:                                    # select_path4
        if lmode in (ONE_A10, ONE_A01, GRID_A10, GRID_A01, GRID_A10L, GRID_A01L) and pow2:  # step_fixed_mode, sa_on (d)
            if maxsusp == TREE_K and tree16:
                return (maxsusp, int(count), lmode, geom, 1, TREE_K)
            return (maxsusp, int(count), lmode, geom, 1, FIXED_POW2)
        return (maxsusp, int(count), lmode, geom, 1, 0)
    return (maxsusp, int(count), lmode, geom, 0, 0)


def constraints(susp, count, lights, geom, generic, pow2, tree16, lds_ok):
    """Whether the abstract launch exists (a-f of the module docstring)."""
    if lights in ("one_a10", "one_a01", "lat_a10", "lat_a01") and geom != BOX:
        return False                                                   # a, b
    if geom != BOX and generic:
        return False                                                   # (generic is a property of box launches)
    if tree16 and not (pow2 and susp == 4):
        return False                                                   # e
    if lds_ok and (susp > 4 or lights not in ("lat_a10", "lat_a01")):
        return False                                                   # f
    return True


def _reachable():
    out = set()
    for a in itertools.product(range(9), (False, True), LIGHT_CLASSES, GEOMS, (False, True), (False, True),
                               (False, True), (False, True)):
        if constraints(*a):
            out.add(select(*a))
    return frozenset(out)


REACHABLE = _reachable()


def _unreachable():
    out = {}
    for m, c in itertools.product((4, 8), (0, 1)):
        for lm, g in itertools.product((ONE_A10, ONE_A01), GEOMS[1:]):
            out[(m, c, lm, g, 0, 0)] = ("plan_scene clears light_axis unless geometry_kind == "
                                        "IPT_GEOM_SPHERE_IN_BOX (rule a)")
    for c, lm in itertools.product((0, 1), (GRID_A10L, GRID_A01L)):
        for boxin, fixed in ((1, 0), (1, FIXED_POW2), (0, 0)):
            out[(8, c, lm, BOX, boxin, fixed)] = ("select_path2: path_lds_bytes<8, kLightsGridA..L> >= 192 KiB "
                                                  "> max_lds (rule f)")
    return out


UNREACHABLE = _unreachable()

# ----------------------------------------------------------------- light sets


def _map_vec(v, rot, scale):
    v = np.asarray(v, f32)
    return (np.asarray([v[abs(r) - 1] * (1 if r > 0 else -1) for r in rot], f32) * np.asarray(scale, f32)).astype(f32)


def map_light(L, gm):
    """The light L of the box's coordinates under the geometry's map gm =
    (rot, scale, offset): p -> offset + scale * rot(p), axes without the
    offset; rot = (i, j, k), signed 1-based source axes (a proper rotation)."""
    rot, scale, offset = gm
    out = dict(L)
    out["position"] = [float(x) for x in (_map_vec(L["position"], rot, scale) + np.asarray(offset, f32)).astype(f32)]
    if L["type"] in (capi.IPT_LIGHT_AREA_DIAMOND, capi.IPT_LIGHT_AREA_TRIANGLE):
        out["x_axis"] = [float(x) for x in _map_vec(L["x_axis"], rot, scale)]
        out["y_axis"] = [float(x) for x in _map_vec(L["y_axis"], rot, scale)]
    else:
        out["x_axis"] = [float(f32(L["x_axis"][0]) * f32(max(scale))), 0.0, 0.0]
    return out


IDENT = ((1, 2, 3), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
# box coordinates -> the geometry's extent
GEOM_MAP = {
    "box": IDENT,
    "sph50": IDENT, "sph400": IDENT,                       # the same box planes
    "corner": IDENT,                                       # walls x, y, z = -1, camera at (4, 1, 1)
    # one plane z = -1 seen from (0, -5, 0) at 11 degrees: the frame shows the plane from y = -2.7 to
    # the horizon, so the lights are spread along y and brought down over it
    "floor": ((1, 2, 3), (2.5, 4.0, 0.5), (0.0, 1.0, -0.4)),
    # the chain of spheres along x in [-2.5, 2.5], radius <= 0.5
    "fractal": ((1, 2, 3), (2.5, 1.0, 1.0), (0.0, 0.0, 0.0)),
    # the room [1, 99] x [0, 81.6] x [0, 170], up = +y, camera looking along -z:
    # box (x, y, z) -> (x, z, -y), a rotation about x
    "smallpt": ((1, 3, -2), (45.0, 38.0, 80.0), (50.0, 40.8, 85.0)),
}


@functools.lru_cache(maxsize=None)
def _random_lights(n):
    return tuple(scenes.make_scene_random_lights(max(n, 64), seed=7)["lights"][:n])


def _round_mix():
    return [scenes.sphere_light((0.3, 0.2, 0.4), 0.15, 0.7), scenes.point_light((-0.4, 0.3, -0.2), 0.05, 0.5),
            scenes.outer_light(9.0, 0.05), scenes.sphere_light((-0.5, -0.6, 0.5), 0.2, 1.3)]


def _lattice(pattern, nu, nv, cw, ch, empty=(), negative=False):
    """nu x nv lights of cw x ch in the plane z = -0.15, lower corner x = 0.1,
    y = -0.9; pattern 1 (A10): x_axis along y, u = y; pattern 2 (A01):
    x_axis along x, u = x. Facing down. negative: A10 with both axes negative,
    A01 with y negative (else A01 has x negative)."""
    cw, ch = f32(cw), f32(ch)
    u0, v0 = (f32(-0.9), f32(0.1)) if pattern == 1 else (f32(0.1), f32(-0.9))
    out = []
    for j in range(nv):
        for i in range(nu):
            if (i, j) in empty:
                continue
            # every light has the same axes bit for bit (the lattice needs one n.z), so a light with a
            # negative axis starts at its cell's upper corner as rounded from the lower one
            lu, lv = f32(u0 + f32(f32(i) * cw)), f32(v0 + f32(f32(j) * ch))
            hu, hv = f32(lu + cw), f32(lv + ch)
            if pattern == 1:   # x_axis = (0, +-cw, 0) spans u = y; y_axis = (+-ch, 0, 0) spans v = x
                if negative:
                    P, X, Y = (hv, hu, -0.15), (0.0, -cw, 0.0), (-ch, 0.0, 0.0)
                else:
                    P, X, Y = (lv, lu, -0.15), (0.0, cw, 0.0), (ch, 0.0, 0.0)
            else:              # x_axis = (+-cw, 0, 0) spans u = x; y_axis = (0, -+ch, 0) spans v = y
                if negative:
                    P, X, Y = (lu, hv, -0.15), (cw, 0.0, 0.0), (0.0, -ch, 0.0)
                else:
                    P, X, Y = (hu, lv, -0.15), (-cw, 0.0, 0.0), (0.0, ch, 0.0)
            out.append({"position": [float(f32(v)) for v in P], "x_axis": [float(v) for v in X],
                        "y_axis": [float(v) for v in Y], "power": float(f32(1.0) / f32(nu * nv)),
                        "type": capi.IPT_LIGHT_AREA_DIAMOND})
    return out


LATTICES = {
    # name: (pattern, nu, nv, lights)
    "a10sq": (1, 5, 5, lambda: _lattice(1, 5, 5, 0.04, 0.04)),
    "a01sq": (2, 5, 5, lambda: _lattice(2, 5, 5, 0.04, 0.04)),
    "a10re": (1, 3, 7, lambda: _lattice(1, 3, 7, 0.06, 0.025, empty=((1, 3),), negative=True)),
    "a01re": (2, 3, 7, lambda: _lattice(2, 3, 7, 0.06, 0.025, empty=((1, 3),), negative=True)),
    "a10big": (1, 17, 18, lambda: _lattice(1, 17, 18, 0.012, 0.011)),
    "a01big": (2, 17, 18, lambda: _lattice(2, 17, 18, 0.012, 0.011, negative=True)),
}

_BASE = {
    "box": scenes.make_scene_box,
    "floor": scenes.make_scene_square_lit_by_square,
    "corner": scenes.make_scene_lit_corner,
    "smallpt": scenes.make_scene_smallpt,
    "fractal": scenes.make_scene_fractal,
    "sph50": lambda: scenes.make_scene_spheres(50),
    "sph400": lambda: scenes.make_scene_spheres(400),
}
GEOM_OF = {"box": 0, "sph50": 1, "sph400": 1, "floor": 2, "corner": 3, "fractal": 4, "smallpt": 5}


@functools.lru_cache(maxsize=None)
def scene(name):
    """'<geometry>/<lights>' -> scene description (shared: do not modify)."""
    geom, lights = name.split("/")
    desc = dict(_BASE[geom]())
    gm = GEOM_MAP[geom]
    if geom == "fractal":
        # the sample scene's camera sees spheres in one sample of fifty at 12 x 8: look from the same
        # place into the crevice where the left sphere (radius 0.5 at x = -2) meets the next one, eight
        # times as narrow: paths bounce there often enough to expand a depth-5 node at 96 samples
        pos = np.asarray((0.0, -4.0, 0.0), f32)
        aim = scenes.normalize((np.asarray((-1.55, 0.0, 0.0), f32) - pos).astype(f32))
        desc["camera"] = scenes.simple_camera(pos, (aim * f32(8.0)).astype(f32))
    if lights == "own":
        pass
    elif lights == "beyond":     # out of range: the launch takes the generic instance by itself
        pos = np.asarray((0.0, -(2.0 ** 40), 0.0), f32)
        desc["camera"] = scenes.simple_camera(pos, scenes.normalize(np.asarray((0.0, 1.0, 0.0), f32)))
    elif lights == "single":     # one area light where the sample scene has a round one: above the fractal's left end
        desc["lights"] = [scenes.square_light((-2.6, -0.6, 1.2), (0.0, 0.0, -1.0), (0.0, 1.2, 0.0), 1.0)]
    elif lights == "tilted":     # one area light that is not axis-aligned: kLightsOne on the box
        desc["lights"] = [{"position": [0.1, -0.9, -0.15], "x_axis": [0.0, 0.2, 0.05], "y_axis": [0.2, 0.0, 0.0],
                           "power": 1.0, "type": capi.IPT_LIGHT_AREA_DIAMOND}]
    elif lights == "a01":        # x_side along x (test_axis_aligned_single_light_bit_exact's A01 line)
        desc["lights"] = [scenes.square_light(scenes.box_light_corner(), (0.0, 0.0, -1.0), (0.2, 0.0, 0.0), 1.0)]
    elif lights == "round":
        desc["lights"] = list(desc["lights"]) + [map_light(L, gm) for L in _round_mix()]
    elif lights in LATTICES:
        desc["lights"] = [map_light(L, gm) for L in LATTICES[lights][3]()]
    else:
        assert lights[0] == "r", name
        desc["lights"] = [map_light(L, gm) for L in _random_lights(int(lights[1:]))]
    return desc


# ---------------------------------------------------------------------- cases
W, H = 12, 8
T12 = dict(n_rays=12, depth_max=4)      # susp 3, no power of two
T8 = dict(n_rays=8, depth_max=6)        # susp 3, a power of two
T16 = dict(n_rays=16, depth_max=6)      # susp 4, the K = 4 tree
D32 = dict(n_rays=32, depth_max=6)      # susp 5: MAXSUSP 8
D33 = dict(n_rays=33, depth_max=6)      # susp 5, no power of two


def _p(tree, w=W, h=H):
    return tuple(sorted(dict(width=w, height=h, spp=1, **tree).items()))


def _cases():
    c = []

    def add(key, scene_name, tree, kind="default", w=W, h=H):
        c.append((key, scene_name, _p(tree, w, h), kind))

    # the five other geometries: every light class they can have, at both stack depths
    for g in ("floor", "corner", "smallpt", "fractal", "sph50", "sph400"):
        G = GEOM_OF[g]
        one = "single" if g == "fractal" else "own"
        for ls, lm in ((one, ONE), ("r4", LDS), ("r16", LDS), ("r17", GLOBAL), ("r64", GLOBAL), ("round", ANY)):
            add((4, lm, G, 0, 0), f"{g}/{ls}", T8)
        for ls, lm in ((one, ONE), ("r16", LDS), ("r17", GLOBAL), ("round", ANY)):
            add((8, lm, G, 0, 0), f"{g}/{ls}", D32)
    # a light BVH too large for LDS (lnodes_lds 0), alone and beside the resumable sphere walk
    add((4, GLOBAL, GEOM_OF["floor"], 0, 0), "floor/r600", T8)
    add((4, GLOBAL, GEOM_OF["sph50"], 0, 0), "sph50/r600", T8)
    # a lattice light set on a sphere-list geometry is no lattice (rule b)
    add((4, GLOBAL, GEOM_OF["sph50"], 0, 0), "sph50/a01re", T8)
    add((4, GLOBAL, GEOM_OF["sph400"], 0, 0), "sph400/a10sq", T8)

    # the box: the classes without a FIXED form, in range and generic (forced and selected)
    for ls, lm in (("tilted", ONE), ("r4", LDS), ("r16", LDS), ("r17", GLOBAL), ("r64", GLOBAL), ("r600", GLOBAL),
                   ("round", ANY)):
        add((4, lm, BOX, 1, 0), f"box/{ls}", T8)
        add((4, lm, BOX, 0, 0), f"box/{ls}", T8, "generic")
    for ls, lm in (("tilted", ONE), ("r16", LDS), ("r17", GLOBAL), ("round", ANY)):
        add((8, lm, BOX, 1, 0), f"box/{ls}", D32)
        add((8, lm, BOX, 0, 0), f"box/{ls}", D32, "generic")
    add((4, ONE, BOX, 0, 0), "box/beyond", T8)
    # the axis-aligned single light
    for ls, lm in (("own", ONE_A10), ("a01", ONE_A01)):
        add((4, lm, BOX, 1, 0), f"box/{ls}", T12)
        add((4, lm, BOX, 1, FIXED_POW2), f"box/{ls}", T8)
        add((4, lm, BOX, 1, TREE_K), f"box/{ls}", T16)
        add((4, lm, BOX, 0, 0), f"box/{ls}", T8, "generic")
        add((8, lm, BOX, 1, 0), f"box/{ls}", D33)
        add((8, lm, BOX, 1, FIXED_POW2), f"box/{ls}", D32)
        add((8, lm, BOX, 0, 0), f"box/{ls}", D32, "generic")
    # the lattices: records in LDS (default) and in global memory
    for ls in ("a10sq", "a01sq", "a10re", "a01re"):
        a10 = LATTICES[ls][0] == 1
        for kind, lm in (("default", GRID_A10L if a10 else GRID_A01L), ("global", GRID_A10 if a10 else GRID_A01)):
            add((4, lm, BOX, 1, 0), f"box/{ls}", T12, kind)
            add((4, lm, BOX, 1, FIXED_POW2), f"box/{ls}", T8, kind)
            add((4, lm, BOX, 1, TREE_K), f"box/{ls}", T16, kind)
        add((4, GRID_A10L if a10 else GRID_A01L, BOX, 0, 0), f"box/{ls}", T8, "generic")
    # 17 x 18 = 306 lights: the records-in-LDS layout needs 4 x 6 x 1024 (stack) + 12 x 1032 (frames) +
    # 564 (cdf, buckets) + 308 (cells) + 12 x 306 (records) = 41 504 words, above 160 KiB = 40 960: the
    # launch takes the global records by the selector's own rule, also in the generic context (no
    # context kind has both overrides)
    for ls in ("a10big", "a01big"):
        lm = GRID_A10 if LATTICES[ls][0] == 1 else GRID_A01
        add((4, lm, BOX, 1, TREE_K), f"box/{ls}", T16)
        add((4, lm, BOX, 0, 0), f"box/{ls}", T8, "generic")
    for ls in ("a10re", "a01re"):
        lm = GRID_A10 if LATTICES[ls][0] == 1 else GRID_A01   # MAXSUSP 8: never in LDS (rule f)
        add((8, lm, BOX, 1, 0), f"box/{ls}", D33)
        add((8, lm, BOX, 1, FIXED_POW2), f"box/{ls}", D32)
        add((8, lm, BOX, 0, 0), f"box/{ls}", D32, "generic")
    return c


CASES = _cases()
# every sample of this case is 0 by construction: exempt from the liveliness conditions
DARK = {"box/beyond"}
# GeometryFloor is one plane seen from above: a ray leaving it meets no surface again, so no node below
# depth 1 exists whatever depth_max. Its MAXSUSP 8 instances are reachable (select_path goes by n_rays and
# depth_max alone) and are rendered, but cannot suspend a fifth level.
SINGLE_BOUNCE = {"floor"}


def case_id(case):
    key, name, params, kind = case
    p = dict(params)
    return f"{name}-n{p['n_rays']}d{p['depth_max']}-{kind}-" + "_".join(str(k) for k in key)


def make_params(case, flags=0):
    return capi.make_params(**dict(case[2]), flags=flags)


def full_key(case, count):
    k = case[0]
    return (k[0], int(count)) + tuple(k[1:])
