"""Host checks of the scene fact of the product FIXED = K box instances
(DESIGN.md 4.19), without a GPU: tests/native/fixed_facts_check.cpp, built with
AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program over
the library's own headers.

  fact       plan_scene finds no_fallthrough as fixed_facts_cases.NO_FALLTHROUGH
             claims; bench.py's scenes (C2 and C4: sample_scenes[0]; C5: 256
             emitters) have it;
  selector   in the single-light and LDS-lattice instances kTreeK exactly with
             the fact (forced on and off on the same launch), for one light
             only with a 32-bit pick threshold as well (pk_u0 forced to 2^32);
             the lattices with global records take kTreeK whatever the fact
             says; the counting flag changes nothing; the tree shapes;
  leaky25    the oracle meets a fall-through (an iteration of one draw) in the
             GPU test's frame of that scene, and none in the default scene's.
"""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import fixed_facts_cases as fc
import instance_cases as ic
import oracle_binding as ob
from ipt_amd import capi

ROOT = Path(__file__).resolve().parents[1]


def _hip_include():
    hipcc = Path(shutil.which(ge._hipcc()) or ge._hipcc())
    for base in (hipcc.parent.parent, hipcc.resolve().parent.parent):
        if (base / "include" / "hip" / "hip_runtime.h").exists():
            return base / "include"
    raise RuntimeError("hip/hip_runtime.h not found beside hipcc")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fixed_facts") / "fixed_facts_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", f"-I{_hip_include()}",
                    "-Wno-unknown-pragmas", "-o", str(exe), str(ROOT / "tests" / "native" / "fixed_facts_check.cpp")],
                   check=True)
    return exe


def _run(exe, args, desc=None):
    r = subprocess.run([str(exe)] + [str(a) for a in args], input=fc.scene_text(desc) if desc else "",
                       capture_output=True, text=True)
    assert not r.stderr, r.stderr[-2000:]
    return r.returncode, r.stdout


def _plan(exe, desc, n_rays=16, depth_max=8, lattice_lds=1):
    rc, out = _run(exe, ["plan", n_rays, depth_max, lattice_lds], desc)
    assert rc == 0, out
    o = {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines()}
    assert o["count_differs"] == 0 and o["fixed0"] == o["fixed1"]
    return o


ONE_LIGHT = ("default", "far", "flipped", "tilted", "overpower")


@pytest.mark.parametrize("name", sorted(fc.NO_FALLTHROUGH))
def test_scene_fact_and_instance(check, name):
    o = _plan(check, fc.scene(name))
    assert o["no_fallthrough"] == fc.NO_FALLTHROUGH[name]
    assert o["sa_on"] == 1 and o["pick32"] == 1
    assert o["lmode"] == (5 if name in ONE_LIGHT else 9)  # kLightsOneA10, kLightsGridA10L
    assert o["fixed0"] == (4 if o["no_fallthrough"] else -1)
    # the same launch with the fact forced: the tree instance with it, not without it;
    # a 2^32 pick threshold (a certain light pick) bars it for one light only
    assert (o["tree_on"], o["tree_off"]) == (1, 0)
    assert o["tree_wide"] == (0 if name in ONE_LIGHT else 1)
    if name == "tilted":
        assert o["sa_nz_bits"] == 0xBF7FFFFF  # one ulp below 1
    assert o["fallthrough_values"] == (4 if name == "leaky25" else 0)


@pytest.mark.parametrize("n_rays,depth_max,fixed", [(16, 8, 4), (16, 6, 4), (16, 5, -1), (8, 8, -1), (32, 8, -1)])
def test_tree_shape_still_decides(check, n_rays, depth_max, fixed):
    o = _plan(check, fc.scene("default"), n_rays, depth_max)
    assert o["fixed0"] == fixed
    assert (o["tree_on"], o["tree_off"], o["tree_wide"]) == ((1, 0, 0) if fixed == 4 else (0, 0, 0))
    # without the fact the same launch takes the power-of-two form
    assert _plan(check, fc.scene("leaky25"), n_rays, depth_max)["fixed0"] == -1


def test_global_record_lattices_are_not_asked(check):
    """kLightsGridA10 / A01 keep the general pick in their FIXED = 4 instances."""
    # the 17 x 18 census lattice (too many records for the LDS): fall-through words, kTreeK all the same
    o = _plan(check, ic.scene("box/a10big"), 16, 6)
    assert (o["lmode"], o["no_fallthrough"], o["fallthrough_values"], o["fixed0"]) == (7, 0, 48, 4)
    assert (o["tree_on"], o["tree_off"], o["tree_wide"]) == (1, 1, 1)
    o = _plan(check, ic.scene("box/a01big"), 16, 6)
    assert (o["lmode"], o["no_fallthrough"], o["fixed0"], o["tree_off"]) == (8, 0, 4, 1)
    # IPT_LATTICE_LDS=0 puts the 64-light lattice and the leaky one there too
    o = _plan(check, fc.scene("lights64"), lattice_lds=0)
    assert (o["lmode"], o["no_fallthrough"], o["fixed0"], o["tree_off"]) == (7, 1, 4, 1)
    o = _plan(check, fc.scene("leaky25"), lattice_lds=0)
    assert (o["lmode"], o["no_fallthrough"], o["fixed0"]) == (7, 0, 4)


def test_the_list_of_16_lights_has_no_fixed_instance(check):
    o = _plan(check, fc.scene("lights16"))
    assert (o["sa_on"], o["lmode"], o["fixed0"]) == (0, 2, 0)
    assert (o["tree_on"], o["tree_off"], o["tree_wide"]) == (0, 0, 0)


def _fallthroughs(name, seed):
    p = capi.make_params(64, 48, 2, n_rays=16, depth_max=8, seed=seed)
    _, _, ev = ob.render_events(fc.scene(name), p)
    it = ev[..., ob.EVENT_NAMES.index("iterations")].astype(np.int64)
    draws = ev[..., ob.EVENT_NAMES.index("draws")].astype(np.int64)
    # a path draws two jitter words and three per iteration, one for a fall-through
    twice = 2 + 3 * it - draws
    assert (twice >= 0).all() and not (twice & 1).any()
    return int(twice.sum() // 2)


def test_the_leaky_frame_meets_a_fallthrough():
    assert _fallthroughs("leaky25", fc.LEAKY_RNG_SEED) >= 1
    assert _fallthroughs("default", fc.LEAKY_RNG_SEED) == 0
