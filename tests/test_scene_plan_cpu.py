"""The library's own scene plan and instance selector, without a GPU.

tests/native/scene_plan_dump.cpp runs plan_scene (ipt_amd/csrc/ipt_scene_plan.h)
and select_path (ipt_select.h) -- the host-only code ipt_upload_scene and
launch_path run -- in a stand-alone program built with AddressSanitizer and
UndefinedBehaviorSanitizer; a sanitizer report ends the program with a non-zero
status, which fails the test that ran it.

  census keys   every case of tests/instance_cases.py takes, by the real
                selector, the instance its key claims, with and without
                IPT_FLAG_COUNTERS (the GPU half, test_gpu_instance_census.py,
                reads ipt_last_instance after a render);
  scene facts   what the plan decides for the scenes of
                test_gpu_parity.py::test_scene_sequence_leaves_nothing_behind and
                of the source's comments;
  buffer count  the buffers ipt_upload_scene allocates for the scene of
                test_failed_upload_leaves_no_scene;
  errors        plan_scene's codes and messages.
"""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import instance_cases as ic
from ipt_amd import capi, scenes

ROOT = Path(__file__).resolve().parents[1]
MAX_LDS = 160 * 1024  # ipt_ctx's default, the figure instance_cases' rule f is written against


def _hip_include():
    hipcc = Path(shutil.which(ge._hipcc()) or ge._hipcc())
    for base in (hipcc.parent.parent, hipcc.resolve().parent.parent):
        if (base / "include" / "hip" / "hip_runtime.h").exists():
            return base / "include"
    raise RuntimeError("hip/hip_runtime.h not found beside hipcc")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = tmp_path_factory.mktemp("scene_plan") / "scene_plan_dump"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", f"-I{_hip_include()}",
                    "-Wno-unknown-pragmas", "-o", str(exe), str(ROOT / "tests" / "native" / "scene_plan_dump.cpp")],
                   check=True)
    return exe


def _num(v):
    return repr(float(np.float32(v)))


def _text(desc):
    cam = desc["camera"]
    lines = [str(desc["geometry_kind"]),
             " ".join(_num(v) for k in ("position", "direction", "right", "up") for v in cam[k]),
             str(len(desc["lights"]))]
    for L in desc["lights"]:
        vals = list(L["position"]) + list(L["x_axis"]) + list(L["y_axis"]) + [L["power"], L["type"]]
        lines.append(" ".join(_num(v) for v in vals))
    spheres = desc.get("spheres", [])
    lines.append(str(len(spheres)))
    for c, r in spheres:
        lines.append(" ".join(_num(v) for v in list(c) + [r]))
    return "\n".join(lines) + "\n"


def _run(exe, desc, n_rays=8, depth_max=6, kind="default", light_grid_on=1, lnodes_lds=1):
    """(exit status, {name: value or tuple of values}); the context kinds as
    test_gpu_instance_census.py's contexts: "generic" IPT_BOX_GENERIC=1,
    "global" IPT_LATTICE_LDS=0."""
    args = [n_rays, depth_max, int(kind == "generic"), int(kind != "global"), MAX_LDS, light_grid_on, lnodes_lds]
    r = subprocess.run([str(exe)] + [str(a) for a in args], input=_text(desc), capture_output=True, text=True)
    out = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "error":
            out["error"] = (int(w[1]), " ".join(w[2:]))
        else:
            v = tuple(int(x) for x in w[1:])
            out[w[0]] = v if len(v) > 1 else v[0]
    assert r.returncode in (0, 3) and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.returncode, out


def _facts(exe, desc, **kw):
    rc, out = _run(exe, desc, **kw)
    assert rc == 0, out
    return out


@pytest.mark.parametrize("case", ic.CASES, ids=[ic.case_id(c) for c in ic.CASES])
def test_census_case_takes_its_instance(dump, case):
    key, name, params, kind = case
    p = dict(params)
    out = _facts(dump, ic.scene(name), n_rays=p["n_rays"], depth_max=p["depth_max"], kind=kind)
    assert out["inst0"] == ic.full_key(case, 0)
    assert out["inst1"] == ic.full_key(case, 1)


def test_there_are_139_census_cases():
    assert len(ic.CASES) == 139


def test_box_scene(dump):
    out = _facts(dump, scenes.make_scene_box())
    assert (out["light_axis"], out["sa_on"], out["box_inrange"]) == (1, 1, 1)
    assert (out["n_grid"], out["n_nodes"], out["n_light_nodes"]) == (0, 0, 0)  # no grid, no BVH, no light nodes
    assert (out["light_pattern"], out["lg_nu"], out["lg_nv"]) == (0, 0, 0)     # no lattice
    assert out["n_bufs"] == 5  # lights, weights, cdf, wall frames, spheres: what every scene has


def test_sphere_scenes(dump):
    out = _facts(dump, scenes.make_scene_spheres(400, seed=1))
    assert out["n_grid"] > 0 and out["n_nodes"] == 0
    # test_failed_upload_leaves_no_scene's scene: the grid's 3 buffers and the 5 every scene has
    assert out["n_bufs"] == 8
    out = _facts(dump, scenes.make_scene_spheres(50, seed=1))
    assert out["n_nodes"] > 0 and out["n_grid"] == 0


def test_lattice_scenes(dump):
    out = _facts(dump, scenes.make_scene_box_lights(5))
    assert out["light_pattern"] != 0 and (out["lg_nu"], out["lg_nv"]) == (5, 5) and out["cdf_p2"] == 0
    assert _facts(dump, scenes.make_scene_box_lights(8))["cdf_p2"] != 0
    assert _facts(dump, scenes.make_scene_box_lights(16))["cdf_p2"] == 2  # "C5's 256 equal emitters"
    # a lattice on geometry 1 is no lattice (instance_cases' rule b)
    assert _facts(dump, ic.scene("sph400/a10sq"))["light_pattern"] == 0


def test_many_and_round_lights(dump):
    out = _facts(dump, scenes.make_scene_random_lights(64, seed=7))
    assert out["light_pattern"] == 0 and out["n_light_nodes"] > 0
    out = _facts(dump, ic.scene("box/round"))
    assert (out["any_round"], out["light_axis"], out["n_light_nodes"]) == (1, 0, 0)


def test_out_of_range_camera(dump):
    assert ic.DARK == {"box/beyond"}
    out = _facts(dump, ic.scene("box/beyond"))
    assert (out["box_inrange"], out["light_axis"]) == (0, 0)


def test_plan_errors(dump):
    desc = dict(scenes.make_scene_box())
    desc["geometry_kind"] = 6
    assert _run(dump, desc) == (3, {"error": (capi.IPT_E_UNSUPPORTED, "unknown geometry_kind")})
    desc = dict(scenes.make_scene_box())
    desc["lights"] = list(desc["lights"]) * 1025
    rc, out = _run(dump, desc)
    assert rc == 3 and out["error"][0] == capi.IPT_E_UNSUPPORTED
    desc = dict(scenes.make_scene_box())
    desc["lights"] = [dict(desc["lights"][0], type=9)]
    assert _run(dump, desc) == (3, {"error": (capi.IPT_E_UNSUPPORTED, "unknown light type")})
