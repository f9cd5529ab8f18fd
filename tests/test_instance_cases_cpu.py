"""The instance census without a GPU (tests/instance_cases.py; the GPU half is
tests/test_gpu_instance_census.py).

  coverage    REACHABLE and UNREACHABLE are disjoint and together are the
              instances of a real build (profiles/path_instances.txt, written
              by scripts/path_instances.py from the build's symbol names), and
              the cases' keys, each with and without COUNT, are REACHABLE: a
              rule changed in instance_cases.py without a matching case, or an
              instance added to the build without a rule, fails here;
  liveliness  on the oracle alone every case hits surfaces and lights, samples
              lights, iterates, gives finite samples and at least 10 % non-zero
              ones (the out-of-range camera's case excepted: every sample is 0
              by construction, asserted instead);
  depth       every MAXSUSP 8 case differs from its depth_max 5 rendering in
              at least one sample: a depth-5 node was expanded, so a fifth
              level was suspended. The floor's four cases cannot: a ray that
              leaves GeometryFloor's one plane meets no surface again. Their
              MAXSUSP 8 instances are reachable all the same and stay in the
              census; here they assert what holds instead, at most one
              surface hit per path and the same bits at both depths;
  lattices    light_grid_build (tests/native/light_grid_check.cpp) takes the
              case lattices with the pattern, nu and nv the cases mean, and
              the restated cell lookup misses no light on them.

Measured with the oracle on 8 threads: the whole file 8 s, of which the
oracle's 139 cases and the 38 depth-5 renderings of the deep ones take 6 s.
"""
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import instance_cases as ic
import oracle_binding as ob

ROOT = Path(__file__).resolve().parents[1]
IDS = [ic.case_id(c) for c in ic.CASES]


def _instantiated():
    keys = []
    for line in (ROOT / "profiles" / "path_instances.txt").read_text().splitlines():
        w = line.split()
        keys.append(tuple(int(x) for x in w[:6]))
        assert "path_kernel" in w[6]
    assert len(keys) == len(set(keys))
    return set(keys)


def test_reachable_and_unreachable_are_the_build():
    inst = _instantiated()
    unreach = set(ic.UNREACHABLE)
    assert not (ic.REACHABLE & unreach)
    assert ic.REACHABLE | unreach == inst, (sorted((ic.REACHABLE | unreach) - inst), sorted(inst - ic.REACHABLE - unreach))
    assert all(isinstance(r, str) and r for r in ic.UNREACHABLE.values())
    assert (len(inst), len(ic.REACHABLE), len(unreach)) == (236, 184, 52)


def test_every_reachable_instance_has_a_case():
    keys = {ic.full_key(c, count) for c in ic.CASES for count in (0, 1)}
    assert keys == set(ic.REACHABLE), (sorted(set(ic.REACHABLE) - keys), sorted(keys - set(ic.REACHABLE)))
    assert len(set(IDS)) == len(IDS)
    assert {c[3] for c in ic.CASES} == {"default", "generic", "global"}


def test_selector_restatement_on_known_launches():
    """select() on launches whose instance the source's comments name."""
    # bench C2: sample_scenes[0], n_rays 16, depth_max 8
    assert ic.select(4, False, "one_a10", 0, False, True, True, False) == (4, 0, ic.ONE_A10, 0, 1, ic.TREE_K)
    # bench C5: the 16 x 16 lattice with its records in LDS
    assert ic.select(4, False, "lat_a10", 0, False, True, True, True) == (4, 0, ic.GRID_A10L, 0, 1, ic.TREE_K)
    # bench C3: 10 000 spheres, n_rays 8
    assert ic.select(3, False, "one", 1, False, True, False, False) == (4, 0, ic.ONE, 1, 0, 0)
    # lattice lights on a sphere list are a light BVH
    assert ic.select(3, True, "lat_a01", 1, False, True, False, False) == (4, 1, ic.GLOBAL, 1, 0, 0)


@functools.lru_cache(maxsize=None)
def _oracle(name, params):
    ov, oc, o = ob.render_values(ic.scene(name), ic.capi.make_params(**dict(params)), 0, with_counters=True)
    ov.setflags(write=False)
    return ov, o


@pytest.mark.parametrize("case", ic.CASES, ids=IDS)
def test_case_is_lively_on_the_oracle(oracle, case):
    key, name, params, kind = case
    ov, o = _oracle(name, params)
    p = dict(params)
    assert ov.size <= 12 * 8 and p["spp"] == 1
    assert o["paths"] == ov.size
    if name in ic.DARK:
        assert o["surface_hits"] == 0 and not ov.view(np.uint32).any()
        return
    for k in ("surface_hits", "light_samples", "light_hits", "iterations"):
        assert o[k] > 0, (k, o)
    assert np.isfinite(ov).all()
    assert (ov != 0).mean() >= 0.10, float((ov != 0).mean())


DEEP = [c for c in ic.CASES if c[0][0] == 8]


@pytest.mark.parametrize("case", DEEP, ids=[ic.case_id(c) for c in DEEP])
def test_deep_case_suspends_a_fifth_level(oracle, case):
    key, name, params, kind = case
    p = dict(params)
    assert p["depth_max"] >= 6 and (p["n_rays"] >> 5) > 0
    ov, _ = _oracle(name, params)
    p["depth_max"] = 5
    o5, o = _oracle(name, tuple(sorted(p.items())))
    if name.split("/")[0] in ic.SINGLE_BOUNCE:
        # one plane: no path meets a surface twice, so no depth can differ (instance_cases.SINGLE_BOUNCE)
        assert o["surface_hits"] <= o["paths"] and np.array_equal(ov.view(np.uint32), o5.view(np.uint32))
        return
    assert (ov.view(np.uint32) != o5.view(np.uint32)).any()


def test_every_maxsusp_has_cases_of_its_depth():
    for key, name, params, kind in ic.CASES:
        p = dict(params)
        susp = max([d for d in range(p["depth_max"]) if (p["n_rays"] >> d) > 0], default=0)  # needed_susp
        assert (key[0] == 4) == (susp <= 4), (name, params)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lgrid_census") / "light_grid_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DIPT_HD=inline", "-o", str(exe),
                    str(ROOT / "tests" / "native" / "light_grid_check.cpp")], check=True)
    return exe


@pytest.mark.parametrize("name", sorted(ic.LATTICES))
def test_case_lattices_on_the_host(checker, name):
    pattern, nu, nv, _ = ic.LATTICES[name]
    lights = ic.scene(f"box/{name}")["lights"]
    lines = [str(len(lights))]
    for L in lights:
        vals = list(L["position"]) + list(L["x_axis"]) + list(L["y_axis"]) + [L["power"], L["type"]]
        lines.append(" ".join(repr(float(np.float32(v))) for v in vals))
    r = subprocess.run([str(checker), "20000"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    w = r.stdout.split()
    out = {w[i]: int(w[i + 1]) for i in range(0, len(w) - 1, 2)}
    assert r.returncode == 0, out
    assert out["lattice"] == 1 and out["pattern"] == pattern
    assert (out["nu"], out["nv"]) == (nu, nv)
    assert out["hits"] > 0 and out["missed"] == 0
    if name.endswith("re"):
        assert nu != nv and len(lights) == nu * nv - 1                      # one empty cell
        x, y = np.float32(lights[0]["x_axis"]), np.float32(lights[0]["y_axis"])
        assert abs(float(np.abs(x).max()) - float(np.abs(y).max())) > 0.01  # cell width != cell height
        assert min(x.min(), y.min()) < 0                                    # an axis points the negative way
