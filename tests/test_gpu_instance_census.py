"""Every reachable path_kernel instance against the oracle, once.

tests/instance_cases.py restates the selector (select_path, ipt_select.h; the
CPU suite holds every case's key against the selector itself,
tests/test_scene_plan_cpu.py) and gives every instance it can return a small case; this file renders each
case with and without IPT_FLAG_COUNTERS and asserts, in this order,

  1. ipt_last_instance() is the case's key, so that a case which drifted onto
     another instance fails as such and not as a pass on the wrong kernel;
  2. drift codes and sample bits equal the oracle's (no tolerance);
  3. with COUNT, the ten event counters equal the oracle's.

Contexts: the session's, one created under IPT_BOX_GENERIC=1 (the generic box
form on rays that hit) and one under IPT_LATTICE_LDS=0 (the lattice records in
global memory); the environment is read at creation. The liveliness of the
cases (no black frames, a fifth suspended level at MAXSUSP 8) is the business
of tests/test_instance_cases_cpu.py, on the oracle alone.
"""
import functools

import numpy as np
import pytest

import instance_cases as ic
import oracle_binding as ob
from ipt_amd import capi
from test_gpu_box_range_instances import TEN

pytestmark = pytest.mark.gpu


def _ctx_under(var, value):
    mp = pytest.MonkeyPatch()
    mp.setenv(var, value)
    try:
        return capi.Context(0)
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def generic_ctx():
    ctx = _ctx_under("IPT_BOX_GENERIC", "1")
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def global_ctx():
    ctx = _ctx_under("IPT_LATTICE_LDS", "0")
    yield ctx
    ctx.close()


CTX_FIXTURE = {"default": "gpu_ctx", "generic": "generic_ctx", "global": "global_ctx"}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle(name, params):
    """Oracle samples, codes and counters of a case, computed once for both COUNT values."""
    ov, oc, o = ob.render_values(ic.scene(name), capi.make_params(**dict(params)), 0, with_counters=True)
    ov.setflags(write=False)
    oc.setflags(write=False)
    return ov, oc, o


def test_no_launch_no_instance():
    """A context that has launched no path kernel has no instance to report
    (also after a scene upload and a preview, which launches another kernel)."""
    ctx = capi.Context(0)
    try:
        for step in range(2):
            with pytest.raises(capi.IptError) as e:
                ctx.last_instance()
            assert e.value.code == capi.IPT_E_INVALID
            ctx.upload_scene(ic.scene("box/own"))
            ctx.render_values(capi.make_params(8, 8, 1, flags=capi.IPT_FLAG_PREVIEW))
        ctx.render_values(capi.make_params(8, 8, 1, n_rays=2, depth_max=2))
        assert ctx.last_instance() == (4, 0, ic.ONE_A10, 0, 1, ic.FIXED_POW2)
    finally:
        ctx.close()


@pytest.mark.parametrize("count", [0, 1], ids=["product", "counting"])
@pytest.mark.parametrize("case", ic.CASES, ids=[ic.case_id(c) for c in ic.CASES])
def test_instance_matches_oracle(request, oracle, case, count):
    key, name, params, kind = case
    ctx = request.getfixturevalue(CTX_FIXTURE[kind])
    ctx.upload_scene(ic.scene(name))
    if count:
        ctx.reset_counters()
    gv, gc = ctx.render_values(ic.make_params(case, flags=capi.IPT_FLAG_COUNTERS if count else 0))
    assert ctx.last_instance() == ic.full_key(case, count)
    ov, oc, o = _oracle(name, params)
    assert np.array_equal(gc, oc), "drift codes differ from the oracle"
    assert np.array_equal(_bits(gv), _bits(ov)), (
        f"instance {ic.full_key(case, count)}: {int((_bits(gv) != _bits(ov)).sum())} of {gv.size} samples differ "
        f"from the oracle")
    if count:
        g = ctx.counters()
        for k in TEN:
            assert g[k] == o[k], (k, g[k], o[k])
