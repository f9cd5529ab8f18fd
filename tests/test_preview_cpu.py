"""The preview estimator (IPT_FLAG_PREVIEW, ipt_preview_values) without a GPU:
the reference restatement tests/native/preview_ref.cpp pinned three ways --
its outcome counts per case, a float32 numpy composition of the oracle's
exported leaves, and the full estimator's own depth-0 light hits -- and the
header, binding and error-order checks of the new entry point."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import gui_cases
import oracle_binding
import preview_cases as pc
import preview_ref
from ipt_amd import capi

ROOT = Path(__file__).resolve().parents[1]
F = np.float32


@pytest.mark.parametrize("name", sorted(pc.EXPECT))
def test_pinned_outcome_counts(oracle, name):
    *_, kinds, hits, cnt = pc.reference(name)
    c = preview_ref.classes(kinds)
    outcomes, sw, lw, la = pc.EXPECT[name]
    assert (c["outcomes"], c["surface_wins"], c["light_wins"], c["light_alone"]) == (outcomes, sw, lw, la)
    pc.check_branches(name, kinds)
    assert np.isfinite(hits).all()
    n = kinds.size
    assert cnt["paths"] == cnt["traced_rays"] == n
    assert cnt["surface_hits"] == int(((kinds & preview_ref.KIND_SI) != 0).sum())
    assert cnt["light_hits"] == int(((kinds & preview_ref.KIND_LI) != 0).sum())
    assert cnt["light_traces"] == n * len(pc.scene(name)["lights"])
    assert all(cnt[k] == 0 for k in preview_ref.ZERO_COUNTERS)


@pytest.mark.parametrize("name", sorted(pc.EXPECT_OUTCOMES))
def test_pinned_degenerate_frames(oracle, name):
    *_, kinds, _, _ = pc.reference(name)
    assert preview_ref.classes(kinds)["outcomes"] == pc.EXPECT_OUTCOMES[name]


def _dot(a, b):
    t = (a * b).astype(F)
    return F(F(t[0] + t[1]) + t[2])


def _length(v):
    return np.sqrt(_dot(v, v), dtype=F)


# (16 x 16 through the sphere holds no sample with both hits: the case's own
# frame adds the comparison's surface side)
@pytest.mark.parametrize("cam,W,H,want", [("box/up", 16, 16, {2 | 4 | 8, 2 | 8}), ("box/thru", 16, 16, set()),
                                          ("box/thru", pc.W, pc.H, {1 | 4 | 8})])
def test_restatement_is_a_composition_of_the_oracle_leaves(oracle, cam, W, H, want):
    """Jitter, camera ray, geometry hit and nearest light from the oracle's
    exported leaves; the length comparison and dot / length in float32 numpy."""
    lib = oracle_binding.setup_probes()
    desc = pc.scene(cam)
    p = capi.make_params(W, H, pc.SPP, spp_offset=pc.OFFSET)
    rv, rc, rk, rh, _ = preview_ref.render(desc, p)
    s, keep = capi.make_scene(desc)
    c = desc["camera"]
    o, cd, cr, cu = (np.array(c[k], F) for k in ("position", "direction", "right", "up"))
    fp = oracle_binding.fptr
    below_one = np.nextafter(F(1.0), F(0.0))
    seen = set()
    for sp in range(p.spp):
        for iy in range(H):
            for ix in range(W):
                u = [F(lib.ipt_oracle_randf(p.seed, p.spp_offset + sp, iy * W + ix, k)) for k in (0, 1)]
                x = F(F(F(ix) + u[0]) / F(W))
                y = F(F(F(iy) + u[1]) / F(H))
                x = below_one if x == F(1.0) else x
                y = below_one if y == F(1.0) else y
                d = np.zeros(3, F)
                lib.ipt_oracle_camera_ray(fp(cd), fp(cr), fp(cu), x, y, fp(d))
                si, li = np.zeros(6, F), np.zeros(4, F)
                has_si = bool(lib.ipt_oracle_trace_box(fp(o), fp(d), fp(si)))
                has_li = bool(lib.ipt_oracle_collection_trace(s.lights, s.n_lights, fp(o), fp(d), fp(li)))
                hit = np.zeros(6, F)
                if has_li and (not has_si or _length((si[:3] - o).astype(F)) > _length((li[:3] - o).astype(F))):
                    value, outcome = F(1.0), 2
                    hit[:3] = li[:3]
                elif not has_si:
                    value, outcome = F(0.0), 0
                else:
                    value, outcome = F(_dot(si[3:], (-d).astype(F)) / _length(d)), 1
                    hit[:] = si
                value = value if value >= 0 else F(0.0)
                kind = outcome | (4 if has_si else 0) | (8 if has_li else 0)
                assert F(value).view(np.uint32) == rv[sp, iy, ix].view(np.uint32), (sp, iy, ix)
                assert kind == rk[sp, iy, ix], (sp, iy, ix)
                assert np.array_equal(hit, rh[sp, iy, ix]), (sp, iy, ix)
                seen.add(kind)
    assert want <= seen


@pytest.mark.parametrize("name", sorted(pc.EXPECT))
def test_light_outcome_is_the_full_estimators_depth0_light(oracle, name):
    """n_rays = 0, depth_max = 1 returns the light's surface power where
    ray_power's first branch is taken and 0 elsewhere: the same si, li and
    comparison. The drift codes are render_sample's, whatever the estimator."""
    _, codes, kinds, _, _ = pc.reference(name)
    ov, oc = oracle_binding.render_values(pc.scene(name), pc.params(name, n_rays=0, depth_max=1))
    assert np.array_equal((kinds & 3) == preview_ref.OUTCOME_LIGHT, ov != 0)
    assert np.array_equal(codes, oc)


def test_gui_codes_are_the_gui_restatements(oracle):
    _, codes, _, _, _ = pc.reference("box/up", capi.IPT_FLAG_GUI_PLANE)
    assert np.array_equal(codes, gui_cases.codes(pc.W, pc.H, pc.SPP, pc.OFFSET))
    v0 = pc.reference("box/up")[0]
    assert np.array_equal(v0, pc.reference("box/up", capi.IPT_FLAG_GUI_PLANE)[0])


def test_header_and_binding():
    hdr = (ROOT / "include" / "ipt_capi.h").read_text()
    assert re.search(r"IPT_FLAG_PREVIEW\s*=\s*4u", hdr)
    assert re.search(r"#define IPT_ABI_VERSION 7\b", hdr)
    assert capi.IPT_FLAG_PREVIEW == 4 and capi.ABI_VERSION == 7
    assert "ipt_preview_values" in capi.EXPORTED_SYMBOLS
    lib = capi.load()
    assert lib.ipt_abi_version() == 7
    assert C.cast(lib.ipt_preview_values, C.c_void_p).value


def test_errors_without_a_device():
    """Argument errors come first (a NULL context is IPT_E_INVALID); a context
    cannot be made without a gfx950 device (IPT_E_DEVICE, no CPU fallback), so
    no preview call can get further here."""
    import torch

    lib = capi.load()
    p = capi.make_params(4, 4, 1, n_rays=-5, depth_max=99, flags=capi.IPT_FLAG_PREVIEW)
    buf = np.zeros(16 * 6, np.float32)
    img = capi.Image()
    img.pixels = img.counters = buf.ctypes.data
    assert lib.ipt_render(None, C.byref(p), C.byref(img)) == capi.IPT_E_INVALID
    assert lib.ipt_preview_values(None, C.byref(p), buf.ctypes.data, buf.ctypes.data, None, None) == capi.IPT_E_INVALID
    if not torch.cuda.is_available():
        with pytest.raises(capi.IptError) as e:
            capi.Context(0).preview_values(p)
        assert e.value.code == capi.IPT_E_DEVICE
