"""The denoiser's restatement (tests/denoise_cases.py) without a GPU: it tells
the wrong variants apart on pinned cases, keeps what the filter must keep,
reduces the error of a 4-pass frame against the oracle's own 256-pass plane,
and the header, the binding and the library agree on the new entry points.
Oracle and preview restatement only."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from ipt_amd import capi, scenes

import denoise_cases as dn
import oracle_binding
import preview_cases as pc

ROOT = Path(__file__).resolve().parents[1]
F = np.float32

# pixels whose (colour, variance) differ from the restatement's, 3 iterations,
# defaults otherwise, box scene 4 passes
WRONG_37x23 = {
    "unsquared_var": (574, 575),
    "linear_step": (548, 547),
    "all_taps": (257, 260),
    "dx_outer": (394, 474),
    "prefilter_at_s": (571, 571),
}
WRONG_DX_OUTER_131x67 = (4848, 5648)


def _differ(W, H, wrong, iterations=3):
    img, m2 = dn.box_plane(W, H)
    g = dn.box_guides(W, H)
    ref = dn.denoise(img["pixels"], img["counters"], m2, g, W, H, iterations=iterations)
    out = dn.denoise(img["pixels"], img["counters"], m2, g, W, H, iterations=iterations, wrong=wrong)
    return int((~dn.same(ref[0], out[0])).sum()), int((~dn.same(ref[1], out[1])).sum())


@pytest.mark.parametrize("wrong", dn.WRONG)
def test_restatement_differs_from_each_wrong_variant(wrong):
    assert _differ(37, 23, wrong) == WRONG_37x23[wrong]


def test_tap_order_matters_on_the_frame_wider_than_a_tile():
    assert _differ(131, 67, "dx_outer") == WRONG_DX_OUTER_131x67


def test_one_iteration_cannot_tell_the_step_rules_apart():
    """Step 1 << 0 == 0 + 1 and the prefilter distance is s = 1: the pinned
    cases above need their 3 iterations."""
    assert _differ(37, 23, "linear_step", 1) == (0, 0)
    assert _differ(37, 23, "prefilter_at_s", 1) == (0, 0)


def _flat_guides(W, H):
    g = np.zeros((H, W), capi.GuideRecord)
    g["kind"] = 1 | 4
    g["pos"][..., 0] = np.arange(W, dtype=F)[None, :]
    g["pos"][..., 1] = np.arange(H, dtype=F)[:, None]
    g["normal"][..., 2] = F(1.0)
    return g


def test_zero_variance_gives_the_input_back():
    """m2 = 0: den = 2^-20. On a flat plane wn = wz = 1. Colours are multiples
    of 2^-8, so a tap of another colour is at least 2^-8 away and has wl = 0,
    a tap of the same colour has w = h, a dyadic fraction of at most 4
    significant bits: every product and sum is exact, sc = col * sw, and the
    quotient is the input bit for bit. The variance stays 0."""
    W, H = 37, 23
    rng = np.random.default_rng(11)
    px = (rng.integers(1, 6, W * H).astype(F) * F(2.0 ** -8)).astype(F)  # few levels: equal neighbours occur
    cn = rng.integers(2, 9, W * H).astype(np.uint32)
    m2 = np.zeros(W * H, F)
    for it in (1, 4):
        out, var = dn.denoise(px, cn, m2, _flat_guides(W, H), W, H, iterations=it)
        assert np.array_equal(out.view(np.uint32), px.view(np.uint32))
        assert np.array_equal(var.view(np.uint32), m2.view(np.uint32))


def test_constant_colour_on_one_plane_comes_back():
    """Colour 0.5 everywhere on a flat plane: wl = wn = wz = 1 whatever the
    variances, w = h exactly, sc = 0.5 * sw exactly: 0.5 comes back bit for
    bit, also next to starved pixels, which keep their own value."""
    W, H = 37, 23
    _, cn, m2 = dn.random_plane(W, H, 5)
    px = np.full(W * H, 0.5, F)
    px[cn < 2] = F(7.25)
    out, var = dn.denoise(px, cn, m2, _flat_guides(W, H), W, H, iterations=5)
    assert np.array_equal(out.view(np.uint32), px.view(np.uint32))
    assert (cn < 2).any() and (var[cn < 2] == 0).all() and np.isfinite(var).all()


def test_depth_step_stops_the_filter_and_a_flat_plane_does_not():
    """Colour 0.25 | 0.75 with the edge on step_guides' depth step of 0.5,
    sigma_z 0.1, sigma_l 1000 (the colour ramp stops nothing): a tap across
    the step has t = max(1 - 0.5 / 0.1, 0) = 0, so w = 0 exactly; a tap on the
    centre's side has e = 0, wn = wz = wl = 1 and w = h, and with colours of
    two significant bits every product and sum is exact: sc = col * sw and
    the edge comes back bit for bit. The same plane on flat guides is mixed
    across the edge."""
    W, H = 67, 35
    px, cn, m2 = dn.two_level_plane(W, H)
    out, _ = dn.denoise(px, cn, m2, dn.step_guides(W, H), W, H, iterations=4, sigma_l=1000.0)
    assert np.array_equal(out.view(np.uint32), px.view(np.uint32))
    flat, _ = dn.denoise(px, cn, m2, _flat_guides(W, H), W, H, iterations=4, sigma_l=1000.0)
    changed = (flat != px).reshape(H, W)
    assert changed[:, W // 2 - 1].all() and changed[:, W // 2].all()
    assert ((flat > 0.25) & (flat < 0.75))[changed.reshape(-1)].all()


def test_pixels_that_take_no_part_are_copied():
    W, H = 37, 23
    img, m2 = dn.box_plane(W, H)
    g = dn.box_guides(W, H)
    part = dn.participation(img["pixels"], img["counters"], m2, g.reshape(-1))
    assert part.any() and (~part).any()
    assert (g["kind"][H - 1] == 0xff).all() and not part.reshape(H, W)[H - 1].any()
    out, var = dn.denoise(img["pixels"], img["counters"], m2, g, W, H)
    assert np.array_equal(out[~part].view(np.uint32), img["pixels"][~part].view(np.uint32))
    assert np.array_equal(var[~part].view(np.uint32), dn.var0_of(img["counters"], m2)[~part].view(np.uint32))
    assert not np.array_equal(out[part], img["pixels"][part])


def test_denoising_reduces_the_error():
    """Box scene 64 x 48, n_rays 4, depth_max 3, 4 passes, the defaults,
    against the oracle's own 256-pass plane: RMSE over the participating
    pixels below the raw frame's (the ratio is in DESIGN.md "Denoising")."""
    W, H = 64, 48
    img, m2 = dn.box_plane(W, H)
    g = dn.box_guides(W, H)
    p = capi.make_params(W, H, 256, **dn.RENDER)
    vals, codes = oracle_binding.render_values(scenes.make_scene_box(), p)
    ref = oracle_binding.accumulate(vals, codes)["pixels"].astype(np.float64)
    part = dn.participation(img["pixels"], img["counters"], m2, g.reshape(-1))
    out, _ = dn.denoise(img["pixels"], img["counters"], m2, g, W, H)
    raw = np.sqrt(np.mean((img["pixels"][part] - ref[part]) ** 2))
    den = np.sqrt(np.mean((out[part] - ref[part]) ** 2))
    print(f"RMSE raw {raw:.6f} denoised {den:.6f} ratio {den / raw:.4f} over {int(part.sum())} pixels")
    assert den / raw < 1.0


@pytest.mark.parametrize("plane", (dn.GRID, dn.GUI))
@pytest.mark.parametrize("shape", ((13, 11), (1, 1), (1, 7), (7, 1), (2, 3)))
def test_guide_scatter_row_rule(shape, plane):
    import preview_ref
    W, H = shape
    desc = pc.scene("box/up")
    p = capi.make_params(W, H, 1, spp_offset=2, flags=dn.ac.FLAG[plane])
    _, _, kinds, hits, _ = preview_ref.render(desc, p)
    g = dn.scatter_guides(kinds[0], hits[0], plane)
    assert g.dtype.itemsize == 32 and (g["zero"] == 0).all()
    for yd in range(H):
        if plane == dn.GUI:
            ys = H - 1 - yd
        else:
            ys = 0 if H == 1 else (H - 2 - yd if yd <= H - 2 else None)
        if ys is None:
            assert (g["kind"][yd] == 0xff).all() and not g["pos"][yd].any() and not g["normal"][yd].any()
        else:
            assert np.array_equal(g["kind"][yd], kinds[0][ys])
            assert np.array_equal(g["pos"][yd].view(np.uint32), hits[0][ys][:, 0:3].view(np.uint32))
            assert np.array_equal(g["normal"][yd].view(np.uint32), hits[0][ys][:, 3:6].view(np.uint32))


def test_header_binding_and_library_agree():
    hdr = (ROOT / "include" / "ipt_capi.h").read_text()
    assert re.search(r"#define IPT_ABI_VERSION 7\b", hdr) and capi.ABI_VERSION == 7
    with tempfile.TemporaryDirectory() as td:
        src = Path(td) / "sz.c"
        src.write_text('#include <stdio.h>\n#include "ipt_capi.h"\nint main(void) { printf("%zu %zu\\n", '
                       "sizeof(ipt_guide), sizeof(ipt_denoise_params)); return 0; }\n")
        exe = Path(td) / "sz"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
        sizes = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes[0] == 32 == C.sizeof(capi.Guide) == capi.GuideRecord.itemsize
    assert sizes[1] == C.sizeof(capi.DenoiseParams) == 24
    for f, (name, _) in zip(("pos", "kind", "normal", "zero"), capi.Guide._fields_):
        assert f == name and capi.GuideRecord.fields[f][1] == getattr(capi.Guide, f).offset
    new = ("ipt_guides_device", "ipt_guides", "ipt_denoise_device", "ipt_denoise", "ipt_denoise_pass_ms")
    nm = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], check=True, capture_output=True,
                        text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    lib = capi.load()
    for s in new:
        assert re.search(r"^int\s+%s\s*\(" % s, hdr, re.M), s
        assert s in capi.EXPORTED_SYMBOLS and s in exported and hasattr(lib, s)
    assert lib.ipt_abi_version() == 7
