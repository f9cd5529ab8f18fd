"""The denoiser's restatement (tests/denoise_cases.py) without a GPU: it tells
the wrong variants apart on pinned cases, keeps what the filter must keep,
reduces the error of a 4-pass frame against the oracle's own 256-pass plane,
and the header, the binding and the library agree on the new entry points;
on which frames a tap leaves its lattice tile (the seam variants), which
planes leave the windows of the range-free division and root or hold
denormals (the operand census), and that the edge planes do not degenerate.
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


# ---- lattice tiles ---------------------------------------------------------------------------
# pixels whose (colour, variance) differ from the restatement's under ("seam",
# axis, S): dn.random_plane(W, H, 6) on dn.crease_guides, 6 iterations, sigma_l
# 6. Pinned where the frame spans two tiles at that step (dn.spans_two_tiles);
# everywhere else no tap leaves its tile and the variant is the restatement.
SEAM_COUNTS = {
    (300, 75): {("x", 4): (14069, 14417), ("x", 8): (7005, 7104), ("y", 4): (21014, 21022), ("y", 8): (17097, 17205)},
    (1061, 9): {("x", 4): (5242, 5403), ("x", 8): (2111, 2144), ("x", 16): (686, 688), ("x", 32): (247, 247)},
    (9, 277): {("y", 4): (2071, 2081), ("y", 8): (1704, 1711), ("y", 16): (902, 906), ("y", 32): (163, 163)},
    (1061, 277): {("x", 4): (249190, 252906), ("x", 8): (132346, 134745), ("x", 16): (43896, 44058),
                  ("x", 32): (15287, 15301), ("y", 4): (278426, 278477), ("y", 8): (269533, 270053),
                  ("y", 16): (189733, 190293), ("y", 32): (37665, 37706)},
    # the largest frame before SEAM_FRAMES: one tile column from step 8, one tile row from step 16
    (131, 67): {("x", 4): (2855, 2930), ("y", 4): (7976, 7991), ("y", 8): (3376, 3441)},
}


def _seam_counts(W, H):
    """{(axis, S): differing (colour, variance)}; a variant goes on from the
    restatement's own plane before step S, where it first applies."""
    px, cn, m2 = dn.random_plane(W, H, 6)
    g = dn.crease_guides(W, H)
    kw = dict(iterations=6, sigma_l=6.0)
    trace = []
    ref = dn.denoise(px, cn, m2, g, W, H, trace=trace, **kw)
    got = {}
    for axis in "xy":
        for S in dn.SEAM_STEPS:
            k = S.bit_length() - 1
            out = dn.denoise(px, cn, m2, g, W, H, wrong=("seam", axis, S), resume=(k,) + trace[k - 1], **kw)
            got[axis, S] = (int((~dn.same(ref[0], out[0])).sum()), int((~dn.same(ref[1], out[1])).sum()))
    return got


@pytest.mark.parametrize("frame", sorted(SEAM_COUNTS), ids=lambda f: "%dx%d" % f)
def test_dropping_the_taps_of_another_tile_shows_where_a_frame_spans_two(frame):
    W, H = frame
    got = _seam_counts(W, H)
    for (axis, S), n in got.items():
        if dn.spans_two_tiles(W, H, axis, S):
            assert n == SEAM_COUNTS[frame][axis, S] and n[0] > 0, (axis, S, n)
        else:
            assert n == (0, 0) and (axis, S) not in SEAM_COUNTS[frame], (axis, S, n)
    if frame == (131, 67):  # what the frames before SEAM_FRAMES could not see
        assert got["x", 8] == got["x", 16] == got["y", 16] == (0, 0)
    else:
        assert frame in dn.SEAM_FRAMES


def test_resuming_a_trace_is_the_whole_run():
    W, H = 67, 35
    px, cn, m2 = dn.random_plane(W, H, 6)
    g = dn.crease_guides(W, H)
    trace = []
    ref = dn.denoise(px, cn, m2, g, W, H, iterations=4, sigma_l=6.0, trace=trace)
    assert len(trace) == 4 and np.array_equal(trace[3][0].reshape(-1).view(np.uint32), ref[0].view(np.uint32))
    for wrong in (None, ("seam", "y", 4)):
        whole = dn.denoise(px, cn, m2, g, W, H, iterations=4, sigma_l=6.0, wrong=wrong)
        part = dn.denoise(px, cn, m2, g, W, H, iterations=4, sigma_l=6.0, wrong=wrong, resume=(2,) + trace[1])
        assert dn.same(whole[0], part[0]).all() and dn.same(whole[1], part[1]).all()
    assert not dn.same(whole[0], ref[0]).all()


# ---- values outside the window ---------------------------------------------------------------
# dn.denoise's census of each dn.EDGE_CASES plane, 67 x 35: per operation
# (evaluations, with an operand outside the window of ipt_math.h's range-free
# division / root, with a denormal operand or result)
EDGE_CENSUS = {
    "colour_e-70": {"var0": (2214, 2205, 2205), "e/sigma_z": (138672, 0, 0), "dc/den": (138672, 132030, 0),
                    "sc/sw": (6642, 6642, 0), "sv/sw2": (6642, 155, 155), "sqrt": (6642, 2088, 2088)},
    "colour_e-64": {"var0": (2214, 2214, 2214), "e/sigma_z": (138672, 0, 0), "dc/den": (138672, 132030, 0),
                    "sc/sw": (6642, 6642, 0), "sv/sw2": (6642, 6642, 6642), "sqrt": (6642, 6642, 6642)},
    "colour_e-50": {"var0": (2214, 2214, 0), "e/sigma_z": (138672, 0, 0), "dc/den": (138672, 132030, 0),
                    "sc/sw": (6642, 6642, 0), "sv/sw2": (6642, 6642, 0), "sqrt": (6642, 6642, 0)},
    "colour_e45": {"var0": (2214, 2214, 0), "e/sigma_z": (138672, 0, 0), "dc/den": (138672, 138672, 0),
                   "sc/sw": (6642, 5509, 0), "sv/sw2": (6642, 6642, 0), "sqrt": (6642, 0, 0)},
    "colour_e63": {"var0": (2214, 2214, 0), "e/sigma_z": (138672, 0, 0), "dc/den": (138672, 138672, 0),
                   "sc/sw": (6642, 6642, 0), "sv/sw2": (6642, 6642, 0), "sqrt": (6642, 0, 0)},
    "colour_e-70_it1": {"var0": (2214, 2205, 2205), "e/sigma_z": (49682, 0, 0), "dc/den": (49682, 47468, 0),
                        "sc/sw": (2214, 2214, 0), "sv/sw2": (2214, 155, 155), "sqrt": (2214, 2082, 2082)},
    "colour_e-64_it5": {"var0": (2214, 2214, 2214), "e/sigma_z": (188016, 0, 0), "dc/den": (188016, 176946, 0),
                        "sc/sw": (11070, 11070, 0), "sv/sw2": (11070, 7376, 7376), "sqrt": (11070, 9565, 9565)},
    "colour_e63_it5": {"var0": (2214, 2214, 0), "e/sigma_z": (188016, 0, 0), "dc/den": (188016, 188016, 0),
                       "sc/sw": (11070, 11070, 0), "sv/sw2": (11070, 11070, 0), "sqrt": (11070, 0, 0)},
    "world_e-140": {"var0": (2214, 0, 0), "e/sigma_z": (138672, 138672, 138672), "dc/den": (138672, 0, 0),
                    "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
    "world_e-120": {"var0": (2214, 0, 0), "e/sigma_z": (138672, 138672, 0), "dc/den": (138672, 0, 0),
                    "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
    "world_e-45": {"var0": (2214, 0, 0), "e/sigma_z": (138672, 138672, 0), "dc/den": (138672, 0, 0),
                   "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
    "world_e45": {"var0": (2214, 0, 0), "e/sigma_z": (138672, 138672, 0), "dc/den": (138672, 0, 0),
                  "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
    "world_e60": {"var0": (2214, 0, 0), "e/sigma_z": (138672, 138672, 0), "dc/den": (138672, 0, 0),
                  "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
    "sigma_l_inf": {"var0": (2214, 0, 0), "e/sigma_z": (138672, 0, 0), "dc/den": (138672, 138672, 0),
                    "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
    "sigma_l_3e38": {"var0": (2214, 0, 0), "e/sigma_z": (138672, 0, 0), "dc/den": (138672, 138672, 77350),
                     "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
    "sigma_l_1e-45": {"var0": (2214, 0, 0), "e/sigma_z": (138672, 0, 0), "dc/den": (138672, 0, 0),
                      "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
    "sigma_z_inf": {"var0": (2214, 0, 0), "e/sigma_z": (138672, 138672, 0), "dc/den": (138672, 0, 0),
                    "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
    "sigma_z_3e38": {"var0": (2214, 0, 0), "e/sigma_z": (138672, 138672, 4725), "dc/den": (138672, 0, 0),
                     "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
    "sigma_z_1e-45": {"var0": (2214, 0, 0), "e/sigma_z": (138672, 138672, 138672), "dc/den": (138672, 0, 0),
                      "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
    "normal_e-30_pow0": {"var0": (2214, 0, 0), "e/sigma_z": (138672, 0, 0), "dc/den": (138672, 0, 0),
                         "sc/sw": (6642, 6642, 0), "sv/sw2": (6642, 6642, 6642), "sqrt": (6642, 0, 0)},
    "normal_e10_pow0": {"var0": (2214, 0, 0), "e/sigma_z": (138672, 0, 0), "dc/den": (138672, 0, 0),
                        "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
    "normal_e-32_pow1": {"var0": (2214, 0, 0), "e/sigma_z": (138672, 0, 0), "dc/den": (138672, 88990, 0),
                         "sc/sw": (2214, 2214, 2214), "sv/sw2": (2214, 2214, 0), "sqrt": (6642, 4428, 0)},
    "counters_2p24": {"var0": (2214, 2214, 0), "e/sigma_z": (138672, 0, 0), "dc/den": (138672, 0, 0),
                      "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
    "counters_2p31": {"var0": (2214, 2214, 0), "e/sigma_z": (138672, 0, 0), "dc/den": (138672, 0, 0),
                      "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
    "counters_mix": {"var0": (2214, 1652, 0), "e/sigma_z": (138672, 0, 0), "dc/den": (138672, 0, 0),
                     "sc/sw": (6642, 0, 0), "sv/sw2": (6642, 0, 0), "sqrt": (6642, 0, 0)},
}
# what each plane is there for: (operation, 1 = outside the window / 2 = denormal).
# normal_e10_pow0 is there for weights of about 2^20, which stay inside every
# window, and sigma_l_1e-45 for a ramp of 2^-20 that stops nearly every tap.
EDGE_THERE_FOR = {
    "colour_e-70": (("sqrt", 2), ("var0", 2)), "colour_e-64": (("sv/sw2", 2), ("sqrt", 2)),
    "colour_e-50": (("sqrt", 1),), "colour_e45": (("dc/den", 1), ("sc/sw", 1)),
    "colour_e63": (("dc/den", 1), ("sc/sw", 1)), "colour_e-70_it1": (("sqrt", 2), ("sv/sw2", 2)),
    "colour_e-64_it5": (("sv/sw2", 2), ("sqrt", 2)), "colour_e63_it5": (("dc/den", 1), ("sc/sw", 1)),
    "world_e-140": (("e/sigma_z", 2),), "world_e-120": (("e/sigma_z", 1),), "world_e-45": (("e/sigma_z", 1),),
    "world_e45": (("e/sigma_z", 1),), "world_e60": (("e/sigma_z", 1),),
    "sigma_l_inf": (("dc/den", 1),), "sigma_l_3e38": (("dc/den", 1),), "sigma_l_1e-45": (),
    "sigma_z_inf": (("e/sigma_z", 1),), "sigma_z_3e38": (("e/sigma_z", 1),), "sigma_z_1e-45": (("e/sigma_z", 2),),
    "normal_e-30_pow0": (("sv/sw2", 2),), "normal_e10_pow0": (), dn.EDGE_OVERFLOW: (("sc/sw", 2), ("sv/sw2", 1)),
    "counters_2p24": (("var0", 1),), "counters_2p31": (("var0", 1),), "counters_mix": (("var0", 1),),
}
# the census of box_plane(131, 67) on box_guides, 6 iterations, the defaults:
# a rendered plane does leave the windows (dark pixels with tiny variances)
BOX_CENSUS_131x67 = {"var0": (8646, 0, 0), "e/sigma_z": (656808, 0, 0), "dc/den": (656808, 634, 0),
                     "sc/sw": (37116, 252, 0), "sv/sw2": (37116, 880, 16), "sqrt": (37116, 8, 5)}
# pixels whose (colour, variance) differ from the restatement's under each
# dn.WRONG_EDGES variant, by plane; "random" is dn.random_plane(67, 35, 3) on
# crease guides, 3 iterations, sigma_l 6. At 2^-70 every variance is 0 after
# two iterations and den is 2^-20 whatever the root: three iterations cannot
# show a flushed denormal there, one iteration does.
WRONG_EDGES_COUNTS = {
    "daz": {"random": (0, 0), "colour_e-64": (0, 2214), "colour_e-70": (0, 0), "colour_e-70_it1": (0, 155),
            "sigma_z_1e-45": (2214, 2214), "world_e-140": (2214, 2214), "normal_e-30_pow0": (2213, 2214)},
    "signed_counter": {"random": (0, 0), "counters_2p24": (0, 0), "counters_2p31": (2214, 2214),
                       "counters_mix": (2214, 2214)},
}


def _edge(name):
    if name == "random":
        return dn.random_plane(67, 35, dn.EDGE_SEED) + (dn.crease_guides(67, 35), dict(iterations=3, sigma_l=6.0))
    return dn.edge_case(name)


@pytest.mark.parametrize("name", dn.EDGE_CASES)
def test_edge_planes_leave_the_windows_and_do_not_degenerate(name):
    W, H = 67, 35
    px, cn, m2, g, kw = dn.edge_case(name)
    census = {}
    out, var = dn.denoise(px, cn, m2, g, W, H, census=census, **kw)
    plain = dn.denoise(px, cn, m2, g, W, H, **kw)  # the census changes no result
    assert dn.same(out, plain[0]).all() and dn.same(var, plain[1]).all()
    assert np.array_equal(dn.var0_of(cn, m2, census={}).view(np.uint32), dn.var0_of(cn, m2).view(np.uint32))
    assert {k: tuple(v) for k, v in census.items()} == EDGE_CENSUS[name]
    for op, column in EDGE_THERE_FOR[name]:
        assert census[op][column] >= 100, (op, column)
    part = dn.participation(px, cn, m2, g.reshape(-1))
    n = int(part.sum())
    assert n == 2214
    changed = int((~dn.same(out, px))[part].sum())
    bad = int((~(np.isfinite(out) & np.isfinite(var)))[part].sum())
    if name == dn.EDGE_OVERFLOW:  # sv / 0 on every pixel: no variance is finite, every colour is
        assert changed == n and np.isfinite(out).all() and not np.isfinite(var[part]).any()
    elif name == "sigma_l_1e-45":
        assert changed == 199 and bad == 0
    else:
        assert 2 * changed >= n and 10 * bad <= n, (changed, bad)


def test_the_planes_before_the_edge_planes_stay_inside_every_window():
    """dn.random_plane and dn.two_level_plane: no operand of the six operations
    is outside its window and none is denormal. The rendered box plane has
    some of each; pinned."""
    W, H = 67, 35
    for (px, cn, m2), g in ((dn.random_plane(W, H, 5), dn.crease_guides(W, H)),
                            (dn.random_plane(W, H, 3), dn.step_guides(W, H)),
                            (dn.two_level_plane(W, H), dn.step_guides(W, H))):
        census = {}
        dn.denoise(px, cn, m2, g, W, H, iterations=5, sigma_l=6.0, census=census)
        assert set(census) == set(dn.OPS)
        for op, (n, outside, denormal) in census.items():
            assert n > 2000 and outside == 0 and denormal == 0, op
    W, H = 131, 67
    img, m2 = dn.box_plane(W, H)
    census = {}
    dn.denoise(img["pixels"], img["counters"], m2, dn.box_guides(W, H), W, H, iterations=6, census=census)
    assert {k: tuple(v) for k, v in census.items()} == BOX_CENSUS_131x67


@pytest.mark.parametrize("wrong,name", [(w, n) for w in dn.WRONG_EDGES for n in WRONG_EDGES_COUNTS[w]])
def test_restatement_differs_from_each_edge_variant(wrong, name):
    px, cn, m2, g, kw = _edge(name)
    ref = dn.denoise(px, cn, m2, g, 67, 35, **kw)
    out = dn.denoise(px, cn, m2, g, 67, 35, wrong=wrong, **kw)
    got = (int((~dn.same(ref[0], out[0])).sum()), int((~dn.same(ref[1], out[1])).sum()))
    assert got == WRONG_EDGES_COUNTS[wrong][name]


def test_counter_planes_round_and_pass_two_to_the_31():
    for key, vals in dn.COUNTER_SETS.items():
        px, cn, m2 = dn.counter_plane(67, 35, dn.EDGE_SEED, vals)
        assert set(np.unique(cn)) == set(vals) | {1}
        v0 = dn.var0_of(cn, m2)
        assert np.isfinite(v0).all() and (v0[cn >= 2] < 0.25).all() and np.median(v0[cn >= 2]) > 0.05
    assert np.float32(np.uint32(2 ** 24 + 1)) == 2 ** 24 and np.float32(np.uint32(2 ** 32 - 1)) == 2 ** 32


def test_guides_that_are_no_numbers_stay_local():
    """NaN (quiet and signalling) and infinite positions and NaN normals: every
    tap of the pixel, its own included, has weight 0, so it keeps its colour;
    nothing beyond the filter's reach 2 (2^iterations - 1) changes; and with
    no infinite normal every colour stays finite. An infinite normal makes
    NaN (inf * 0) on its pixel and the taps that reach it, nowhere else."""
    W, H = 67, 35
    px, cn, m2 = dn.random_plane(W, H, dn.EDGE_SEED)
    g0 = dn.crease_guides(W, H)
    part0 = dn.participation(px, cn, m2, g0.reshape(-1))
    # (three iterations reach 14 pixels and leave 18 of this frame's out of reach, two reach 6)
    for it, infinite_normals in ((3, False), (3, True), (2, False), (2, True)):
        kw = dict(iterations=it, sigma_l=6.0)
        clean = dn.denoise(px, cn, m2, g0, W, H, **kw)
        r = 2 * (2 ** it - 1)
        g, where, kinds = dn.poisoned_guides(g0, part0, infinite_normals)
        assert len(where) == (6 if infinite_normals else 4) and len(kinds) == 6
        assert g["pos"].view(np.uint32).reshape(-1, 3)[where["pos_snan"], 1] == 0x7f800001
        part = dn.participation(px, cn, m2, g.reshape(-1))
        assert {k: bool(part[i]) for i, k in kinds.items()} == {0: False, 2: False, 3: False, 0x81: True, 0xfd: True,
                                                                 0xfe: False}
        assert part[list(where.values())].all()
        out, var = dn.denoise(px, cn, m2, g, W, H, **kw)
        kept = [where[k] for k in ("pos_nan", "pos_snan", "normal_nan", "pos_inf")]
        assert np.array_equal(out[kept].view(np.uint32), px[kept].view(np.uint32))
        far = ~dn.reach(W, H, list(where.values()) + list(kinds), r)
        assert far.sum() >= (18 if it == 3 else 300) and dn.same(out, clean[0])[far].all() and dn.same(var, clean[1])[far].all()
        assert not dn.same(out, clean[0]).all()
        if infinite_normals:
            inf_at = [where["normal_pinf"], where["normal_ninf"]]
            assert np.isnan(out[inf_at]).all()
            assert np.isfinite(out[~dn.reach(W, H, inf_at, r)]).all()
        else:
            assert np.isfinite(out).all()
