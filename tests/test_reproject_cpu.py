"""Temporal reprojection's restatement (tests/reproject_cases.py) without a
GPU: it tells the wrong variants apart on pinned cases (and does not where
that is the point), keeps the invariants of the contract, buys what it is
for -- a frame continued from reprojected history is closer to the oracle's
own 256-pass plane than the same passes from zero -- and the header, the
binding and the library agree on the new entry points. Oracle and preview
restatement only."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from ipt_amd import capi, scenes

import adaptive_cases as ac
import denoise_cases as dn
import drift_cases as dc
import oracle_binding
import reproject_cases as rc

ROOT = Path(__file__).resolve().parents[1]
F = np.float32

# pixels whose (mean, counter, m2) differ from the restatement's, 37 x 23, 4
# passes, Grid map, the defaults, the previous camera of the move "shift"
WRONG_BOX_SHIFT = {
    "dx_outer": (57, 0, 37),
    "unsquared_var": (0, 0, 534),
    "nearest": (525, 82, 525),
    "no_half": (540, 55, 538),
    "unit_direction": (0, 0, 0),   # the box camera's direction has length 1
    "grid_as_gui": (540, 57, 541),
    "source_index": (527, 427, 526),
    "no_cap": (0, 0, 0),           # no counter reaches the default cap of 64
    "signed_counter": (0, 0, 0),   # nor 2^31
}
# the scene whose camera direction has length 2
WRONG_SQUARE_SHIFT_UNIT_DIRECTION = (113, 10, 113)
# max_count 2: every history is capped
WRONG_BOX_SHIFT_NO_CAP_AT_2 = (0, 550, 534)
# the poisoned crease planes (counters of 2^31 and 2^32 - 1 among them), 67 x 35
WRONG_POISONED_CREASE = {"signed_counter": (35, 34, 35), "no_cap": (0, 51, 51)}
STATS_37x23 = {  # (move, plane): reused, disoccluded, not_surface
    ("same", rc.GRID): (575, 0, 276), ("same", rc.GUI): (612, 0, 239),
    ("shift", rc.GRID): (550, 25, 276), ("shift", rc.GUI): (585, 27, 239),
    ("turn", rc.GRID): (522, 53, 276), ("turn", rc.GUI): (555, 57, 239),
    ("behind", rc.GRID): (0, 575, 276), ("behind", rc.GUI): (1, 611, 239),
    ("far", rc.GRID): (226, 349, 276), ("far", rc.GUI): (244, 368, 239),
}


def _run(case, W, H, plane=rc.GRID, **kw):
    return rc.reproject(*case[:5], W, H, case[5], plane, **kw)


@pytest.mark.parametrize("wrong", rc.WRONG)
def test_restatement_differs_from_each_wrong_variant(oracle, wrong):
    W, H = 37, 23
    case = rc.rendered_case("box", "shift", W, H)
    assert rc.differ(_run(case, W, H), _run(case, W, H, wrong=wrong)) == WRONG_BOX_SHIFT[wrong]


def test_a_direction_of_length_two_tells_unit_direction_apart(oracle):
    W, H = 37, 23
    case = rc.rendered_case("square", "shift", W, H)
    d = np.array(case[5]["direction"], F)
    assert abs(float(np.sqrt((d.astype(np.float64) ** 2).sum())) - 2.0) < 1e-6
    assert rc.differ(_run(case, W, H), _run(case, W, H, wrong="unit_direction")) == WRONG_SQUARE_SHIFT_UNIT_DIRECTION


def test_the_gui_map_is_its_own_wrong_variant(oracle):
    W, H = 37, 23
    case = rc.rendered_case("box", "shift", W, H, rc.GUI)
    assert rc.differ(_run(case, W, H, rc.GUI), _run(case, W, H, rc.GUI, wrong="grid_as_gui")) == (0, 0, 0)


def test_the_cap_and_the_counter_type_show_where_counters_are_large(oracle):
    W, H = 37, 23
    case = rc.rendered_case("box", "shift", W, H)
    assert rc.differ(_run(case, W, H, max_count=2), _run(case, W, H, max_count=2, wrong="no_cap")) == \
        WRONG_BOX_SHIFT_NO_CAP_AT_2
    W, H = 67, 35
    case = rc.poisoned(rc.synthetic_case("crease", W, H), W, H)
    for wrong, pinned in WRONG_POISONED_CREASE.items():
        assert rc.differ(_run(case, W, H), _run(case, W, H, wrong=wrong)) == pinned, wrong


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("move", tuple(rc.BOX_MOVES))
def test_classes_and_invariants(oracle, move, plane):
    """Stats sum to W * H, empty pixels are exact zeros, c' lies within
    [2, max_count], and the classes are the pinned ones (behind: t <= 0
    everywhere; far: part of the frame has no history)."""
    W, H = 37, 23
    case = rc.rendered_case("box", move, W, H, plane)
    for mc in (2, 16, 1 << 24):
        px, cn, m2, stats, cls = _run(case, W, H, plane, max_count=mc)
        assert tuple(int(s) for s in stats[:3]) == STATS_37x23[move, plane] and stats[3] == 0
        assert int(stats.sum()) == W * H
        empty = cls != rc.REUSED
        assert not dc.bits(px)[empty].any() and not cn[empty].any() and not dc.bits(m2)[empty].any()
        if (~empty).any():
            assert cn[~empty].min() >= 2 and cn[~empty].max() <= mc
            assert np.isfinite(px[~empty]).all() and np.isfinite(m2[~empty]).all()
    if plane == rc.GRID:  # the Grid map's row H-1 has no nominal source
        assert (cls.reshape(H, W)[H - 1] == rc.NOT_SURFACE).all()


@pytest.mark.parametrize("plane", ac.PLANES)
def test_identity_camera_reuses_every_participating_pixel(oracle, plane):
    W, H = 64, 48
    case = rc.rendered_case("box", "same", W, H, plane)
    assert case[3] is case[4] or np.array_equal(case[3].view(np.uint8), case[4].view(np.uint8))
    part = dn.participation(case[0], case[1], case[2], case[3].reshape(-1))
    px, cn, m2, stats, cls = _run(case, W, H, plane)
    assert part.sum() > W * H // 2 and (cls[part] == rc.REUSED).all()
    assert stats[1] == 0  # every surface pixel has itself among its taps


def test_normal_min_of_infinity_reuses_nothing(oracle):
    W, H = 37, 23
    case = rc.rendered_case("box", "shift", W, H)
    stats = _run(case, W, H, normal_min=float("inf"))[3]
    assert stats[0] == 0 and stats[1] == 575
    assert _run(case, W, H, normal_min=-1.0)[3][0] >= _run(case, W, H, normal_min=0.9)[3][0] > 0


@pytest.mark.parametrize("guides", ("crease", "step"))
def test_poison_stays_where_it_is(guides):
    """NaN and infinite pixels and m2, counters 0, 1, 2^24 + 1, 2^31 and
    2^32 - 1, kinds of every kind & 3 and guides that are no numbers: every
    output is finite, the classes still sum to the frame."""
    W, H = 67, 35
    clean = rc.synthetic_case(guides, W, H)
    case = rc.poisoned(clean, W, H)
    px, cn, m2, stats, cls = _run(case, W, H)
    assert int(stats.sum()) == W * H and stats[2] > 0 and stats[1] > 0
    assert np.isfinite(px).all() and np.isfinite(m2).all()
    assert cn[cls == rc.REUSED].min() >= 2 and cn.max() <= rc.DEFAULTS["max_count"]
    assert rc.differ(_run(clean, W, H), (px, cn, m2)) != (0, 0, 0)


def test_reprojected_history_reduces_the_error(oracle):
    """Box scene 64 x 48, n_rays 4, depth_max 3: 16 passes at camera A (the
    move "shift"), reprojected to the scene's camera B and continued with 2
    passes at B, against the same 2 passes at B from zero; RMSE against the
    oracle's own 256-pass plane at B over the reused pixels (the ratio is in
    DESIGN.md "Temporal reprojection"). The move reuses 2052 of B's 2149
    surface pixels."""
    W, H = 64, 48
    case = rc.rendered_case("box", "shift", W, H, rc.GRID, spp=16)
    px, cn, m2, stats, cls = _run(case, W, H)
    surface = int(stats[0] + stats[1])
    assert (int(stats[0]), surface) == (2052, 2149) and 2 * int(stats[0]) >= surface
    p = capi.make_params(W, H, 2, spp_offset=16, **rc.RENDER)
    vals, codes = (np.asarray(a) for a in oracle_binding.render_values(scenes.make_scene_box(), p))
    img = dc.plane(W, H)
    img["pixels"][:], img["counters"][:] = px, cn
    cont, _ = ac.replay(vals, codes, None, rc.GRID, img=img, m2=m2.copy())
    fresh, _ = ac.replay(vals, codes, None, rc.GRID)
    p = capi.make_params(W, H, 256, **rc.RENDER)
    v, c = oracle_binding.render_values(scenes.make_scene_box(), p)
    ref = oracle_binding.accumulate(v, c)["pixels"].astype(np.float64)
    m = cls == rc.REUSED
    e_cont = np.sqrt(np.mean((cont["pixels"][m] - ref[m]) ** 2))
    e_fresh = np.sqrt(np.mean((fresh["pixels"][m] - ref[m]) ** 2))
    print(f"RMSE continued {e_cont:.6f} fresh {e_fresh:.6f} ratio {e_cont / e_fresh:.4f} over {int(m.sum())} pixels")
    assert e_cont / e_fresh < 1.0


def test_header_binding_and_library_agree():
    hdr = (ROOT / "include" / "ipt_capi.h").read_text()
    assert re.search(r"#define IPT_ABI_VERSION 7\b", hdr) and capi.ABI_VERSION == 7
    fields = ("width", "height", "flags", "prev_camera", "sigma_z", "normal_min", "max_count")
    with tempfile.TemporaryDirectory() as td:
        src = Path(td) / "sz.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ipt_capi.h"\nint main(void) { '
                       'printf("%zu", sizeof(ipt_reproject_params));\n' +
                       "".join('printf(" %%zu", offsetof(ipt_reproject_params, %s));\n' % f for f in fields) +
                       "return 0; }\n")
        exe = Path(td) / "sz"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
        sizes = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes[0] == C.sizeof(capi.ReprojectParams) == 72
    assert [n for n, _ in capi.ReprojectParams._fields_] == list(fields)
    assert sizes[1:] == [getattr(capi.ReprojectParams, f).offset for f in fields]
    rp = capi.make_reproject_params(5, 7, scenes.box_camera(), flags=capi.IPT_FLAG_GUI_PLANE)
    assert (rp.width, rp.height, rp.flags, rp.max_count) == (5, 7, 2, capi.REPROJECT_DEFAULTS["max_count"])
    assert list(rp.prev_camera.up) == [float(F(v)) for v in scenes.box_camera()["up"]]
    new = ("ipt_reproject_device", "ipt_reproject")
    nm = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], check=True, capture_output=True,
                        text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    lib = capi.load()
    for s in new:
        assert re.search(r"^int\s+%s\s*\(" % s, hdr, re.M), s
        assert s in capi.EXPORTED_SYMBOLS and s in exported and hasattr(lib, s)
    assert lib.ipt_abi_version() == 7
