"""Temporal reprojection's definition on its exact comparisons, without a
GPU: a dyadic lattice (tests/reproject_cases.py lattice_case) on which fx and
fy are whole, half and quarter pixels, the plane distance equals sigma_z, n.n_q
equals normal_min and counters equal the cap; the same lattice moved by one and
two ulp; cameras at the ends of step 2; one- and two-pixel frames. The
vectorised restatement equals a second one written pixel by pixel from the
header; a census counts how often each comparison lands on equality (and did
not, but at the cap, on the earlier suites' cases); each device-side slip of WRONG_EDGES shows
on a pinned case and the slips no input can show are shown to show nowhere; the
contract's invariants hold, with out_m2 = +inf where the definition overflows.
tests/test_gpu_reproject_edges.py runs the same cases through the kernel."""
import numpy as np
import pytest

import adaptive_cases as ac
import drift_cases as dc
import reproject_cases as rc

F = np.float32
SHIFTS = tuple(name for name, _ in rc.LATTICE_SHIFTS)
SCALAR_PIXELS = 2500  # reproject_scalar's frames
TINY_SHIFTS = ((0.0, 0.0), (0.5, 0.5), (-0.5, -0.5), (0.0, -1.0))


def _params(mc=rc.LATTICE["max_count"]):
    return dict(rc.LATTICE, max_count=mc)


def edge_cases(plane):
    """(name, case, W, H, params) of every edge case of one row map."""
    for w, h in rc.LATTICE_FRAMES:
        for shift in SHIFTS:
            for mc in rc.LATTICE_MAX_COUNTS:
                yield ("lattice", w, h, shift, mc), rc.lattice_case(w, h, shift, plane, max_count=mc), w, h, _params(mc)
    for w, h in rc.NEAR_FRAMES:
        for shift in SHIFTS:
            for mc in (16, 2) if w * h <= SCALAR_PIXELS else (16,):
                yield (("near", w, h, shift, mc), rc.near_lattice_case(w, h, shift, plane, max_count=mc), w, h,
                       _params(mc))
    W, H = 32, 16
    for name, cam in rc.camera_edge_cases(W, H).items():
        yield ("camera", name), rc.lattice_case(W, H, "quarter_xy", plane)[:5] + (cam,), W, H, _params()
    for w, h in rc.TINY_LATTICE_FRAMES:
        for shift in TINY_SHIFTS:
            yield ("tiny", w, h, shift), rc.constant_lattice_case(w, h, shift, plane), w, h, _params()


def _run(case, W, H, plane, **kw):
    return rc.reproject(*case[:5], W, H, case[5], plane, **kw)


# ---- the second restatement ------------------------------------------------------------------
@pytest.mark.parametrize("plane", ac.PLANES)
def test_scalar_restatement_equals_the_vectorised_one(plane):
    """Bit for bit on the three planes, the stats and the classes, on every
    edge case of at most SCALAR_PIXELS pixels (all but the near-lattice at
    131 x 67): every shift at every cap on both lattice frames, the
    near-lattice at caps 16 and 2, the cameras, the tiny frames. Where the
    vectorised one hides its dead lanes, the header's steps read one pixel at
    a time agree."""
    ran = 0
    for name, case, W, H, par in edge_cases(plane):
        if W * H > SCALAR_PIXELS:
            continue
        ref, got = _run(case, W, H, plane, **par), rc.reproject_scalar(*case[:5], W, H, case[5], plane, **par)
        assert rc.differ(ref, got) == (0, 0, 0), name
        assert ref[3].tolist() == got[3].tolist() and np.array_equal(ref[4], got[4]), name
        ran += 1
    assert ran == 243  # 126 lattice, 84 near-lattice, 9 cameras, 24 tiny


# ---- the census ------------------------------------------------------------------------------
# the events of rc.EVENTS over the lattice at max_count 16, the near-lattice and
# the camera cases of one row map
CENSUS = {
    rc.GRID: {
        't == 0': 480, 't not finite': 1920, 'fx == -1': 47, 'fy == -1': 47, 'fx == W': 77, 'fy == H': 195,
        'tx == 0': 43295, 'ty == 0': 41730, 'x0 == -1': 1278, 'y0 == -1': 2165, 'x0 == W-1': 955,
        'tap on Grid source row H-1': 5245, 'e == sigma_z': 102765, 'n.n_q == normal_min': 89744,
        'c_q == max_count': 25161, 'c_q > max_count': 158620, 'c_q >= 2^24': 107510,
        'used tap with bw == 0': 66258, 'a tap passed yet sw == 0': 18130, 'denormal sv term': 18388,
        'cf within an ulp of an integer': 88105, "c' == 2": 9037, "c' == max_count": 68433,
        'out_m2 not finite': 1866, 'denormal out_m2': 5657,
    },
    rc.GUI: {
        't == 0': 512, 't not finite': 2048, 'fx == -1': 48, 'fy == -1': 45, 'fx == W': 74, 'fy == H': 329,
        'tx == 0': 44091, 'ty == 0': 42249, 'x0 == -1': 1344, 'y0 == -1': 2112, 'x0 == W-1': 984,
        'e == sigma_z': 106372, 'n.n_q == normal_min': 89860, 'c_q == max_count': 28065,
        'c_q > max_count': 159226, 'c_q >= 2^24': 105474, 'used tap with bw == 0': 67999,
        'a tap passed yet sw == 0': 18946, 'denormal sv term': 18927, 'cf within an ulp of an integer': 88094,
        "c' == 2": 9822, "c' == max_count": 67767, 'out_m2 not finite': 1482, 'denormal out_m2': 5679,
    },
}


def _census(cases, plane):
    total = {}
    for _, case, W, H, par in cases:
        for k, v in rc.census(case, W, H, plane, **par).items():
            total[k] = total.get(k, 0) + v
    return total


@pytest.mark.parametrize("plane", ac.PLANES)
def test_every_event_occurs_on_the_edge_cases(plane):
    cases = [c for c in edge_cases(plane) if c[0][0] == "camera" or (c[0][0] == "near" and c[0][4] == 16) or
             (c[0][0] == "lattice" and c[0][1:3] == (32, 16) and c[0][4] == 16)]
    total = _census(cases, plane)
    print(plane, total)
    assert set(total) == set(rc.EVENTS) - set(rc.GRID_ONLY_EVENTS if plane == rc.GUI else ())
    assert all(v > 0 for v in total.values()), total
    assert total == CENSUS[plane]


# events that are equalities of the definition's comparisons: none occurs on a
# case of the earlier suites (DESIGN.md 4.18 has the whole table). The cap is
# not among them: test_cap_and_normal_bound's poisoned crease planes at
# max_count 2, 16 and 1 << 24 do meet c_q == max_count and c' == max_count.
EQUALITIES = ("t == 0", "fx == -1", "fy == -1", "fx == W", "fy == H", "tx == 0", "a tap passed yet sw == 0",
              "e == sigma_z", "n.n_q == normal_min", "denormal sv term", "out_m2 not finite", "denormal out_m2")
EARLIER = {
    't == 0': 0, 't not finite': 0, 'fx == -1': 0, 'fy == -1': 0, 'fx == W': 0, 'fy == H': 0, 'tx == 0': 0,
    'ty == 0': 536, 'x0 == -1': 1249, 'y0 == -1': 0, 'x0 == W-1': 633, 'tap on Grid source row H-1': 351,
    'e == sigma_z': 0, 'n.n_q == normal_min': 0, 'c_q == max_count': 2243, 'c_q > max_count': 18031,
    'c_q >= 2^24': 605, 'used tap with bw == 0': 988, 'a tap passed yet sw == 0': 0, 'denormal sv term': 0,
    'cf within an ulp of an integer': 82267, "c' == 2": 7412, "c' == max_count": 5593, 'out_m2 not finite': 0,
    'denormal out_m2': 0,
}


def earlier_cases(plane):
    """(name, case, W, H, params) of every case tests/test_gpu_reproject.py
    runs on one row map: the synthetic cases clean and poisoned, the rendered
    box frames, every camera move, the poisoned rendered planes, and (Grid
    map only) test_cap_and_normal_bound's two cases at its nine parameter
    pairs."""
    for guides in ("crease", "step"):
        clean = rc.synthetic_case(guides, 67, 35)
        yield guides, clean, 67, 35, {}
        yield guides, rc.poisoned(clean, 67, 35), 67, 35, {}
    for W, H in rc.FRAMES + rc.TINY_FRAMES + (rc.BLOCK_FRAME,):
        yield "box", rc.rendered_case("box", "shift", W, H, plane), W, H, {}
    for scene, moves in (("box", rc.BOX_MOVES), ("square", rc.SQUARE_MOVES)):
        for move in moves:
            yield scene, rc.rendered_case(scene, move, 64, 48, plane), 64, 48, {}
    yield "poisoned", rc.poisoned(rc.rendered_case("box", "turn", 131, 67, plane), 131, 67), 131, 67, {}
    if plane == rc.GRID:
        for mc in (2, 16, 1 << 24):
            for nmin in (-1.0, 0.9, float("inf")):
                par = dict(max_count=mc, normal_min=nmin)
                yield "cap", rc.rendered_case("box", "shift", 37, 23), 37, 23, par
                yield "cap", rc.poisoned(rc.synthetic_case("crease", 67, 35), 67, 35), 67, 35, par


def test_census_of_the_earlier_suites_cases(oracle):
    """What tests/test_gpu_reproject.py runs, counted over both row maps."""
    total = {}
    for plane in ac.PLANES:
        for k, v in _census(earlier_cases(plane), plane).items():
            total[k] = total.get(k, 0) + v
    print("earlier suites:", total)
    assert [k for k in EQUALITIES if total[k]] == []
    assert total == EARLIER


# ---- the slips -------------------------------------------------------------------------------
# variant: (builder, W, H, shift, plane, max_count), then the pixels whose
# (mean, counter, m2) differ from the restatement's and the pixels whose class does
WRONG_EDGES_SHOW = {
    "trunc_floor": (("near", 37, 23, "quarter_xy", rc.GRID, 1 << 24), ((46, 30, 38), 13)),
    "contracted": (("near", 37, 23, "quarter_xy", rc.GUI, 1 << 24), ((53, 11, 45), 0)),
    "strict_sigma": (("lattice", 32, 16, "half_xy", rc.GUI, 16), ((253, 158, 223), 81)),
    "strict_normal": (("lattice", 32, 16, "half_xy", rc.GRID, 16), ((231, 147, 181), 81)),
    "cap_strict": (("lattice", 32, 16, "half_xy", rc.GRID, 16), ((0, 323, 290), 0)),
    "round_counter": (("lattice", 32, 16, "half_xy", rc.GUI, 16), ((0, 86, 80), 0)),
    "grid_last_row": (("near", 37, 23, "whole_xy", rc.GRID, 2), ((18, 17, 15), 17)),
    "reused_if_any_tap": (("lattice", 32, 16, "one_y", rc.GUI, 2), ((246, 246, 246), 246)),
    "daz": (("lattice", 32, 16, "half_xy", rc.GRID, 16), ((0, 0, 38), 0)),
}
# the same counts on the earlier suites' cases: the box "shift" case at
# 37 x 23 and the clean crease and step cases at 67 x 35 with the default
# parameters, then test_cap_and_normal_bound's poisoned crease planes at
# max_count 2, 16 and 1 << 24
WRONG_EDGES_EARLIER = {
    # fx in (-1, 0) occurs on them: caught already
    "trunc_floor": ((16, 0, 16), (35, 20, 35), (35, 20, 35), (35, 0, 35), (35, 20, 35), (35, 20, 35)),
    # so is a fused fx
    "contracted": ((26, 0, 30), (196, 0, 216), (143, 0, 158), (188, 0, 209), (188, 1, 199), (188, 6, 200)),
    "strict_sigma": ((0, 0, 0),) * 6,
    "strict_normal": ((0, 0, 0),) * 6,
    # the poisoned crease planes meet the cap at every max_count: caught already
    "cap_strict": ((0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 2245), (0, 10, 11), (0, 20, 20)),
    "round_counter": ((0, 17, 16), (0, 1127, 1127), (0, 1123, 1123), (0, 0, 0), (0, 1086, 1086), (0, 1074, 1074)),
    "grid_last_row": ((1, 0, 3),) + ((0, 0, 0),) * 5,
    "reused_if_any_tap": ((0, 0, 0),) * 6,
    "daz": ((0, 0, 0),) * 6,
}


def _built(builder, W, H, shift, plane, mc):
    if builder == "lattice":
        return rc.lattice_case(W, H, shift, plane, max_count=mc)
    return rc.near_lattice_case(W, H, shift, plane, max_count=mc)


def _shows(ref, out):
    return rc.differ(ref, out), int((ref[4] != out[4]).sum())


@pytest.mark.parametrize("wrong", rc.WRONG_EDGES)
def test_each_slip_shows_on_a_lattice_case(wrong):
    (builder, W, H, shift, plane, mc), pinned = WRONG_EDGES_SHOW[wrong]
    case = _built(builder, W, H, shift, plane, mc)
    got = _shows(_run(case, W, H, plane, **_params(mc)), _run(case, W, H, plane, wrong=wrong, **_params(mc)))
    print(wrong, got)
    assert got == pinned and got != ((0, 0, 0), 0)


@pytest.mark.parametrize("wrong", rc.WRONG_EDGES)
def test_where_the_earlier_cases_miss_each_slip(oracle, wrong):
    """The gap: most slips change no pixel of the cases the kernel was tested
    on; those that do were caught there already."""
    got = []
    poisoned = rc.poisoned(rc.synthetic_case("crease", 67, 35), 67, 35)
    for case, W, H, par in ((rc.rendered_case("box", "shift", 37, 23), 37, 23, {}),
                            (rc.synthetic_case("crease", 67, 35), 67, 35, {}),
                            (rc.synthetic_case("step", 67, 35), 67, 35, {}),
                            (poisoned, 67, 35, dict(max_count=2)), (poisoned, 67, 35, dict(max_count=16)),
                            (poisoned, 67, 35, dict(max_count=1 << 24))):
        got.append(rc.differ(_run(case, W, H, rc.GRID, **par), _run(case, W, H, rc.GRID, wrong=wrong, **par)))
    print(wrong, got)
    assert tuple(got) == WRONG_EDGES_EARLIER[wrong]


@pytest.mark.parametrize("plane", ac.PLANES)
def test_slips_that_no_input_shows(plane):
    """open_left, closed_right, t_nonneg and no_floor_two (rc.SAME_RESULT) give
    the restatement's bits and classes on every edge case, though fx == -1,
    fx == W, t == 0 and c' == 2 all occur there: these are not in WRONG_EDGES
    because no case can ask for them."""
    for name, case, W, H, par in edge_cases(plane):
        ref = _run(case, W, H, plane, **par)
        for wrong in rc.SAME_RESULT:
            assert _shows(ref, _run(case, W, H, plane, wrong=wrong, **par)) == ((0, 0, 0), 0), (name, wrong)


# ---- invariants ------------------------------------------------------------------------------
OVERFLOWS = {rc.GRID: 2476, rc.GUI: 2093}  # reused pixels with out_m2 = +inf, over edge_cases


@pytest.mark.parametrize("plane", ac.PLANES)
def test_invariants_on_every_edge_case(plane):
    """The classes sum to W H, empty pixels are exact zeros, c' lies within
    [2, max_count] and out_pixels is finite on reused pixels; out_m2 is finite
    too, or +inf on the pixels the census counts: finite inputs with m2 = 3e38
    whose var (nf' (nf' - 1)) overflows (include/ipt_capi.h, step 4)."""
    overflows = 0
    for name, case, W, H, par in edge_cases(plane):
        px, cn, m2, stats, cls = _run(case, W, H, plane, **par)
        assert int(stats.sum()) == W * H and stats[3] == 0, name
        assert [int((cls == k).sum()) for k in range(3)] == stats[:3].tolist(), name
        empty = cls != rc.REUSED
        assert not dc.bits(px)[empty].any() and not cn[empty].any() and not dc.bits(m2)[empty].any(), name
        if plane == rc.GRID and H > 1:
            assert (cls.reshape(H, W)[H - 1] == rc.NOT_SURFACE).all(), name
        if (~empty).any():
            assert cn[~empty].min() >= 2 and cn[~empty].max() <= par["max_count"], name
            assert np.isfinite(px[~empty]).all(), name
        bad = ~np.isfinite(m2)
        assert (m2[bad] == np.inf).all(), name
        assert int(bad.sum()) == rc.census(case, W, H, plane, **par)["out_m2 not finite"], name
        if bad.any():  # only from the largest m2 of the set
            assert (np.asarray(case[2]) == F(3e38)).any(), name
        overflows += int(bad.sum())
    print(plane, "overflows", overflows)
    assert overflows == OVERFLOWS[plane] and overflows > 0


# ---- identity --------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", rc.LATTICE_FRAMES + ((2, 2), (1, 1)), ids=lambda f: "%dx%d" % f)
def test_identity_returns_the_previous_pixels_and_counters(frame, plane):
    """No move, counters in 2..max_count, finite m2, heights within sigma_z and
    normals at or above normal_min: tx == ty == 0 on every pixel, the own pixel
    is the one tap with a weight, and mean and counter come back bit for bit.
    (m2 is not claimed: m2 / k * k need not round back.)"""
    W, H = frame
    case = rc.lattice_case(W, H, "none", plane, benign=True)
    c = rc.census(case, W, H, plane, **_params())
    px, cn, m2, stats, cls = _run(case, W, H, plane, **_params())
    surface = (case[4]["kind"].reshape(-1) & 3) == 1
    assert surface.sum() == (W * (H - 1) if plane == rc.GRID and H > 1 else W * H)
    assert c["tx == 0"] == c["ty == 0"] == int(surface.sum()) == int(stats[0]) and stats[1] == 0
    assert np.array_equal(dc.bits(px)[surface], dc.bits(np.asarray(case[0]))[surface])
    assert np.array_equal(cn[surface], np.asarray(case[1])[surface])
    assert np.isfinite(m2).all()


# ---- tiny frames -----------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", rc.TINY_LATTICE_FRAMES, ids=lambda f: "%dx%d" % f)
def test_tiny_frames(frame, plane):
    """Constant planes (rc.constant_lattice_case: every tap inside the frame
    that the row map gives a pixel is used), so that the row map and the
    frame's border alone decide. No move: every surface pixel is reused and
    gets its own mean back. Half a pixel either way: every surface pixel's own
    source pixel is among its taps with weight 1/4, so all are reused. One row
    up (fy = ys + 1, ty = 0): the one tap with a weight is source row ys + 1,
    which under the Gui map is destination row H-2-ys and under the Grid map
    has a destination only up to row H-2; the pixels of the last source row
    find row H-1 under the Grid map, which is no pixel's nominal source, or
    leave the frame, and are "disoccluded". Every reused counter is 4."""
    W, H = frame
    rows = H - 1 if plane == rc.GRID and H > 1 else H  # rows with a nominal source
    for shift in TINY_SHIFTS:
        case = rc.constant_lattice_case(W, H, shift, plane)
        px, cn, m2, stats, cls = _run(case, W, H, plane, **_params())
        assert stats[2] == W * (H - rows) and int(stats.sum()) == W * H
        assert (cn[cls == rc.REUSED] == 4).all()
        if shift[1] != -1.0:
            assert stats[0] == W * rows and stats[1] == 0, (shift, stats)
            if shift == (0.0, 0.0):
                assert np.array_equal(dc.bits(px)[cls == rc.REUSED], dc.bits(case[0])[cls == rc.REUSED])
        else:
            assert stats[0] == W * (rows - 1) and stats[1] == W, (shift, stats)
