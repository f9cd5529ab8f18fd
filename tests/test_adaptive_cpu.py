"""The conditions that make tests/test_gpu_adaptive.py discriminating, checked
on the CPU oracle alone (no GPU): the seeded half mask really separates the
nominal-destination indexing from the wrong ones on the drift frames, the loop
case really switches most pixels off and keeps some on, and the bindings of
the adaptive entry points exist."""
import ctypes as C

import numpy as np
import pytest

import adaptive_cases as ac
import drift_cases as dc
from ipt_amd import capi

bits = dc.bits


@pytest.mark.parametrize("frame", ac.HALF_FRAMES, ids=lambda f: "%dx%dx%d" % f)
def test_half_mask_counts(oracle, frame):
    """Pinned: how many samples the half mask drops with radiance, and how
    many drifted samples cross between active and masked pixels each way. A
    change of seed, jitter or mask that emptied a class fails here."""
    W, H, spp = frame
    v, c, _ = dc.oracle_samples(W, H, spp)
    m = ac.half_mask(W, H)
    act = ac.active_samples(c, m, ac.GRID)
    _, yi, xi = ac.destinations(c, ac.GRID)
    land = m[yi, xi] != 0
    drift, nz = c != 0x05, v != 0
    got = (int((~act & nz).sum()),
           (int((act & drift & ~land).sum()), int((act & drift & ~land & nz).sum())),
           (int((~act & drift & land).sum()), int((~act & drift & land & nz).sum())),
           int((act & drift & land).sum()))
    assert got == ac.HALF_COUNTS[frame]
    paths, drifted = ac.counts(c, m, ac.GRID)
    assert paths == int(act.sum()) and 0 < drifted == got[1][0] + got[3] < int(drift.sum())


def test_wrong_variants_differ(oracle):
    """Each wrong replay differs from the right one on (60000, 3, 9): the mask
    by source pixel, the mask at the landing pixel, masked samples as zeros
    (pixels and counters), m2 as a sum of squares (m2 alone)."""
    W, H, spp = ac.HALF_FRAMES[0]
    v, c, _ = dc.oracle_samples(W, H, spp)
    m = ac.half_mask(W, H)
    ref, m2 = ac.replay(v, c, m, ac.GRID)
    assert (m2 >= 0).all() and (m2 > 0).any()
    for how in ("source", "landing", "zeros"):
        w, wm2 = ac.replay(v, c, m, ac.GRID, how=how)
        assert (bits(w["pixels"]) != bits(ref["pixels"])).any(), how
        assert (w["counters"] != ref["counters"]).any(), how
        assert (bits(wm2) != bits(m2)).any(), how
    w, wm2 = ac.replay(v, c, m, ac.GRID, how="sumsq")
    assert all((bits(w[k]) == bits(ref[k])).all() for k in w)
    assert (bits(wm2) != bits(m2)).any()


def test_all_ones_mask_is_the_unmasked_plane(oracle):
    """An all-ones mask and no mask replay to ob.accumulate's plane, on both
    row maps' code sets (the Gui's against gui_cases' restatement)."""
    import gui_cases as gc
    W, H, spp = 4099, 61, 2
    v, c, _ = dc.oracle_samples(W, H, spp)
    for mask in (None, np.ones((H, W), np.uint8)):
        img, _ = ac.replay(v, c, mask, ac.GRID)
        ref = dc.oracle_plane(W, H, spp)
        assert all((bits(img[k]) == bits(ref[k])).all() for k in img)
        img, _ = ac.replay(v, ac.codes_of(W, H, spp, ac.GUI), mask, ac.GUI)
        ref = gc.gui_plane(W, H, spp)
        assert all((bits(img[k]) == bits(ref[k])).all() for k in img)


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", ac.LOOP_FRAMES, ids=lambda f: "%dx%d" % f)
def test_loop_case_condition(oracle, frame, plane):
    """The loop case: nearly everything is active after round 1 (row H-1 of the
    Grid plane, which has no nominal source, is excluded: 1/H less than
    counting it), between a tenth and a half after each later round, so masks
    change from round to round and the counters end up different."""
    W, H = frame
    v, _, _ = dc.oracle_samples(W, H, ac.LOOP_SPP)
    c = ac.codes_of(W, H, ac.LOOP_SPP, plane)
    rounds, used = ac.loop(v, c, plane, ac.LOOP_ROUND, **ac.LOOP_ADAPT)
    assert used == ac.LOOP_SPP and len(rounds) == ac.LOOP_SPP // ac.LOOP_ROUND
    share = [float(r[3][0]) / (W * H) for r in rounds]
    assert share[0] >= 0.85, share
    assert all(0.10 <= s <= 0.50 for s in share[1:]), share
    for img, m2, mask, stats in rounds:
        assert not (m2 < 0).any()
        assert int(mask.sum()) == int(stats[0])
        if plane == ac.GRID:
            assert not mask.reshape(H, W)[H - 1].any()
    final = rounds[-1][0]["counters"]
    live = final.reshape(H, W)[:H - 1] if plane == ac.GRID else final
    assert np.unique(live).size > 2
    assert any((a[2] != b[2]).any() for a, b in zip(rounds, rounds[1:]))


def test_adapt_restatement_classes():
    """starved pixels are active whatever their m2; a NaN on either side is
    inactive and counted; the Grid map's last row is nobody's."""
    W, H = 4, 2
    px = np.array([1, 1, np.nan, 1, 1, 1, 1, 1], np.float32)
    cn = np.array([0, 7, 8, 8, 0, 0, 0, 0], np.uint32)
    m2 = np.array([0, np.nan, 1, np.nan, 0, 0, 0, 0], np.float32)
    mask, stats = ac.adapt(px, cn, m2, W, H, 8, 0.1, 0.0)
    assert mask.tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and stats.tolist() == [2, 2, 2, 0]
    mask, stats = ac.adapt(px, cn, m2, W, H, 8, 0.1, 0.0, gui=True)
    assert mask.tolist() == [1, 1, 0, 0, 1, 1, 1, 1] and stats.tolist() == [6, 6, 2, 0]


def test_adaptive_bindings_exist():
    """The library exports the adaptive entry points, the binding declares them
    and ipt_adapt_params has the header's layout. Fails without the feature."""
    lib = capi.load()
    for name in ("ipt_render_masked_device_async", "ipt_render_masked_device", "ipt_adapt_device",
                 "ipt_render_adaptive"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert capi.ABI_VERSION == 7 and lib.ipt_abi_version() == 7
    assert C.sizeof(capi.AdaptParams) == 24
    assert [(n, getattr(capi.AdaptParams, n).offset) for n, _ in capi.AdaptParams._fields_] == [
        ("width", 0), ("height", 4), ("min_count", 8), ("rel_tol", 12), ("abs_tol", 16), ("flags", 20)]
    ap = capi.make_adapt_params(13, 11, min_count=8, rel_tol=0.25, abs_tol=1e-3, flags=capi.IPT_FLAG_GUI_PLANE)
    assert (ap.width, ap.height, ap.min_count, ap.flags) == (13, 11, 8, 2)
    assert np.float32(ap.rel_tol) == np.float32(0.25) and np.float32(ap.abs_tol) == np.float32(1e-3)
    for m in ("render_masked_device", "render_masked_device_async", "adapt_device", "render_adaptive"):
        assert callable(getattr(capi.Context, m))
    # refused without a context, before anything else is looked at
    assert lib.ipt_adapt_device(None, C.byref(ap), None, None, None, None, None, None) == capi.IPT_E_INVALID
