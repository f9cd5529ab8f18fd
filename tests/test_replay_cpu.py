"""The cases of tests/replay_cases.py bite: conditions checked on the CPU alone.

tests/test_gpu_replay.py hands these samples to accumulate_kernel through
ipt_replay_samples and compares the plane with ob.accumulate (Grid) or
gui_cases.replay (Gui). That is worth something while the references agree
with each other on these very cases, while the cases hold what they are meant
to hold (every code, 9- and 12-fold convergence, drift across shard
boundaries), and while a replay that scans in another order gives another
plane. Each of those is asserted here."""
import numpy as np
import pytest

import drift_cases as dc
import gui_cases as gc
import oracle_binding as ob
import replay_cases as rc

bits = dc.bits
KEYS = tuple(k for k, _ in dc.PLANE_KEYS)


def _equal(a, b, rows=None, W=None):
    for k in KEYS:
        x, y = bits(a[k]), bits(b[k])
        if rows is not None:
            x, y = x.reshape(-1, W)[rows], y.reshape(-1, W)[rows]
        if not np.array_equal(x, y):
            return False
    return True


def _pixels_differ(a, b):
    return bool((bits(a["pixels"]) != bits(b["pixels"])).any())


def _reference(values, codes, plane, img=None):
    """The reference the GPU tests use."""
    if plane == rc.GUI:
        return gc.replay(values, codes, img=img)
    return ob.accumulate(values, codes, img=img)


DENSE = [(W, H, spp, plane) for plane in rc.PLANES for W, H in rc.DENSE_FRAMES for spp in rc.DENSE_SPPS]
SINGLE = [(code, plane) for plane in rc.PLANES for code in rc.DRIFT_CODES]
CONVERGE = [(W, H, plane) for plane in rc.PLANES for W, H in rc.CONVERGE_FRAMES]


def _all_cases():
    for W, H, spp, plane in DENSE:
        yield "dense-%dx%dx%d-%s" % (W, H, spp, plane), plane, lambda a=(W, H, spp, plane): rc.dense_case(*a)
    for code, plane in SINGLE:
        yield "single-%#x-%s" % (code, plane), plane, lambda a=(code, plane): rc.single_code(
            a[0], *rc.SINGLE_FRAME, rc.SINGLE_SPP, a[1])
    for W, H, plane in CONVERGE:
        yield "converge-%dx%d-%s" % (W, H, plane), plane, lambda a=(W, H, plane): rc.converge(
            a[0], a[1], rc.CONVERGE_SPP, a[2])
    yield "shard-grid", rc.GRID, lambda: rc.dense_case(*rc.SHARD_FRAME, rc.SHARD_SPP, rc.GRID)
    yield "shard-gui", rc.GUI, lambda: rc.dense_case(*rc.SHARD_FRAME, rc.SHARD_SPP, rc.GUI)


ALL = list(_all_cases())


@pytest.mark.parametrize("plane,make", [c[1:] for c in ALL], ids=[c[0] for c in ALL])
def test_references_agree(oracle, plane, make):
    """Grid: ob.accumulate (pinned to the compiled reference) equals the numpy
    replay in raster order, bit for bit. Gui: gui_cases.replay equals the same
    numpy replay under the Gui map, and -- through the row identity
    (replay_cases.gui_as_grid) -- rows 1..H-1 equal ob.accumulate's of the
    same samples on a Grid frame one row taller, whose row H stays empty."""
    v, c = make()
    _, H, W = v.shape
    numpy_ref = rc.replay(v, c, plane)
    assert _equal(_reference(v, c, plane), numpy_ref)
    if plane == rc.GRID:
        assert _equal(dc.replay(v, c), numpy_ref)
    elif H >= 3:
        grid = ob.accumulate(*rc.gui_as_grid(v, c))
        for k in KEYS:
            g = bits(grid[k]).reshape(H + 1, W)
            assert np.array_equal(g[1:H], bits(numpy_ref[k]).reshape(H, W)[1:]), k
            assert not g[H].any()
        assert (grid["counters"].reshape(H + 1, W)[0] > numpy_ref["counters"].reshape(H, W)[0]).all()


# Frames below 5x4: the replays of rc.WRONG that give another plane than the
# right order, by (plane, W, H, spp); the others coincide with it there, which
# the test asserts. Where only "nominal_only" is listed (or nothing: 1x1 holds
# no drift) the case tests parity with the reference and no ordering.
SMALL_DIFFERS = {
    ('grid', 1, 1, 1): (),
    ('grid', 1, 1, 8): (),
    ('grid', 1, 1, 9): (),
    ('grid', 1, 1, 17): (),
    ('grid', 1, 7, 1): ('nominal_only',),
    ('grid', 1, 7, 8): ('rows_descending', 'nominal_only'),
    ('grid', 1, 7, 9): ('rows_descending', 'drift_last', 'nominal_only'),
    ('grid', 1, 7, 17): ('rows_descending', 'drift_last', 'nominal_only'),
    ('grid', 7, 1, 1): ('nominal_only',),
    ('grid', 7, 1, 8): ('nominal_only',),
    ('grid', 7, 1, 9): ('drift_last', 'nominal_only'),
    ('grid', 7, 1, 17): ('drift_last', 'nominal_only'),
    ('grid', 2, 2, 1): ('nominal_only',),
    ('grid', 2, 2, 8): ('cols_first', 'rows_descending', 'nominal_only'),
    ('grid', 2, 2, 9): ('rows_descending', 'drift_last', 'nominal_only'),
    ('grid', 2, 2, 17): ('rows_descending', 'nominal_only'),
    ('grid', 3, 3, 1): ('nominal_only',),
    ('grid', 3, 3, 8): ('drift_last', 'nominal_only'),
    ('grid', 3, 3, 9): ('cols_first', 'rows_descending', 'diag_late', 'drift_last', 'nominal_only'),
    ('grid', 3, 3, 17): ('cols_first', 'rows_descending', 'drift_last', 'nominal_only'),
    ('gui', 1, 1, 1): (),
    ('gui', 1, 1, 8): (),
    ('gui', 1, 1, 9): (),
    ('gui', 1, 1, 17): (),
    ('gui', 1, 7, 1): ('nominal_only',),
    ('gui', 1, 7, 8): ('rows_descending', 'drift_last', 'nominal_only'),
    ('gui', 1, 7, 9): ('rows_descending', 'drift_last', 'nominal_only'),
    ('gui', 1, 7, 17): ('rows_descending', 'nominal_only'),
    ('gui', 7, 1, 1): ('nominal_only',),
    ('gui', 7, 1, 8): ('drift_last', 'nominal_only'),
    ('gui', 7, 1, 9): ('drift_last', 'nominal_only'),
    ('gui', 7, 1, 17): ('drift_last', 'nominal_only'),
    ('gui', 2, 2, 1): ('nominal_only',),
    ('gui', 2, 2, 8): ('rows_descending', 'drift_last', 'nominal_only'),
    ('gui', 2, 2, 9): ('nominal_only',),
    ('gui', 2, 2, 17): ('cols_first', 'rows_descending', 'drift_last', 'nominal_only'),
    ('gui', 3, 3, 1): ('nominal_only',),
    ('gui', 3, 3, 8): ('drift_last', 'nominal_only'),
    ('gui', 3, 3, 9): ('nominal_only',),
    ('gui', 3, 3, 17): ('cols_first', 'rows_descending', 'diag_late', 'drift_last', 'nominal_only'),
}


@pytest.mark.parametrize("W,H,spp,plane", DENSE, ids=lambda v: str(v))
def test_dense_cases_discriminate(W, H, spp, plane):
    """From 5x4 upward every dense case holds all eight drift codes and a
    replay by columns first, by descending rows, with the 0x0 / 0x2 samples
    deferred, or without the drifted samples gives other pixels; so does one
    with all drifted samples deferred once there are eight passes (in a single
    pass from zeros its reordering mostly swaps a pixel's first two samples,
    which commute). Below 5x4: exactly the replays of SMALL_DIFFERS differ."""
    v, c = rc.dense_case(W, H, spp, plane)
    ref = rc.replay(v, c, plane)
    differs = tuple(h for h in rc.WRONG if _pixels_differ(rc.replay(v, c, plane, h), ref))
    if W * H < 20:
        assert differs == SMALL_DIFFERS[plane, W, H, spp]  # (the others: equal pixels, bit for bit)
        return
    assert set(dc.histogram(c)) == set(rc.DRIFT_CODES)
    assert {"cols_first", "rows_descending", "diag_late", "nominal_only"} <= set(differs)
    if spp >= 8:
        assert "drift_last" in differs
    share = float((c != 0x05).mean())
    assert 0.5 <= share <= 0.75  # p_drift = 0.7 less what the edges take back
    # the pixels a launch flags (nominal pixel and destination of every drifted
    # sample of all its passes): in a one-pass launch flagged and unflagged
    # pixels sit side by side in a row; from eight passes on nine pixels in ten
    # of a dense case are flagged, and the one-pass launches of the chunked GPU test
    # are what mixes the two branches within a wave at more passes
    yn, yi, xi = rc.destinations(c, plane)
    ix = np.broadcast_to(np.arange(W)[None, None, :], c.shape)
    d = c != 0x05
    flags = np.zeros((H, W), bool)
    flags[yn[d], ix[d]] = True
    flags[yi[d], xi[d]] = True
    if spp == 1:
        assert (flags[:, 1:] != flags[:, :-1]).any()
        if W >= 37:
            assert min(int((flags[:, 1:] & ~flags[:, :-1]).sum()), int((~flags[:, 1:] & flags[:, :-1]).sum())) >= 10
    else:
        assert flags.mean() >= 0.9
        one = np.zeros((H, W), bool)
        one[yn[0][d[0]], ix[0][d[0]]] = True
        one[yi[0][d[0]], xi[0][d[0]]] = True
        assert W * H <= 20 or (one[:, 1:] != one[:, :-1]).any()
    if spp == max(rc.DENSE_SPPS):
        # drift arrives in every corner, and at every edge from inside and along it
        for y in (0, H - 1):
            for x in (0, W - 1):
                assert (d & (yi == y) & (xi == x)).any(), (x, y)
        assert (d & (xi == 0) & (xi - ix == -1)).any() and (d & (xi == W - 1) & (xi - ix == 1)).any()
        assert (d & (yi == 0) & (yi - yn == -1)).any() and (d & (yi == H - 1) & (yi - yn == 1)).any()
        for edge in (yi == 0, yi == H - 1):
            assert {-1, 1} <= set((xi - ix)[d & edge].tolist())
        for edge in (xi == 0, xi == W - 1):
            assert {-1, 1} <= set((yi - yn)[d & edge].tolist())


def test_structural_coincidences():
    """Why the smallest frames cannot tell: one column has no second source
    column and no dx, one row no second source row and no dy, one pixel no
    drift at all."""
    for key, differs in SMALL_DIFFERS.items():
        _, W, H, _ = key
        if W == 1:
            assert not {"cols_first", "diag_late"} & set(differs)
        if H == 1:
            assert not {"cols_first", "rows_descending", "diag_late"} & set(differs)
        if W == H == 1:
            assert differs == ()


@pytest.mark.parametrize("code,plane", SINGLE, ids=lambda v: hex(v) if isinstance(v, int) else v)
def test_single_code_cases(code, plane):
    """The code sits on at least a third of the samples and no other drift
    code appears; the frames of 0x0 and 0x2 tell the deferred-diagonal replay
    from the right one, every frame tells the replay that drops the drift."""
    v, c = rc.single_code(code, *rc.SINGLE_FRAME, rc.SINGLE_SPP, plane)
    assert {code} <= set(np.unique(c).tolist()) <= {code, 0x05}  # (Grid 0x9: every destination is in the frame)
    assert float((c == code).mean()) >= 1.0 / 3.0
    ref = rc.replay(v, c, plane)
    assert _pixels_differ(rc.replay(v, c, plane, "nominal_only"), ref)
    assert _pixels_differ(rc.replay(v, c, plane, "diag_late"), ref) == (code in rc.DIAG_DOWN)
    if code in dc.ORDER_SENSITIVE:
        assert _pixels_differ(rc.replay(v, c, plane, "drift_last"), ref)


@pytest.mark.parametrize("W,H,plane", CONVERGE, ids=lambda v: str(v))
def test_converge_cases(W, H, plane):
    """(The 9- and 12-sample counts and their source rows are asserted by the
    generator.) Every wrong replay gives other pixels, and a centre's counter
    after the passes is 9 or 12 a pass."""
    v, c = rc.converge(W, H, rc.CONVERGE_SPP, plane)
    ref = rc.replay(v, c, plane)
    for h in rc.WRONG:
        assert _pixels_differ(rc.replay(v, c, plane, h), ref), h
    want = {9 * rc.CONVERGE_SPP} if plane == rc.GUI else {9 * rc.CONVERGE_SPP, 12 * rc.CONVERGE_SPP}
    assert want <= set(ref["counters"].tolist())
    assert int(ref["counters"].max()) == (rc.MAX_PER_PASS if plane == rc.GRID else 9) * rc.CONVERGE_SPP


@pytest.mark.parametrize("plane", rc.PLANES)
def test_sharded_case_cuts_through_drift(plane):
    """Drifted samples whose nominal and destination rows have different
    owners (0xfe halo samples for the one, candidate-row samples for the
    other): at least 100 under the one-row plans, from above, below and
    diagonally; the Grid count is drift_cases.cross_shard's."""
    W, H = rc.SHARD_FRAME
    _, c = rc.dense_case(W, H, rc.SHARD_SPP, plane)
    for tile, n in rc.SHARD_PLANS:
        x = rc.cross_shard(c, plane, tile, n)
        if plane == rc.GRID:
            assert x == dc.cross_shard(c, tile, n)
        assert x >= (100 if tile == 1 else 1), (tile, n, x)
    yn, yi, xi = rc.destinations(c, plane)
    ix = np.arange(W)[None, None, :]
    cross = dc.shard_of(yn, 1, 3) != dc.shard_of(yi, 1, 3)
    for dy in (-1, 1):
        for dx in (-1, 0, 1):
            assert int((cross & (yi - yn == dy) & (xi - ix == dx)).sum()) >= 10, (dy, dx)


@pytest.mark.parametrize("plane", rc.PLANES)
@pytest.mark.parametrize("spp", rc.PRELOAD_SPPS)
def test_preloaded_case(oracle, spp, plane):
    """Every preloaded kind of every array sits on a destination of drifted
    samples, no counter can wrap (twelve samples a pass allowed for), no
    pairing generates a NaN, and the plane changes."""
    W, H = rc.PRELOAD_FRAME
    v, c = rc.dense_case(W, H, spp, plane)
    hot = np.unique(rc.hot_pixels(c, plane))
    pre, pick = rc.preloaded(W, H, spp)
    for k, names in dc.preload_kinds(spp, rc.MAX_PER_PASS).items():
        assert np.bincount(pick[k][hot], minlength=len(names)).min() >= 3, k
    added = rc.replay(v, c, plane)["counters"]
    assert int(added.max()) <= rc.MAX_PER_PASS * spp
    assert int((pre["counters"].astype(np.uint64) + added).max()) < 0xffffffff
    assert not (np.isinf(pre["pixels"]) & (pre["counters"] == 0)).any()
    ref = _reference(v, c, plane, img=dc.copy_plane(pre))
    assert _equal(ref, rc.replay(v, c, plane, img=dc.copy_plane(pre)))
    assert _pixels_differ(ref, pre)


def test_generators_refuse_out_of_frame_codes():
    """The generators' own guard: what ipt_replay_samples refuses."""
    for plane in rc.PLANES:
        for bad in (0x10, 0xfe, 0xff, 0x03, 0x0c):
            with pytest.raises(AssertionError):
                rc.assert_in_frame(np.full((1, 4, 5), bad, np.uint8), plane)
        c = np.full((1, 4, 5), 0x05, np.uint8)
        rc.assert_in_frame(c, plane)
        for (iy, ix, code) in ((1, 0, 0x4), (1, 4, 0x6)):  # dx = -1 at column 0, +1 at column W-1
            c2 = c.copy()
            c2[0, iy, ix] = code
            with pytest.raises(AssertionError):
                rc.assert_in_frame(c2, plane)
        c2 = c.copy()
        c2[0, 3, 2] = 0x1  # source row H-1: nominal row 0 under both maps; dy = -1
        with pytest.raises(AssertionError):
            rc.assert_in_frame(c2, plane)
    c2 = np.full((1, 4, 5), 0x05, np.uint8)
    c2[0, 0, 2] = 0x9  # source row 0, dy = +1: the Gui's top row H-1 is its nominal row, Grid row H-2 is
    rc.assert_in_frame(c2, rc.GRID)
    with pytest.raises(AssertionError):
        rc.assert_in_frame(c2, rc.GUI)
