"""accumulate_kernel on chosen samples, through the replay probe
(ipt_replay_samples): every drift code, densely.

A render drifts 5.6e-5 of its samples, never produces the codes 0x0 and 0x2
and essentially never lands two drifted samples in one pixel in one pass, so
the frames of test_gpu_drift.py and test_gpu_gui_plane.py show the replay's
flagged-pixel branch one drifted sample at a time. The probe runs what a
render runs behind its path kernel (shard plan, candidate-row layout, drift
flags, chunking, the accumulate_kernel launch) on the samples of
tests/replay_cases.py: most samples drifted, nine and twelve sources into one
pixel, drift from every side at every edge and corner, flagged and unflagged
pixels side by side, 0xfe halos from above, below and diagonally in one tile.
tests/test_replay_cpu.py shows without a GPU that the references agree on
these cases and that a replay scanning in another order fails them.

Every comparison is on the bit patterns of all four arrays, against
ob.accumulate (Grid) or gui_cases.replay (Gui)."""
import numpy as np
import pytest
import torch

import drift_cases as dc
import gui_cases as gc
import oracle_binding as ob
import replay_cases as rc
from ipt_amd import capi, scenes

pytestmark = pytest.mark.gpu

bits = dc.bits
KEYS = tuple(k for k, _ in dc.PLANE_KEYS)
SUBSETS = (KEYS, ("pixels", "counters", "pixel_max"), ("pixels", "counters", "sums"), ("pixels", "counters"))


def _assert_plane_equal(img, ref, keys=KEYS, what="", rows=None, W=None):
    for k in keys:
        a, b = bits(img[k]), bits(ref[k])
        if rows is not None:
            a, b = a.reshape(-1, W)[rows], b.reshape(-1, W)[rows]
        bad = (a != b).reshape(-1)
        assert not bad.any(), (what, k, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())


def _to_device(img, keys=KEYS):
    dev = torch.device("cuda", 0)
    return {k: torch.from_numpy(img[k].view(np.int32) if k == "counters" else img[k]).to(dev) for k in keys}


def _ptrs(t):
    return (t["pixels"].data_ptr(), t["counters"].data_ptr(), t["sums"].data_ptr() if "sums" in t else None,
            t["pixel_max"].data_ptr() if "pixel_max" in t else None)


def _to_host(t):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if k == "counters" else v.cpu().numpy()) for k, v in t.items()}


def _params(W, H, spp, plane, **kw):
    return capi.make_params(W, H, spp, flags=rc.flag(plane), **kw)


def _reference(v, c, plane, img=None):
    return gc.replay(v, c, img=img) if plane == rc.GUI else ob.accumulate(v, c, img=img)


def _replay(ctx, v, c, plane, start=None, keys=KEYS, **kw):
    """The probe's plane of samples (v, c) into a copy of `start` (zeros)."""
    spp, H, W = v.shape
    t = _to_device(dc.plane(W, H) if start is None else start, keys)
    ctx.replay_samples(_params(W, H, spp, plane, **kw), v, c, *_ptrs(t))
    return _to_host(t)


# ---- A: the probe against the product ------------------------------------------
@pytest.mark.parametrize("plane", rc.PLANES)
@pytest.mark.parametrize("frame,spp", [(dc.WIDE, 9), (dc.TALL, 2)], ids=["60000x3x9", "3x60000x2"])
def test_probe_equals_render_on_rendered_samples(gpu_ctx, frame, spp, plane):
    """ipt_render_values' samples through the probe give ipt_render_device's
    plane, whole and with the (1, 3) shard plan one shard at a time into one
    image: the marking kernel's flag rule and its 0xfe rule are raygen's, on
    real drift and real halos."""
    W, H = frame
    gpu_ctx.upload_scene(scenes.make_scene_box())
    p = dc.params(W, H, spp, flags=rc.flag(plane))
    v, c = gpu_ctx.render_values(p)
    assert int((c != 0x05).sum()) >= 100 and not (c >= 0x10).any()
    t = _to_device(dc.plane(W, H))
    gpu_ctx.render_device(p, *_ptrs(t))
    product = _to_host(t)
    assert product["counters"].any()
    _assert_plane_equal(_replay(gpu_ctx, v, c, plane), product, what="whole frame")
    t = _to_device(dc.plane(W, H))
    for s in range(3):
        gpu_ctx.replay_samples(_params(W, H, spp, plane, tile_rows=1, n_shards=3, shard_id=s), v, c, *_ptrs(t))
    _assert_plane_equal(_to_host(t), product, what="three shards into one image")


# ---- B: dense codes from zeros ---------------------------------------------------
@pytest.mark.parametrize("plane", rc.PLANES)
@pytest.mark.parametrize("spp", rc.DENSE_SPPS)
@pytest.mark.parametrize("frame", rc.DENSE_FRAMES, ids=lambda f: "%dx%d" % f)
def test_dense_bit_exact(gpu_ctx, oracle, frame, spp, plane):
    v, c = rc.dense_case(*frame, spp, plane)
    _assert_plane_equal(_replay(gpu_ctx, v, c, plane), _reference(v, c, plane))


# ---- C: one code at a time ---------------------------------------------------------
@pytest.mark.parametrize("plane", rc.PLANES)
@pytest.mark.parametrize("code", rc.DRIFT_CODES, ids=hex)
def test_single_code_bit_exact(gpu_ctx, oracle, code, plane):
    v, c = rc.single_code(code, *rc.SINGLE_FRAME, rc.SINGLE_SPP, plane)
    _assert_plane_equal(_replay(gpu_ctx, v, c, plane), _reference(v, c, plane))


# ---- D: nine and twelve sources into one pixel ---------------------------------------
@pytest.mark.parametrize("plane", rc.PLANES)
@pytest.mark.parametrize("frame", rc.CONVERGE_FRAMES, ids=lambda f: "%dx%d" % f)
def test_converge_bit_exact(gpu_ctx, oracle, frame, plane):
    v, c = rc.converge(*frame, rc.CONVERGE_SPP, plane)
    ref = _reference(v, c, plane)
    assert int(ref["counters"].max()) == (12 if plane == rc.GRID else 9) * rc.CONVERGE_SPP
    _assert_plane_equal(_replay(gpu_ctx, v, c, plane), ref)


# ---- E: preloaded planes -----------------------------------------------------------------
@pytest.mark.parametrize("plane", rc.PLANES)
@pytest.mark.parametrize("spp", rc.PRELOAD_SPPS)
def test_preloaded_bit_exact(gpu_ctx, oracle, spp, plane):
    """add_ray on existing state (counters around 2^24 and 2^31 and up to the
    last value that cannot wrap at twelve samples a pass, negative, -0.0,
    subnormal, infinite and NaN pixels, pixel_max below, above and NaN,
    infinite sums) under dense codes; with sums, without, without pixel_max,
    without both."""
    W, H = rc.PRELOAD_FRAME
    v, c = rc.dense_case(W, H, spp, plane)
    pre, _ = rc.preloaded(W, H, spp)
    ref = _reference(v, c, plane, img=dc.copy_plane(pre))
    assert (bits(ref["pixels"]) != bits(pre["pixels"])).any()
    for keys in SUBSETS:
        _assert_plane_equal(_replay(gpu_ctx, v, c, plane, pre, keys), ref, keys, what="+".join(keys))


# ---- F: shards ---------------------------------------------------------------------------
@pytest.mark.parametrize("plane", rc.PLANES)
@pytest.mark.parametrize("tile,n_shards", rc.SHARD_PLANS)
def test_sharded_bit_exact(gpu_ctx, oracle, tile, n_shards, plane):
    """Each shard replays into its own copy of a preloaded plane: the rows
    ipt_shard_plan calls owned equal the whole-frame reference, every other
    row is the preload's bit for bit, and the shards cover every row once."""
    W, H = rc.SHARD_FRAME
    v, c = rc.dense_case(W, H, rc.SHARD_SPP, plane)
    if tile == 1:
        assert rc.cross_shard(c, plane, tile, n_shards) >= 100
        if plane == rc.GRID:
            assert dc.cross_shard(c, tile, n_shards) >= 100
    pre, _ = rc.preloaded(W, H, rc.SHARD_SPP)
    ref = _reference(v, c, plane, img=dc.copy_plane(pre))
    covered = np.zeros(H, np.int32)
    for s in range(n_shards):
        kw = dict(tile_rows=tile, n_shards=n_shards, shard_id=s)
        owned, _ = capi.shard_plan(_params(W, H, rc.SHARD_SPP, plane, **kw))
        owned = owned.astype(bool)
        covered += owned
        got = _replay(gpu_ctx, v, c, plane, pre, **kw)
        _assert_plane_equal(got, ref, what=f"shard {s}: owned rows", rows=owned, W=W)
        _assert_plane_equal(got, pre, what=f"shard {s}: rows of other shards", rows=~owned, W=W)
    assert (covered == 1).all()


# ---- G: chunked launches -----------------------------------------------------------------
@pytest.mark.parametrize("plane", rc.PLANES)
def test_chunked_and_split_calls(gpu_ctx, oracle, monkeypatch, plane):
    """IPT_TEST_CHUNK_UNITS = 2600 splits the nine passes of 851 samples into
    three launches of three (render_chunks: ceil(7659 / 2600) = 3 chunks), each
    with its own flags; the plane is the single launch's and the reference's.
    Then two calls of four and five passes into one image."""
    W, H = rc.CHUNK_FRAME
    spp = rc.CHUNK_SPP
    v, c = rc.dense_case(W, H, spp, plane)
    ref = _reference(v, c, plane)
    single = _replay(gpu_ctx, v, c, plane)
    _assert_plane_equal(single, ref, what="one launch")
    units = 2600
    assert -(-spp * W * H // units) >= 3 and units >= W * H
    monkeypatch.setenv("IPT_TEST_CHUNK_UNITS", str(units))
    ctx = capi.Context(0)
    try:
        chunked = _replay(ctx, v, c, plane)
        _assert_plane_equal(chunked, single, what="three launches against one")
        _assert_plane_equal(chunked, ref, what="three launches")
        t = _to_device(dc.plane(W, H))
        ctx.replay_samples(_params(W, H, 4, plane), v[:4], c[:4], *_ptrs(t))
        ctx.replay_samples(_params(W, H, 5, plane), v[4:], c[4:], *_ptrs(t))
        _assert_plane_equal(_to_host(t), ref, what="two calls")
    finally:
        ctx.close()
    # one pass per launch: each launch's flags are its own pass's, so flagged
    # and unflagged pixels alternate within a wave (all nine passes together
    # flag nearly every pixel) and a pixel changes branch from launch to launch
    monkeypatch.setenv("IPT_TEST_CHUNK_UNITS", "1")
    ctx = capi.Context(0)
    try:
        _assert_plane_equal(_replay(ctx, v, c, plane), ref, what="nine launches")
    finally:
        ctx.close()


# ---- H: what the host refuses ------------------------------------------------------------
SENTINEL = {"pixels": np.float32(-123.25), "counters": np.uint32(0xabcd1234), "sums": np.float32(77.5),
            "pixel_max": np.float32(-3.0)}


def _refused(ctx, code, p, v, c, null_image=False):
    W, H = p.width, p.height
    start = {k: np.full(W * H, SENTINEL[k], dt) for k, dt in dc.PLANE_KEYS}
    t = _to_device(start)
    ptrs = (None,) + _ptrs(t)[1:] if null_image else _ptrs(t)
    with pytest.raises(capi.IptError) as e:
        ctx.replay_samples(p, v, c, *ptrs)
    assert e.value.code == code, (e.value.code, str(e.value))
    _assert_plane_equal(_to_host(t), start, what="image touched by a refused call")


@pytest.mark.parametrize("plane", rc.PLANES)
def test_invalid_input_is_refused_on_the_host(gpu_ctx, plane):
    """Every rule of ipt_replay_samples returns its code and leaves the image
    alone. No call here reaches a kernel: the kernels are never asked to
    consume a code the host would refuse."""
    W, H, spp = 5, 4, 2
    v = np.full((spp, H, W), 0.5, np.float32)
    ok = np.full((spp, H, W), 0x05, np.uint8)
    p = _params(W, H, spp, plane)

    def one(iy, ix, code, s=1):
        c = ok.copy()
        c[s, iy, ix] = code
        return c

    INV, UNS = capi.IPT_E_INVALID, capi.IPT_E_UNSUPPORTED
    for code in (0x03, 0x07, 0x0c, 0x0d, 0x0f, 0x10, 0x15, 0x85, 0xfe, 0xff):  # a field of 3; >= 0x10
        _refused(gpu_ctx, INV, p, v, one(2, 2, code))
    _refused(gpu_ctx, INV, p, v, one(2, 0, 0x4))          # dx = -1 at column 0
    _refused(gpu_ctx, INV, p, v, one(2, W - 1, 0x6))      # dx = +1 at column W-1
    _refused(gpu_ctx, INV, p, v, one(H - 1, 2, 0x1))      # dy = -1 from nominal row 0 (source row H-1)
    _refused(gpu_ctx, INV, p, v, one(H - 1, 0, 0x0, s=0))  # the corner, diagonally
    if plane == rc.GUI:
        _refused(gpu_ctx, INV, p, v, one(0, 2, 0x9))      # dy = +1 from the top row H-1 (source row 0)
        _refused(gpu_ctx, INV, p, v, one(0, W - 1, 0xa))  # and out of the top right corner
    else:
        # Grid: source row H-2 folds into row 0 as well; the top row H-1 is
        # nobody's nominal row above one row, so dy = +1 leaves a one-row frame
        _refused(gpu_ctx, INV, p, v, one(H - 2, 2, 0x1))
        p1 = _params(W, 1, spp, plane)
        c1 = np.full((spp, 1, W), 0x05, np.uint8)
        c1[1, 0, 2] = 0x9
        _refused(gpu_ctx, INV, p1, v[:, :1], c1)
    _refused(gpu_ctx, INV, p, None, ok)
    _refused(gpu_ctx, INV, p, v, None)
    _refused(gpu_ctx, INV, p, v, ok, null_image=True)
    _refused(gpu_ctx, INV, _params(W, H, -1, plane), v, ok)
    for kw in (dict(n_shards=3, shard_id=3), dict(n_shards=2, shard_id=-1)):
        _refused(gpu_ctx, INV, _params(W, H, spp, plane, tile_rows=1, **kw), v, ok)
    for extra in (capi.IPT_FLAG_PREVIEW, capi.IPT_FLAG_COUNTERS, 8):
        _refused(gpu_ctx, UNS, capi.make_params(W, H, spp, flags=rc.flag(plane) | extra), v, ok)
    # the size bound: 2^24 samples pass the check, one pass more does not
    # (zero pages, never touched: the call is refused before it reads them)
    big_v, big_c = np.zeros(4097 * 4096, np.float32), np.zeros(4097 * 4096, np.uint8)
    assert 4097 * 4096 > capi.IPT_REPLAY_MAX_SAMPLES == 1 << 24
    _refused(gpu_ctx, UNS, _params(4096, 1, 4097, plane), big_v, big_c)
    # sizes
    start = {k: np.full(W * H, SENTINEL[k], dt) for k, dt in dc.PLANE_KEYS}
    t = _to_device(start)
    for w, h in ((0, 4), (5, 0), (-5, 4), (65537, 1)):
        with pytest.raises(capi.IptError) as e:
            gpu_ctx.replay_samples(_params(w, h, 1, plane), big_v, big_c, *_ptrs(t))
        assert e.value.code == INV
    _assert_plane_equal(_to_host(t), start, what="image touched by a refused call")


@pytest.mark.parametrize("plane", rc.PLANES)
def test_zero_passes_is_a_no_op(gpu_ctx, plane):
    W, H = 5, 4
    start = {k: np.full(W * H, SENTINEL[k], dt) for k, dt in dc.PLANE_KEYS}
    t = _to_device(start)
    gpu_ctx.replay_samples(_params(W, H, 0, plane), np.zeros(0, np.float32), np.zeros(0, np.uint8), *_ptrs(t))
    _assert_plane_equal(_to_host(t), start)
