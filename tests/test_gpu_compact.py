"""Unit compaction (IPT_FLAG_COMPACT) on the device: the plan of a launch
(ipt_compact_plan) against tests/compact_cases.py's numpy restatement, and every
output of a flagged call against the same call without the flag and against
tests/adaptive_cases.py's replay -- bit for bit, no tolerance anywhere.
ipt_last_units is checked against the restatement's sums after the waits.
tests/test_compact_cpu.py pins, without a GPU, that the masks and frames hold
what this file relies on.

Without the feature this file fails at the first last_units or compact_plan
call (the library has neither entry point, the binding neither method)."""
import ctypes as C

import numpy as np
import pytest
import torch

import adaptive_cases as ac
import compact_cases as cc
import drift_cases as dc
import test_gpu_adaptive as tga
from ipt_amd import capi, scenes

pytestmark = pytest.mark.gpu

KEYS, BARE, DEV = tga.KEYS, tga.BARE, tga.DEV
COMPACT = capi.IPT_FLAG_COMPACT
fid = lambda f: "x".join(str(x) for x in f)


def _params(W, H, spp, plane, compact=False, **kw):
    kw["flags"] = kw.get("flags", 0) | (COMPACT if compact else 0)
    return cc.params(W, H, spp, plane, **kw)


def _pair(ctx, W, H, spp, plane, mask, valid=None, **kw):
    """The call without and with the flag: ((plane, m2), (plane, m2)); the
    flagged call's ipt_last_units against the restatement where `valid` is
    given, the unflagged call's three equal numbers."""
    pkw = {k: kw.pop(k) for k in ("flags", "spp_offset", "tile_rows", "n_shards", "shard_id") if k in kw}
    plain = tga._masked(ctx, _params(W, H, spp, plane, **pkw), mask, **kw)
    dense = ctx.last_units()
    assert dense[0] == dense[1] == dense[2] > 0
    got = tga._masked(ctx, _params(W, H, spp, plane, True, **pkw), mask, **kw)
    lu = ctx.last_units()
    assert lu[0] == dense[0] and lu[2] <= lu[1] <= lu[0]
    if valid is not None:
        assert lu == cc.last_units(valid)
    return plain, got


def _assert_same(plain, got, keys=KEYS, nan=False, what=""):
    tga._assert_plane_equal(got[0], plain[0], keys, what)
    if plain[1] is not None:
        (tga._assert_bits_nan if nan else tga._assert_bits)(got[1], plain[1], "m2 " + what)


# ---- the plan ----------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", cc.PLAN_FRAMES, ids=fid)
def test_plan(gpu_ctx, oracle, frame, plane):
    """src, n_active and start of the launch against the restatement, for every
    mask kind of the frame (NULL, all ones, all zero, half; n_active a
    multiple of 256, one more than a multiple, one)."""
    W, H, spp = frame
    tga._box(gpu_ctx)
    codes = ac.codes_of(W, H, spp, plane)
    for kind in cc.mask_kinds(frame):
        mask = cc.make_mask(kind, W, H, spp, plane)
        tmask = None if mask is None else tga._t(mask.reshape(-1))
        src, n, start = gpu_ctx.compact_plan(_params(W, H, spp, plane), None if tmask is None else tmask.data_ptr())
        rsrc, rn, rstart, _ = cc.plan(cc.valid_units(codes, mask, plane))
        assert (n, start) == (rn, rstart), kind
        assert np.array_equal(src, rsrc), (kind, np.flatnonzero(src != rsrc)[:8].tolist())


@pytest.mark.parametrize("plane", ac.PLANES)
def test_plan_sharded(gpu_ctx, oracle, plane):
    """Three shards of one-row tiles: a unit is a candidate row's, and the
    destination row's owner decides whether it is valid."""
    W, H, spp = 3, 60000, 2
    tga._box(gpu_ctx)
    codes = ac.codes_of(W, H, spp, plane)
    tmask = tga._t(ac.half_mask(W, H).reshape(-1))
    for s in range(3):
        owned, cand = cc.shard(W, H, plane, tile_rows=1, n_shards=3, shard_id=s)
        p = _params(W, H, spp, plane, tile_rows=1, n_shards=3, shard_id=s)
        for mask, ptr in ((None, None), (ac.half_mask(W, H), tmask.data_ptr())):
            src, n, start = gpu_ctx.compact_plan(p, ptr)
            rsrc, rn, rstart, _ = cc.plan(cc.valid_units(codes, mask, plane, owned, cand))
            assert (n, start) == (rn, rstart), (s, mask is None)
            assert np.array_equal(src, rsrc), (s, mask is None)


def test_plan_refusals(gpu_ctx, oracle):
    W, H, spp = 13, 11, 9
    tga._box(gpu_ctx)
    p = _params(W, H, spp, ac.GRID)
    src = np.zeros(4, np.uint32)
    n, start = C.c_uint64(), C.c_uint64()
    rc = gpu_ctx.lib.ipt_compact_plan(gpu_ctx.h, C.byref(p), None, src.ctypes.data, 4, C.byref(n), C.byref(start))
    assert rc == capi.IPT_E_INVALID and (n.value, start.value) == (W * H * spp, 0) and not src.any()
    with pytest.raises(capi.IptError) as e:
        gpu_ctx.compact_plan(_params(W, H, spp, ac.GRID, flags=capi.IPT_FLAG_PREVIEW))
    assert e.value.code == capi.IPT_E_UNSUPPORTED
    t = tga._to_device(dc.plane(W, H))
    v, c = tga._samples(W, H, spp, ac.GRID)
    with pytest.raises(capi.IptError) as e:  # the replay probe takes IPT_FLAG_GUI_PLANE alone
        gpu_ctx.replay_samples(_params(W, H, spp, ac.GRID, True), v, c, *tga._ptrs(t))
    assert e.value.code == capi.IPT_E_UNSUPPORTED


# ---- equality ----------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", cc.SMALL_FRAMES + cc.EXTRA_FRAMES[:1] + ac.HALF_FRAMES, ids=fid)
def test_flagged_equals_unflagged(gpu_ctx, oracle, frame, plane):
    """Pixels, counters, sums, pixel_max and m2 under every mask kind of the
    frame; the half mask against the numpy replay too, and without sums /
    pixel_max / m2."""
    W, H, spp = frame
    tga._box(gpu_ctx)
    v, c = tga._samples(W, H, spp, plane)
    for kind in cc.mask_kinds(frame):
        mask = cc.make_mask(kind, W, H, spp, plane)
        plain, got = _pair(gpu_ctx, W, H, spp, plane, mask, cc.valid_units(c, mask, plane))
        _assert_same(plain, got, what=kind)
        if kind == "half":
            ref, rm2 = ac.replay(v, c, mask, plane)
            tga._assert_plane_equal(got[0], ref, what="replay")
            tga._assert_bits(got[1], rm2, "m2, replay")
            plain, got = _pair(gpu_ctx, W, H, spp, plane, mask, keys=BARE, with_m2=False)
            assert got[1] is None
            _assert_same(plain, got, BARE, what="no sums / pixel_max / m2")
            tga._assert_plane_equal(got[0], ref, BARE, what="replay, bare")


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", ((13, 11, 9), (4099, 61, 2)), ids=fid)
def test_preloaded_planes(gpu_ctx, oracle, frame, plane):
    """Into drift_cases.preload's plane and a seeded m2: the flagged call
    continues them as the unflagged one and the replay do (m2 with
    test_gpu_adaptive._assert_bits_nan's rule: a NaN equals a NaN)."""
    W, H, spp = frame
    tga._box(gpu_ctx)
    v, c = tga._samples(W, H, spp, plane)
    pre, _ = dc.preload(W, H, spp)
    pm2 = np.random.default_rng(3).random(W * H, dtype=np.float32)
    for kind in ("half", "null", "zeros"):
        mask = cc.make_mask(kind, W, H, spp, plane)
        plain, got = _pair(gpu_ctx, W, H, spp, plane, mask, cc.valid_units(c, mask, plane), img=pre, m2=pm2)
        _assert_same(plain, got, nan=True, what=kind)
        ref, rm2 = ac.replay(v, c, mask, plane, img=dc.copy_plane(pre), m2=pm2.copy())
        tga._assert_plane_equal(got[0], ref, what="replay, " + kind)
        tga._assert_bits_nan(got[1], rm2, "m2, replay, " + kind)


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", ((13, 11, 9), (257, 5, 9), (60000, 3, 9)), ids=fid)
def test_counters(gpu_ctx, oracle, frame, plane):
    """IPT_FLAG_COUNTERS: all fifteen fields are the unflagged call's, and
    paths is the number of units the compaction kept."""
    W, H, spp = frame
    tga._box(gpu_ctx)
    c = ac.codes_of(W, H, spp, plane)
    for kind in ("half", "null", "zeros", "r1"):
        mask = cc.make_mask(kind, W, H, spp, plane)
        cnt = []
        for compact in (False, True):
            gpu_ctx.reset_counters()
            tga._masked(gpu_ctx, _params(W, H, spp, plane, compact, flags=capi.IPT_FLAG_COUNTERS), mask)
            cnt.append(gpu_ctx.counters())
        assert len(cnt[0]) == 15 and cnt[0] == cnt[1], kind
        assert cnt[1]["paths"] == gpu_ctx.last_units()[2] == ac.counts(c, mask, plane)[0], kind


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", ((13, 11, 9), (4099, 61, 2)), ids=fid)
def test_render_values(gpu_ctx, oracle, frame, plane):
    """ipt_render_values: the dense values and codes after the expansion."""
    W, H, spp = frame
    tga._box(gpu_ctx)
    v, c = tga._samples(W, H, spp, plane)
    pv, pcodes = gpu_ctx.render_values(_params(W, H, spp, plane))
    gv, gcodes = gpu_ctx.render_values(_params(W, H, spp, plane, True))
    assert gpu_ctx.last_units() == cc.last_units(cc.valid_units(c, None, plane))
    assert np.array_equal(gcodes, pcodes) and np.array_equal(gcodes, c)
    tga._assert_bits(gv, pv, "values")
    tga._assert_bits(gv, v, "values against the oracle")


# ---- launch paths ------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ac.PLANES)
def test_chunked_launches_and_the_stale_pad(oracle, monkeypatch, plane):
    """IPT_TEST_CHUNK_UNITS of three passes in a fresh context; 257 x 5, so a
    launch has 3855 or 2570 units. Consecutive launches alternate between the
    context's two work slots, and a call of five passes is two launches (3 + 2
    passes): launch k of the second call reuses the slot, and so the record
    buffer, of launch k of the first. The first call's mask is the half mask
    with every inactive byte of rows 1.. set (nearly everything valid: its
    compact range begins near the front of the buffer), the second call's is
    the half mask: its compact range begins about half-way, so its pad -- the
    positions from the chunk boundary below that begin -- lies where the first
    call left records with valid = 1. A pad that was not rewritten would be
    traced: the values would still be right (a ghost path stores into the
    compact values, outside the expanded range), so the counters are what
    shows it -- paths and traced_rays above the unflagged call's. A third
    call of eight passes is three launches in one call."""
    W, H = 257, 5
    per_pass = W * H
    dense = ac.half_mask(W, H).copy()
    dense[1:] = 1
    half = ac.half_mask(W, H)
    calls = ((5, 0, dense), (5, 5, half), (8, 10, half))
    v, c = tga._samples(W, H, 18, plane)
    plans, residues = [], []
    for spp, off, mask in calls:
        lp = cc.launch_plans(cc.valid_units(c[off:off + spp], mask, plane), 3 * per_pass)
        plans.append(lp)
        residues += [p[1] % 256 for p in lp]
    assert [len(lp) for lp in plans] == [2, 2, 3] and len(set(residues)) >= 4
    for k in range(2):  # the second call's pads lie inside the first call's compact ranges
        (_, _, _, first_a), (_, _, start_b, first_b) = plans[0][k], plans[1][k]
        assert first_a < start_b < first_b
    monkeypatch.setenv("IPT_TEST_CHUNK_UNITS", str(3 * per_pass))
    out = {}
    for compact in (False, True):
        ctx = capi.Context(0)
        try:
            tga._box(ctx)
            t, tm2 = tga._to_device(dc.plane(W, H)), tga._t(np.zeros(W * H, np.float32))
            cnts, units = [], []
            for spp, off, mask in calls:
                ctx.reset_counters()
                tmask = tga._t(mask.reshape(-1))
                ctx.render_masked_device(_params(W, H, spp, plane, compact, spp_offset=off, flags=capi.IPT_FLAG_COUNTERS),
                                         *tga._ptrs(t), mask_ptr=tmask.data_ptr(), m2_ptr=tm2.data_ptr())
                torch.cuda.synchronize()
                cnts.append(ctx.counters())
                units.append(ctx.last_units())
            out[compact] = (tga._to_host(t), tga._h(tm2), cnts, units)
        finally:
            ctx.close()
    tga._assert_plane_equal(out[True][0], out[False][0], what="three chunked calls")
    tga._assert_bits(out[True][1], out[False][1], "m2")
    assert out[True][2] == out[False][2]
    ref, rm2 = dc.plane(W, H), np.zeros(W * H, np.float32)
    for (spp, off, mask), cnt, lu_c, lu_d in zip(calls, out[True][2], out[True][3], out[False][3]):
        ac.replay(v[off:off + spp], c[off:off + spp], mask, plane, ref, rm2)
        valid = cc.valid_units(c[off:off + spp], mask, plane)
        assert lu_c == cc.last_units(valid, 3 * per_pass)
        assert lu_d == cc.last_units(valid, 3 * per_pass, compact=False)
        assert cnt["paths"] == lu_c[2] == int(valid.sum())
    tga._assert_plane_equal(out[True][0], ref, what="replay")
    tga._assert_bits(out[True][1], rm2, "m2, replay")


@pytest.mark.parametrize("plane", ac.PLANES)
def test_queued_mixes(gpu_ctx, oracle, plane):
    """Five async calls of two passes into one image on one stream: unflagged
    unmasked, flagged masked, a masked preview (with the flag, which it
    ignores), unflagged masked, flagged unmasked. The planes are those of the
    same calls made one by one without the flag; ipt_last_units after the wait
    sums the four full-estimator calls."""
    W, H, n = 257, 5, 2
    tga._box(gpu_ctx)
    mask = ac.half_mask(W, H)
    c = ac.codes_of(W, H, 5 * n, plane)
    seq = ((0, False, False), (COMPACT, True, False), (COMPACT | capi.IPT_FLAG_PREVIEW, True, True),
           (0, True, False), (COMPACT, False, False))
    tmask = tga._t(mask.reshape(-1))
    # one by one, unflagged
    t, tm2 = tga._to_device(dc.plane(W, H)), tga._t(np.zeros(W * H, np.float32))
    for k, (flags, masked, _) in enumerate(seq):
        gpu_ctx.render_masked_device(_params(W, H, n, plane, spp_offset=k * n, flags=flags & ~COMPACT), *tga._ptrs(t),
                                     mask_ptr=tmask.data_ptr() if masked else None,
                                     m2_ptr=tm2.data_ptr() if masked else None)
    torch.cuda.synchronize()
    ref, rm2 = tga._to_host(t), tga._h(tm2)
    s = torch.cuda.Stream(DEV)
    t, tm2 = tga._to_device(dc.plane(W, H)), tga._t(np.zeros(W * H, np.float32))
    want = [0, 0, 0]
    with torch.cuda.stream(s):
        for k, (flags, masked, preview) in enumerate(seq):
            gpu_ctx.render_masked_device_async(_params(W, H, n, plane, spp_offset=k * n, flags=flags), *tga._ptrs(t),
                                               mask_ptr=tmask.data_ptr() if masked else None,
                                               m2_ptr=tm2.data_ptr() if masked else None, stream=s.cuda_stream)
            if not preview:
                lu = cc.last_units(cc.valid_units(c[k * n:(k + 1) * n], mask if masked else None, plane),
                                   compact=bool(flags & COMPACT))
                want = [a + b for a, b in zip(want, lu)]
    s.synchronize()
    gpu_ctx.wait()
    tga._assert_plane_equal(tga._to_host(t), ref, what="queued mix")
    tga._assert_bits(tga._h(tm2), rm2, "m2, queued mix")
    assert gpu_ctx.last_units() == tuple(want) and want[1] < want[0]


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("tile,n_shards", ((1, 3), (16, 2)))
def test_sharded(gpu_ctx, oracle, tile, n_shards, plane):
    """Every shard, with and without a mask: the planes are the unflagged
    ones, and the pool hands out fewer units than the launch has by the
    restatement's amount (the other shards' halo rows are gone)."""
    W, H, spp = 3, 60000, 2
    tga._box(gpu_ctx)
    c = ac.codes_of(W, H, spp, plane)
    for s in range(n_shards):
        kw = dict(tile_rows=tile, n_shards=n_shards, shard_id=s)
        owned, cand = cc.shard(W, H, plane, **kw)
        for mask in (None, ac.half_mask(W, H)):
            plain, got = _pair(gpu_ctx, W, H, spp, plane, mask, cc.valid_units(c, mask, plane, owned, cand), **kw)
            _assert_same(plain, got, what="shard %d" % s)
            lu = gpu_ctx.last_units()
            assert lu[0] == spp * len(cand) * W and lu[1] < lu[0]


# ---- the loop ----------------------------------------------------------------------------
def _loop_units(c, rounds, n_rounds, plane):
    want, mask = [0, 0, 0], None
    for r in range(n_rounds):
        lu = cc.last_units(cc.valid_units(c[r * ac.LOOP_ROUND:(r + 1) * ac.LOOP_ROUND], mask, plane))
        want = [a + b for a, b in zip(want, lu)]
        mask = rounds[r][2]
    return tuple(want)


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", ac.LOOP_FRAMES, ids=fid)
def test_render_adaptive(gpu_ctx, oracle, frame, plane):
    """ipt_render_adaptive with the flag, capped at each round in turn: plane,
    m2, mask, stats and passes are the unflagged loop's (and the numpy
    loop's); ipt_last_units sums the call's rounds."""
    W, H = frame
    tga._box(gpu_ctx)
    v, c = tga._samples(W, H, ac.LOOP_SPP, plane)
    rounds, _ = ac.loop(v, c, plane, ac.LOOP_ROUND, **ac.LOOP_ADAPT)
    ap = capi.make_adapt_params(W, H, flags=ac.FLAG[plane], **ac.LOOP_ADAPT)
    for k, (img, m2, mask, stats) in enumerate(rounds, 1):
        res = []
        for compact in (False, True):
            got, gm2, gmask = dc.plane(W, H), np.zeros(W * H, np.float32), np.zeros(W * H, np.uint8)
            st = gpu_ctx.render_adaptive(_params(W, H, k * ac.LOOP_ROUND, plane, compact), ap, ac.LOOP_ROUND, got, gm2, gmask)
            res.append((got, gm2, gmask, st))
        tga._assert_plane_equal(res[1][0], res[0][0], what="cap %d passes" % (4 * k))
        tga._assert_bits(res[1][1], res[0][1], "m2")
        assert np.array_equal(res[1][2], res[0][2]) and res[1][3] == res[0][3]
        tga._assert_plane_equal(res[1][0], img, what="numpy loop, cap %d passes" % (4 * k))
        assert np.array_equal(res[1][2], mask) and res[1][3]["passes"] == k * ac.LOOP_ROUND
        lu = gpu_ctx.last_units()
        assert lu == _loop_units(c, rounds, k, plane)
    assert lu[1] < lu[0]


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", ac.LOOP_FRAMES, ids=fid)
def test_loop_device_resident(gpu_ctx, oracle, frame, plane):
    """Flagged render_masked -> adapt, every round queued on one stream with no
    host wait in between, against the numpy loop (which the unflagged loop
    equals, test_gpu_adaptive.py) round for round."""
    W, H = frame
    tga._box(gpu_ctx)
    v, c = tga._samples(W, H, ac.LOOP_SPP, plane)
    rounds, _ = ac.loop(v, c, plane, ac.LOOP_ROUND, **ac.LOOP_ADAPT)
    ap = capi.make_adapt_params(W, H, flags=ac.FLAG[plane], **ac.LOOP_ADAPT)
    s = torch.cuda.Stream(DEV)
    t, tm2 = tga._to_device(dc.plane(W, H)), tga._t(np.zeros(W * H, np.float32))
    tmask = torch.zeros(W * H, dtype=torch.uint8, device=DEV)
    tstats = torch.zeros(4, dtype=torch.int32, device=DEV)
    snaps = []
    with torch.cuda.stream(s):
        for r in range(len(rounds)):
            gpu_ctx.render_masked_device_async(
                _params(W, H, ac.LOOP_ROUND, plane, True, spp_offset=r * ac.LOOP_ROUND), *tga._ptrs(t),
                mask_ptr=tmask.data_ptr() if r else None, m2_ptr=tm2.data_ptr(), stream=s.cuda_stream)
            gpu_ctx.adapt_device(ap, t["pixels"].data_ptr(), t["counters"].data_ptr(), tm2.data_ptr(),
                                 tmask.data_ptr(), tstats.data_ptr(), s.cuda_stream)
            snaps.append(({k: x.clone() for k, x in t.items()}, tm2.clone(), tmask.clone(), tstats.clone()))
    s.synchronize()
    gpu_ctx.wait()
    for r, ((img, m2, mask, stats), (gi, gm2, gmask, gstats)) in enumerate(zip(rounds, snaps)):
        tga._assert_plane_equal(tga._to_host(gi), img, what="round %d" % r)
        tga._assert_bits(tga._h(gm2), m2, "m2, round %d" % r)
        assert np.array_equal(tga._h(gmask), mask), r
        assert tga._h(gstats).tolist() == stats.tolist(), r
    lu = gpu_ctx.last_units()
    assert lu == _loop_units(c, rounds, len(rounds), plane) and lu[1] < lu[0]


# ---- other geometry and lights -----------------------------------------------------------
@pytest.mark.parametrize("scene", ("spheres", "lattice"))
def test_other_instances(gpu_ctx, scene):
    """A sphere-list scene (300 spheres) and the 25-light lattice: their path
    kernel instances refill through the same pool with other workgroup sizes
    and wave counts. 64 x 8 x 3 (1536 units, six chunks) with the half mask:
    planes, m2 and all counters are the unflagged call's."""
    W, H, spp = 64, 8, 3
    gpu_ctx.upload_scene(scenes.make_scene_spheres(300) if scene == "spheres" else scenes.make_scene_box_lights(5))
    mask = ac.half_mask(W, H)
    res = []
    for compact in (False, True):
        gpu_ctx.reset_counters()
        res.append(tga._masked(gpu_ctx, _params(W, H, spp, ac.GRID, compact, flags=capi.IPT_FLAG_COUNTERS), mask))
        res[-1] += (gpu_ctx.counters(), gpu_ctx.last_units())
    tga._assert_plane_equal(res[1][0], res[0][0], what=scene)
    tga._assert_bits(res[1][1], res[0][1], "m2")
    assert res[1][2] == res[0][2] and res[1][2]["paths"] > 0 and res[1][0]["pixels"].any()
    dense, lu = res[0][3], res[1][3]
    assert dense == (W * H * spp,) * 3
    assert lu[0] == dense[0] and lu[2] == res[1][2]["paths"] and lu[1] == lu[0] - (lu[0] - lu[2]) // 256 * 256 < lu[0]
