"""The drift frames of tests/drift_cases.py bite: conditions checked with the
CPU oracle alone (no GPU).

tests/test_gpu_drift.py compares accumulate_kernel's drift branch with the
oracle on these frames. That comparison is only worth something while the
frames hold drifted samples of the right kinds, with radiance, at the special
rows and across shard boundaries -- and while a replay that gets the drift
wrong would actually produce a different plane. Each of those is asserted
here, with the measured counts pinned."""
import numpy as np
import pytest

import drift_cases as dc
import oracle_binding as ob
from ipt_amd import capi, scenes

bits = dc.bits


@pytest.mark.parametrize("key", sorted(dc.HIST), ids=lambda k: "%dx%dx%d" % k)
def test_code_histogram_pinned(oracle, key):
    W, H, spp = key
    v, c, cnt = dc.oracle_samples(W, H, spp)
    assert dc.histogram(c) == dc.HIST[key]
    assert 0xff not in dc.HIST[key] and 0xfe not in dc.HIST[key]
    assert cnt["drifted"] == sum(dc.HIST[key].values())
    d = c != 0x05
    assert int((v[d] > 0).sum()) == dc.NONZERO[key]


@pytest.mark.parametrize("frame", dc.THIN + (dc.MAX_HEIGHT,), ids=lambda f: "%dx%d" % f)
def test_thin_frames_hold_enough_drift(frame):
    """The floors, on the pinned numbers: >= 100 drifted samples per thin
    frame at the fewest passes it is rendered with, >= 50 of them with a
    non-zero radiance."""
    key = frame + (2,)
    assert sum(dc.HIST[key].values()) >= 100
    assert dc.NONZERO[key] >= 50


def test_each_direction_is_present():
    for spp in dc.SPPS:
        assert {0x4, 0x6} <= set(dc.HIST[dc.WIDE + (spp,)])   # dx = -1, +1
        assert {0x1, 0x9} <= set(dc.HIST[dc.TALL + (spp,)])   # dy = -1, +1
    # the mixed frame drifts along both axes in one render
    assert {0x6, 0x9} <= set(dc.HIST[dc.MIXED + (2,)])


@pytest.mark.parametrize("case", dc.DIAGONAL, ids=lambda c: "%#x-pass%d" % (c[0], c[3]))
def test_diagonal_sample(oracle, case):
    """The diagonal passes hold their code where pinned, once, and the oracle's
    value there is non-zero at the tree the GPU test uses (and zero one ray or
    one level below: the tree is the shallowest that serves)."""
    code, n, seed, off, ix, iy, n_rays, depth_max, value = case
    assert capi.make_params(1, 1, 1).seed == dc.DEFAULT_SEED
    _, c, _ = dc.oracle_samples(n, n, 1, off, 0, 0, seed)  # codes do not depend on the tree
    diag = np.argwhere(~np.isin(c, (0x01, 0x04, 0x05, 0x06, 0x09)))
    assert diag.tolist() == [[0, iy, ix]] and c[0, iy, ix] == code
    desc = scenes.make_scene_box()

    def at(nr, dm):
        p = capi.make_params(n, n, 1, spp_offset=off, n_rays=nr, depth_max=dm, seed=seed)
        return float(ob.render_rows_values(desc, p, n, iy, n, ix, n_threads=1)[0].ravel()[0])

    assert at(n_rays, depth_max) == value and value > 0
    assert at(n_rays, depth_max - 1) == 0 and at(n_rays - 1, depth_max) == 0


def test_diagonal_codes_accounted_for():
    """0x0 and 0x2 are still unreached by a render; the replay probe's cases
    (tests/replay_cases.py) reach them, and every other drift code."""
    import replay_cases as rc

    assert {c[0] for c in dc.DIAGONAL} | set(dc.DIAGONAL_UNREACHED) == {0x0, 0x2, 0x8, 0xa}
    assert not {c[0] for c in dc.DIAGONAL} & set(dc.DIAGONAL_UNREACHED)
    assert set(rc.DIAG_DOWN) == set(dc.DIAGONAL_UNREACHED)
    assert set(rc.DRIFT_CODES) == {dx | dy << 2 for dx in range(3) for dy in range(3)} - {0x05}
    for plane in rc.PLANES:
        for code in dc.DIAGONAL_UNREACHED:
            _, c = rc.single_code(code, *rc.SINGLE_FRAME, rc.SINGLE_SPP, plane)
            assert int((c == code).sum()) >= c.size // 3


@pytest.mark.parametrize("frame", dc.THIN + (dc.SMALL,), ids=lambda f: "%dx%d" % f)
def test_numpy_replay_is_the_oracles(oracle, frame):
    """The numpy replay in raster order is ob.accumulate, bit for bit: what the
    wrong variants below change is the only thing wrong with them."""
    v, c, _ = dc.oracle_samples(*frame, 2)
    ref, got = dc.oracle_plane(*frame, 2), dc.replay(v, c)
    for k in ref:
        assert np.array_equal(bits(got[k]), bits(ref[k])), k


@pytest.mark.parametrize("frame", dc.THIN, ids=lambda f: "%dx%d" % f)
def test_wrong_replays_discriminate(oracle, frame):
    """A replay that drops the drifted samples, and one that adds a pass's
    drifted samples after its nominal ones, give other pixels than the oracle.

    The second is wrong only where a drifted sample precedes its destination's
    nominal sample (dc.ORDER_SENSITIVE); the frames that are two pixels wide
    and tall hold 0x9 alone, where both orders are the raster's, so there the
    check is that the deferred replay changes nothing."""
    v, c, _ = dc.oracle_samples(*frame, 2)
    ref = dc.oracle_plane(*frame, 2)
    dropped = dc.replay(v, c, "nominal_only")
    assert (bits(dropped["pixels"]) != bits(ref["pixels"])).any()
    assert (dropped["counters"] != ref["counters"]).any()
    deferred = dc.replay(v, c, "drift_last")
    assert np.array_equal(deferred["counters"], ref["counters"])
    differs = bool((bits(deferred["pixels"]) != bits(ref["pixels"])).any())
    assert differs == bool(set(dc.HIST[frame + (2,)]) & set(dc.ORDER_SENSITIVE))
    if frame in (dc.WIDE, dc.TALL):
        assert differs


@pytest.mark.parametrize("frame,tile,n_shards", [(f, t, n) for f, plans in dc.SHARD_PLANS.items() for t, n in plans],
                         ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_sharded_plans_cut_through_drift(oracle, frame, tile, n_shards):
    _, c, _ = dc.oracle_samples(*frame, dc.SHARD_SPP[frame])
    n = dc.cross_shard(c, tile, n_shards)
    assert n == dc.CROSS[frame, tile, n_shards]
    if frame == dc.TALL and tile == 1:
        assert n >= 20
    # the owner of a row, restated here, is ipt_shard_plan's
    for s in range(n_shards):
        owned, _ = capi.shard_plan(capi.make_params(*frame, 1, tile_rows=tile, n_shards=n_shards, shard_id=s))
        assert np.array_equal(owned, dc.shard_of(np.arange(frame[1]), tile, n_shards) == s)


def test_tall_variants_cut_through_drift(oracle):
    _, c, _ = dc.oracle_samples(*dc.TALL, 4)
    assert dc.cross_shard(c, 1, 3) == dc.CROSS_TALL_SPP4 >= 20


# drifted samples by (frame, spp) at the special rows: source rows H-2 and H-1
# (both nominally row 0), destination row H-1 (which receives nothing but
# dy = +1 drift of source row 0), destination row 0. The tall frames drift at
# their high source rows only and hold none of these; the wide ones hold the
# first two and the last in every pass, and two samples into row H-1 (of
# radiance zero: they show in the counters and the means) in passes 7 and 8.
SPECIAL = {
    (dc.WIDE, 2): (137, 156, 0, 293),
    (dc.WIDE, 9): (645, 692, 2, 1337),
    (dc.WIDE_MAX, 2): (182, 162, 0, 344),
    (dc.WIDE_MAX, 9): (767, 767, 2, 1532),
    (dc.MIXED, 9): (1, 5, 1, 6),
    (dc.TALL, 2): (0, 0, 0, 0),
}


@pytest.mark.parametrize("key", SPECIAL, ids=lambda k: "%dx%dx%d" % (k[0] + (k[1],)))
def test_special_rows_hold_drift(oracle, key):
    (W, H), spp = key
    _, c, _ = dc.oracle_samples(W, H, spp)
    _, yi, _ = dc.destinations(c)
    d = c != 0x05
    got = (int(d[:, H - 2].sum()), int(d[:, H - 1].sum()), int((d & (yi == H - 1)).sum()), int((d & (yi == 0)).sum()))
    assert got == SPECIAL[key]
    if (W, H) in (dc.WIDE, dc.WIDE_MAX):
        assert min(got[0], got[1], got[3]) >= 100
        assert (got[2] >= 1) == (spp == 9)


def test_preload_puts_every_kind_on_drifted_pixels(oracle):
    """Each preloaded kind of each array sits on drifted destination pixels of
    the wide frame, no counter can wrap, and no pairing generates a NaN."""
    W, H = dc.WIDE
    for spp in dc.SPPS:
        _, c, _ = dc.oracle_samples(W, H, spp)
        _, yi, xi = dc.destinations(c)
        d = c != 0x05
        hot = np.unique(yi[d] * W + xi[d])
        img, pick = dc.preload(W, H, spp, hot)
        kinds = dc.preload_kinds(spp)
        for k, names in kinds.items():
            n = np.bincount(pick[k][hot], minlength=len(names))
            assert n.min() >= 3, (k, n)
        ref = dc.oracle_plane(W, H, spp)
        assert int(img["counters"].astype(np.uint64).max() + ref["counters"].max()) < 0xffffffff
        assert not (np.isinf(img["pixels"]) & (img["counters"] == 0)).any()
        assert (np.isinf(img["pixels"]) & (img["counters"] > 0)).any()
    for spp in dc.SMALL_SPPS:
        img, pick = dc.preload(*dc.SMALL, spp)
        for k, names in dc.preload_kinds(spp).items():
            assert len(np.unique(pick[k])) == len(names), k
