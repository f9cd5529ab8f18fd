"""Unit compaction without a GPU: the masks and frames tests/test_gpu_compact.py
plans and renders hold the properties it relies on (every n_active residue the
pool's start depends on, frames below and across the pool's chunk, a block scan
longer than one workgroup), and the restatement (tests/compact_cases.py) tells
three wrong plans from the right one on them."""
from pathlib import Path

import numpy as np
import pytest

import adaptive_cases as ac
import compact_cases as cc
from ipt_amd import capi


def _valid(frame, plane, kind, **shard):
    W, H, spp = frame
    codes = ac.codes_of(W, H, spp, plane)
    mask = cc.make_mask(kind, W, H, spp, plane)
    if shard:
        owned, cand = cc.shard(W, H, plane, **shard)
        return cc.valid_units(codes, mask, plane, owned, cand)
    return cc.valid_units(codes, mask, plane)


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", cc.R1_FRAMES, ids=lambda f: "%dx%dx%d" % f)
def test_residue_masks(oracle, frame, plane):
    """n_active % 256 == 0 with n_active > 0 (the pool starts at the compact
    range itself) and n_active % 256 == 1 (a pad of all but one unit of a
    chunk, where the frame is that large)."""
    for kind, residue in (("r0", 0), ("r1", 1)):
        if kind not in cc.mask_kinds(frame):
            continue
        v = _valid(frame, plane, kind)
        _, n, start, first = cc.plan(v)
        assert 0 < n < v.size and n % 256 == residue
        assert first == v.size - n and start == first // 256 * 256 and start <= first < start + 256
    v = _valid(frame, plane, "half")
    assert 0 < cc.plan(v)[1] < v.size


@pytest.mark.parametrize("plane", ac.PLANES)
def test_corner_masks_and_frames(oracle, plane):
    W, H, spp = cc.ONE_FRAME
    src, n, start, first = cc.plan(_valid(cc.ONE_FRAME, plane, "one"))
    assert n == 1 and first == W * H - 1 and start == (W * H - 1) // 256 * 256 == 0
    totals = {}
    for frame in cc.PLAN_FRAMES:
        v = _valid(frame, plane, "zeros")
        src, n, start, first = cc.plan(v)
        totals[frame] = v.size
        # nothing valid: the pool starts at the last chunk's begin, or at the end
        assert n == 0 and first == v.size and start == v.size // 256 * 256
        assert (start == v.size) == (v.size % 256 == 0)
    assert totals[(64, 8, 3)] % 256 == 0 and totals[(64, 8, 3)] > 0
    assert totals[(13, 11, 9)] % 256 != 0 and totals[(13, 11, 9)] > 256
    assert all(totals[f] < 256 for f in ((1, 1, 9), (2, 2, 9), (5, 4, 9), (13, 11, 1)))
    # the block-count scan: more 256-unit blocks than one 256-thread workgroup has threads
    assert totals[(60000, 3, 9)] // 256 == 6328 > 256
    # an unmasked launch drops only samples without a destination; the small frames have none
    for frame in cc.SMALL_FRAMES:
        assert cc.plan(_valid(frame, plane, "null"))[1] == totals[frame]
    # a mask byte of 0xff is active like 1
    assert cc.same_plan(cc.plan(_valid((13, 11, 9), plane, "ones")), cc.plan(_valid((13, 11, 9), plane, "null")))


@pytest.mark.parametrize("plane", ac.PLANES)
def test_sharded_plans_drop_halo_rows(oracle, plane):
    """Three shards of one-row tiles: every source row is a candidate of every
    shard's neighbours, so about two thirds of a shard's units are other
    shards' (exactly: the destination row's owner decides)."""
    W, H, spp = 3, 60000, 2
    seen = np.zeros((spp, H, W), np.int32)
    for s in range(3):
        owned, cand = cc.shard(W, H, plane, tile_rows=1, n_shards=3, shard_id=s)
        v = cc.valid_units(ac.codes_of(W, H, spp, plane), None, plane, owned, cand)
        assert v.shape == (spp, len(cand), W) and len(cand) > H // 2
        _, n, start, first = cc.plan(v)
        assert 0 < n < v.size * 0.4 and start > 0
        seen[:, cand, :] += v
    # every sample with a destination is traced by exactly one shard
    assert np.array_equal(seen, (ac.codes_of(W, H, spp, plane) < 0x10).astype(np.int32))


@pytest.mark.parametrize("plane", ac.PLANES)
def test_wrong_plans_differ(oracle, plane):
    """front: wherever something is dropped; unrounded: wherever the compact
    range does not begin on a chunk; descending: wherever two units are valid."""
    differs = {"front": 0, "unrounded": 0, "descending": 0}
    for frame in cc.PLAN_FRAMES:
        for kind in cc.mask_kinds(frame):
            v = _valid(frame, plane, kind)
            right = cc.plan(v)
            _, n, start, first = right
            for how, must in (("front", n < v.size), ("unrounded", first % 256 != 0), ("descending", n >= 2)):
                d = not cc.same_plan(cc.plan(v, how), right)
                assert d == must, (frame, kind, how)
                differs[how] += d
    assert all(differs.values())
    for frame in ((13, 11, 9), (60000, 3, 9)):
        for kind in ("half", "r1"):
            v = _valid(frame, plane, kind)
            assert not any(cc.same_plan(cc.plan(v, how), cc.plan(v)) for how in differs), (frame, kind)


def test_last_units_over_chunks(oracle):
    """The chunked call of test_gpu_compact.py: three launches of three passes
    whose n_active differ modulo 256, summed as ipt_last_units does."""
    W, H, spp = 13, 11, 9
    assert cc.launches(spp, W * H, 3 * W * H) == [(0, 3), (3, 3), (6, 3)]
    assert cc.launches(spp, W * H, 1) == [(s, 1) for s in range(9)]
    assert cc.launches(spp, W * H) == [(0, 9)]
    for plane in ac.PLANES:
        v = _valid((W, H, spp), plane, "half")
        plans = cc.launch_plans(v, 3 * W * H)
        assert len(plans) == 3
        total = 3 * W * H
        assert cc.last_units(v, 3 * W * H) == (3 * total, sum(total - p[2] for p in plans), sum(p[1] for p in plans))
        assert cc.last_units(v, 3 * W * H, compact=False) == (3 * total,) * 3
        # (a launch of 429 units with half of them valid: the compact range begins below 256,
        # so its pool hands out every unit -- the saving starts where a launch drops a chunk)
        assert cc.last_units(v, 3 * W * H)[1] == 3 * total


def test_binding_declares_the_entry_points():
    assert capi.IPT_FLAG_COMPACT == 8
    for name in ("ipt_last_units", "ipt_compact_plan"):
        assert name in capi.EXPORTED_SYMBOLS
    hdr = (Path(__file__).resolve().parents[1] / "include" / "ipt_capi.h").read_text()
    assert "IPT_FLAG_COMPACT = 8u" in hdr
    lib = capi.load()
    assert hasattr(lib, "ipt_last_units") and hasattr(lib, "ipt_compact_plan")
