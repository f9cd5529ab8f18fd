"""Unit compaction (IPT_FLAG_COMPACT) restated in numpy: which
work units of a launch are valid, the compact order, where the compact range
lies in the dense index range and where the pool starts; ipt_last_units summed
over a call's launches; and three wrong plans the CPU test must tell from the
right one. Shared by tests/test_compact_cpu.py (the conditions the chosen masks
must hold, oracle only) and tests/test_gpu_compact.py (the same cases through
the kernels). Built on adaptive_cases and drift_cases; changes nothing there.

A launch's dense unit is (pass, candidate row, column), pass-major. A unit is
valid when its sample has a destination (code != 0xff), its NOMINAL destination
pixel is not masked and its destination ROW is owned by the shard. Valid unit
number j, in ascending dense order, gets the compact index total - n_active +
j; the pool starts at that range's begin rounded down to the pool's chunk."""
import numpy as np

import adaptive_cases as ac
import drift_cases as dc
from ipt_amd import capi

POOL_CHUNK = 256

SMALL_FRAMES = ((1, 1, 9), (2, 2, 9), (5, 4, 9), (13, 11, 9), (257, 5, 9))
# total_units a multiple of 256 (1536); one pass, for the mask with one valid unit
EXTRA_FRAMES = ((64, 8, 3), (13, 11, 1))
PLAN_FRAMES = SMALL_FRAMES + EXTRA_FRAMES + ac.HALF_FRAMES
# frames with an odd number of passes and enough pixels: a flipped mask byte
# moves n_active by spp (twice that in the Grid map's row 0), and spp is
# coprime to 256, so every residue is within 256 flips. 13 x 11 x 9 has too few
# units for a multiple of both 9 and 256: it gets the residue 1 (513) alone
RESIDUE_FRAMES = ((257, 5, 9), (64, 8, 3), (60000, 3, 9))
R1_FRAMES = RESIDUE_FRAMES + ((13, 11, 9),)
ONE_FRAME = (13, 11, 1)
MASK_KINDS = ("null", "ones", "zeros", "half", "r0", "r1")


def params(W, H, spp, plane, **kw):
    kw["flags"] = kw.get("flags", 0) | ac.FLAG[plane]
    return dc.params(W, H, spp, **kw)


def shard(W, H, plane, tile_rows=0, n_shards=1, shard_id=0):
    """(owned rows bool[H], candidate source rows) of a plan, by ipt_shard_plan."""
    return capi.shard_plan(params(W, H, 1, plane, tile_rows=tile_rows, n_shards=n_shards, shard_id=shard_id))


def valid_units(codes, mask, plane, owned=None, cand=None):
    """bool [spp][n_cand][W]: the units a launch over codes' passes traces."""
    spp, H, W = codes.shape
    act = ac.active_samples(codes, mask, plane)
    if owned is not None:
        _, yi, _ = ac.destinations(codes, plane)
        act = act & np.asarray(owned, bool)[np.clip(yi, 0, H - 1)]
    return act if cand is None else act[:, np.asarray(cand, np.int64), :]


def plan(valid, how="right"):
    """(src, n_active, start, first): the dense units in compact order, their
    number, the pool's first unit and the compact index of src[0].
    how: "right"; wrong: "front" (the compact units at the front of the index
    range), "unrounded" (the pool starts at the compact range itself),
    "descending" (the compact order reversed)."""
    v = np.asarray(valid).reshape(-1)
    total = v.size
    src = np.flatnonzero(v).astype(np.uint32)
    n = int(src.size)
    first = total - n
    start = first // POOL_CHUNK * POOL_CHUNK
    if how == "front":
        first = start = 0
    elif how == "unrounded":
        start = first
    elif how == "descending":
        src = src[::-1].copy()
    elif how != "right":
        raise ValueError(how)
    return src, n, start, first


def same_plan(a, b):
    return np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def launches(spp, per_pass, chunk_units=None):
    """The passes [(s0, ns)] of a call's launches: render_chunks' equal chunks
    under IPT_TEST_CHUNK_UNITS (None: one launch; the frames here are far
    below the memory budget)."""
    if chunk_units is None:
        return [(0, spp)]
    budget = max(per_pass, chunk_units)
    n_chunks = max(1, (spp * per_pass + budget - 1) // budget)
    chunk = max(1, (spp + n_chunks - 1) // n_chunks)
    while chunk > 1 and chunk * per_pass > budget:
        chunk -= 1
    return [(s0, min(chunk, spp - s0)) for s0 in range(0, spp, chunk)]


def launch_plans(valid, chunk_units=None):
    """plan() of each launch of a call over valid's passes."""
    spp = valid.shape[0]
    per_pass = valid[0].size
    return [plan(valid[s0:s0 + ns]) for s0, ns in launches(spp, per_pass, chunk_units)]


def last_units(valid, chunk_units=None, compact=True):
    """ipt_last_units of one call: (dense, handed out, traced)."""
    spp = valid.shape[0]
    per_pass = valid[0].size
    out = [0, 0, 0]
    for s0, ns in launches(spp, per_pass, chunk_units):
        total = ns * per_pass
        _, n, start, _ = plan(valid[s0:s0 + ns])
        out[0] += total
        out[1] += total - start if compact else total
        out[2] += n if compact else total
    return tuple(out)


def residue_mask(W, H, spp, plane, residue):
    """The seeded half mask with single bytes flipped, in pixel order, until
    n_active % 256 == residue (and n_active > 0)."""
    codes = ac.codes_of(W, H, spp, plane)
    yn, _, _ = ac.destinations(codes, plane)
    ix = np.broadcast_to(np.arange(W, dtype=np.int64)[None, None, :], codes.shape)
    # active samples per nominal pixel, were the pixel active
    per_px = np.bincount((yn * W + ix)[codes < 0x10], minlength=W * H)
    for to in (0, 1):  # clearing active bytes; if that runs out (a small frame), setting inactive ones
        mask = ac.half_mask(W, H).copy()
        flat = mask.reshape(-1)
        n = int(per_px[flat != 0].sum())
        for k in np.flatnonzero(((flat != 0) == (to == 0)) & (per_px > 0)):
            if n % POOL_CHUNK == residue and n > 0:
                break
            flat[k] = to
            n += int(per_px[k]) * (1 if to else -1)
        if n % POOL_CHUNK == residue and n > 0:
            return mask
    raise AssertionError((W, H, spp, plane, residue))


def make_mask(kind, W, H, spp, plane):
    """The mask of a kind (MASK_KINDS, or "one": a single active pixel off the
    Grid map's folded row), None for "null"."""
    if kind == "null":
        return None
    if kind == "ones":
        return np.ones((H, W), np.uint8)
    if kind == "zeros":
        return np.zeros((H, W), np.uint8)
    if kind == "half":
        return ac.half_mask(W, H)
    if kind == "r0":
        return residue_mask(W, H, spp, plane, 0)
    if kind == "r1":
        return residue_mask(W, H, spp, plane, 1)
    if kind == "one":
        m = np.zeros((H, W), np.uint8)
        m[H // 2, W // 2] = 1
        return m
    raise ValueError(kind)


def mask_kinds(frame):
    """The mask kinds a frame is planned with."""
    kinds = ("null", "ones", "zeros", "half")
    if frame in RESIDUE_FRAMES:
        kinds += ("r0",)
    if frame in R1_FRAMES:
        kinds += ("r1",)
    if frame == ONE_FRAME:
        kinds += ("one",)
    return kinds
