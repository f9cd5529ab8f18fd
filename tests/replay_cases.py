"""Samples for the render-plane replay probe (ipt_replay_samples), chosen
instead of rendered. Pure numpy and deterministic; shared by
tests/test_replay_cpu.py (the conditions that make each case discriminating,
no GPU) and tests/test_gpu_replay.py (the same cases through
accumulate_kernel).

A render drifts 5.6e-5 of its samples and never produces the codes 0x0 and
0x2, so the replay's flagged-pixel branch sees one drifted sample at a time
there. Here most samples drift, every code appears, several sources hit one
destination in one pass, at every edge of the frame. Values are spread over
six decades, so that a running mean taken in another order has other bits.

Every generator takes the plane: GRID (GridRenderPlane::addRay's row map,
nominal row max(H-2-iy, 0)) or GUI (Gui::addRay's, H-1-iy), and asserts that
every destination lies inside the frame: ipt_oracle_accumulate does not check
bounds, and ipt_replay_samples refuses such a code."""
import numpy as np

import drift_cases as dc
import gui_cases as gc

GRID, GUI = "grid", "gui"
PLANES = (GRID, GUI)
F = np.float32

# (dx + 1) | (dy + 1) << 2 for every (dx, dy) but (0, 0)
DRIFT_CODES = (0x0, 0x1, 0x2, 0x4, 0x6, 0x8, 0x9, 0xa)
DIAG_DOWN = (0x0, 0x2)  # dy = -1 with dx = -1, +1: no render in the suite produces them

# frames of the dense cases, (W, H). 257 and 513 columns: rows wider than one
# and two 256-thread blocks, where a pixel scans its neighbouring block's
# columns. Below 5x4 a frame cannot hold all eight codes with room for the
# orders to show: which replays of WRONG coincide with the right one there is
# pinned case by case in test_replay_cpu.py; those frames test parity first.
DENSE_FRAMES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (5, 4), (37, 23), (257, 5), (513, 3))
# (one pass: a launch with flagged and unflagged pixels side by side; from
# eight passes on nearly every pixel of a dense case is flagged by some pass)
DENSE_SPPS = (1, 8, 9, 17)
SINGLE_FRAME, SINGLE_SPP = (9, 8), 9
CONVERGE_FRAMES, CONVERGE_SPP = ((9, 9), (10, 7)), 9
PRELOAD_FRAME, PRELOAD_SPPS = dc.SMALL, (7, 9, 17)
SHARD_FRAME, SHARD_SPP = (9, 40), 9
SHARD_PLANS = ((1, 2), (1, 3), (4, 3), (16, 2))  # (tile_rows, n_shards)
CHUNK_FRAME, CHUNK_SPP = (37, 23), 9
MAX_PER_PASS = 12  # samples one pixel can receive in one pass (Grid row 1: four source rows, three columns)

WRONG = ("cols_first", "rows_descending", "diag_late", "drift_last", "nominal_only")


def flag(plane):
    return gc.FLAG if plane == GUI else 0


def nominal_rows(H, plane):
    iy = np.arange(H, dtype=np.int64)
    return H - 1 - iy if plane == GUI else np.maximum(H - 2 - iy, 0)


def encode(dx, dy):
    return ((dx + 1) | ((dy + 1) << 2)).astype(np.uint8)


def destinations(codes, plane):
    """(nominal row, destination row, destination column) of codes [spp][H][W]."""
    return gc.destinations(codes) if plane == GUI else dc.destinations(codes)


def assert_in_frame(codes, plane):
    _, H, W = codes.shape
    c = codes.astype(np.int64)
    assert (codes < 0x10).all() and ((c & 3) != 3).all() and ((c >> 2) != 3).all()
    _, yi, xi = destinations(codes, plane)
    assert (xi >= 0).all() and (xi < W).all() and (yi >= 0).all() and (yi < H).all()


def _values(rng, shape):
    """A random float32 in [0, 1) times 10^k, k in -3..2."""
    scale = np.array([1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2], F)[rng.integers(0, 6, shape)]
    return (rng.random(shape, dtype=F) * scale).astype(F)


def _clip(dx, dy, W, H, plane):
    """dx, dy reset to 0, each on its own, where the destination would leave
    the frame."""
    yn = nominal_rows(H, plane)[None, :, None]
    ix = np.arange(W, dtype=np.int64)[None, None, :]
    dx = np.where((ix + dx < 0) | (ix + dx >= W), 0, dx)
    dy = np.where((yn + dy < 0) | (yn + dy >= H), 0, dy)
    return dx, dy


def _done(values, codes, plane):
    assert_in_frame(codes, plane)
    values.setflags(write=False)
    codes.setflags(write=False)
    return values, codes


def dense(W, H, spp, seed, plane, p_drift=0.7):
    """A share p_drift of the samples drifts, uniformly over the eight
    directions (less what the frame's edges take back)."""
    rng = np.random.default_rng([seed, W, H, spp, PLANES.index(plane)])
    shape = (spp, H, W)
    pick = rng.integers(0, 8, shape)
    d = np.array([((c & 3) - 1, (c >> 2) - 1) for c in DRIFT_CODES], np.int64)
    drift = rng.random(shape) < p_drift
    dx, dy = _clip(np.where(drift, d[pick, 0], 0), np.where(drift, d[pick, 1], 0), W, H, plane)
    return _done(_values(rng, shape), encode(dx, dy), plane)


# 5x4 is the smallest frame on which all eight codes fit and every wrong
# replay shows; with 20 samples a pass that takes a seed chosen for it: the
# first (from 0) under which the case holds every code and differs from each
# replay of WRONG (test_replay_cpu.py asserts both). Every other case: seed 0.
DENSE_SEEDS = {(5, 4, 1, GRID): 56, (5, 4, 1, GUI): 20, (5, 4, 17, GUI): 1}


def dense_case(W, H, spp, plane):
    return dense(W, H, spp, DENSE_SEEDS.get((W, H, spp, plane), 0), plane)


def single_code(code, W, H, spp, plane):
    """Every sample whose destination stays in the frame carries `code`, the
    rest 0x05."""
    assert code in DRIFT_CODES
    rng = np.random.default_rng([code, W, H, spp])
    shape = (spp, H, W)
    dx, dy = np.full(shape, (code & 3) - 1, np.int64), np.full(shape, (code >> 2) - 1, np.int64)
    cx, cy = _clip(dx, dy, W, H, plane)
    codes = np.where((cx == dx) & (cy == dy), code, 0x05).astype(np.uint8)
    return _done(_values(rng, shape), codes, plane)


def converge_centres(W, H):
    """The centres: columns 1, 4, 7, ...; the rows of column group g = x // 3
    are those congruent to g mod 3, so that rows 0, 1 and 2 each head a
    column group (a stride-3 lattice, sheared by one row per group)."""
    return [(cx, cy) for cx in range(1, W, 3) for cy in range((cx // 3) % 3, H, 3)]


def converge(W, H, spp, plane):
    """Every source whose nominal pixel lies in a centre's 3x3 neighbourhood
    targets that centre (0x05 where the centre is outside the frame), so a
    centre away from the edges receives nine samples per pass and, under the
    Grid map, row 1 twelve: its row 0 neighbours are fed by source rows H-2
    and H-1 both. Asserted on the reference's counters after one pass."""
    assert W >= 3 and H >= 5
    rng = np.random.default_rng([W, H, spp, PLANES.index(plane)])
    yn = nominal_rows(H, plane)[:, None]
    ix = np.arange(W, dtype=np.int64)[None, :]
    ph = (ix // 3) % 3
    cx = 3 * (ix // 3) + 1
    cy = 3 * ((yn - ph + 1) // 3) + ph
    ok = (cx < W) & (cy >= 0) & (cy < H)
    code = np.where(ok, encode(np.where(ok, cx - ix, 0), np.where(ok, cy - yn, 0)), 0x05).astype(np.uint8)
    codes = np.ascontiguousarray(np.broadcast_to(code[None], (spp, H, W)))
    values = _values(rng, (spp, H, W))
    assert_in_frame(codes, plane)
    cnt = replay(values[:1], codes[:1], plane)["counters"].reshape(H, W)
    _, yi, xi = destinations(codes[:1], plane)
    src = np.broadcast_to(np.arange(H)[None, :, None], yi.shape)
    seen = {9: 0, 12: 0}
    for x, y in converge_centres(W, H):
        if not 1 <= x <= W - 2:
            continue
        rows = sorted(set(src[(yi == y) & (xi == x)].tolist()))
        if plane == GUI:
            if 1 <= y <= H - 2:
                assert cnt[y, x] == 9 and rows == [H - 2 - y, H - 1 - y, H - y]
                seen[9] += 1
        elif y == 0:
            assert cnt[y, x] == 9 and rows == [H - 3, H - 2, H - 1]
            seen[9] += 1
        elif y == 1:
            assert cnt[y, x] == 12 and rows == [H - 4, H - 3, H - 2, H - 1]
            seen[12] += 1
        elif y <= H - 3:
            assert cnt[y, x] == 9 and rows == [H - 3 - y, H - 2 - y, H - 1 - y]
            seen[9] += 1
    assert seen[9] >= 2 and (plane == GUI or seen[12] >= 1)
    return _done(values, codes, plane)


def hot_pixels(codes, plane):
    """Destination pixels of the drifted samples."""
    _, H, W = codes.shape
    _, yi, xi = destinations(codes, plane)
    d = codes != 0x05
    return yi[d] * W + xi[d]


def preloaded(W, H, spp, seed=7):
    """(plane, kind index per pixel and array): drift_cases.preload's kinds of
    counters, pixels, sums and pixel_max, a seeded mix over the frame (under
    dense codes nearly every pixel is a drifted sample's destination:
    test_replay_cpu.py checks that each kind sits on some), the top counter
    leaving room for MAX_PER_PASS samples per pass below the uint32 wrap; the
    +inf pixel / counter 0 pairing stays out (drift_cases.preload says why)."""
    return dc.preload(W, H, spp, None, seed, per_pass=MAX_PER_PASS)


def cross_shard(codes, plane, tile_rows, n_shards):
    """Drifted samples whose nominal and destination rows have different owners."""
    yn, yi, _ = destinations(codes, plane)
    d = codes != 0x05
    return int((dc.shard_of(yn[d], tile_rows, n_shards) != dc.shard_of(yi[d], tile_rows, n_shards)).sum())


# ---- the replay restated, and wrong ones ---------------------------------------
def replay(values, codes, plane, how="raster", img=None):
    """The plane after the samples (into `img`, zeros if None).
    "raster":          passes, source rows, source columns: render_sample's
                       order (drift_cases.replay's / gui_cases.replay's);
    "cols_first":      wrong: within a pass by source column, then source row;
    "rows_descending": wrong: a pass's source rows from H-1 down;
    "diag_late":       wrong: the 0x0 and 0x2 samples at the end of their pass;
    "drift_last":      wrong: a pass's drifted samples after its nominal ones;
    "nominal_only":    wrong: drifted samples dropped."""
    spp, H, W = values.shape
    img = dc.plane(W, H) if img is None else img
    _, yi, xi = destinations(codes, plane)
    dest = (yi * W + xi).reshape(spp, -1)
    vals = values.reshape(spp, -1)
    flat = codes.reshape(spp, -1)
    raster = np.arange(H * W).reshape(H, W)
    for s in range(spp):
        if how == "raster":
            k = raster.reshape(-1)
        elif how == "cols_first":
            k = raster.T.reshape(-1)
        elif how == "rows_descending":
            k = raster[::-1].reshape(-1)
        elif how == "diag_late":
            late = np.isin(flat[s], DIAG_DOWN)
            k = np.r_[np.flatnonzero(~late), np.flatnonzero(late)]
        elif how == "drift_last":
            late = flat[s] != 0x05
            k = np.r_[np.flatnonzero(~late), np.flatnonzero(late)]
        elif how == "nominal_only":
            k = np.flatnonzero(flat[s] == 0x05)
        else:
            raise ValueError(how)
        dc._add_rays(img, dest[s][k], vals[s][k])
    return img


def gui_as_grid(values, codes):
    """A Gui case on W x H as a Grid case on W x (H+1): GridRenderPlane's
    nominal row of source row s in a frame of H+1 rows is H-1-s, the Gui's in
    a frame of H rows, for every s < H; the added source row H folds into row
    0 (code 0x05, values of its own). Pixels are independent of each other, so
    rows 1..H-1 of the Grid plane are the Gui plane's, and row H stays empty;
    row 0 alone differs, by the fold."""
    spp, H, W = values.shape
    rng = np.random.default_rng([spp, H, W])
    v = np.concatenate([values, _values(rng, (spp, 1, W))], axis=1)
    c = np.concatenate([codes, np.full((spp, 1, W), 0x05, np.uint8)], axis=1)
    assert_in_frame(c, GRID)
    return v, c
