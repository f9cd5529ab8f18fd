"""The Gui render plane (IPT_FLAG_GUI_PLANE) restated in numpy float32, and the
frames that reach what distinguishes it from GridRenderPlane. Shared by
tests/test_gui_plane_cpu.py (the restatement itself, no GPU) and
tests/test_gpu_gui_plane.py (the same frames through the kernels). Imports
from drift_cases and changes nothing there.

Gui::addRay (gui.cpp:165-182) maps a sample at (x, y) to

    ix = min(size_t(x*W), W-1)        iy = min(size_t(H - y*H), H-1)

(its 640 and 639 generalised to W, H, W-1, H-1) where GridRenderPlane::addRay
(GridRenderPlane.cpp:66-67) has size_t(H - y*H - 1). (H - t) - 1.0f is exact
for H - t >= 1, so away from the two edge source rows the Gui row is the Grid
row + 1 and the drift code -- relative to the nominal row H-1-s of source row
s -- is the Grid code of the same sample. They differ at the edges:

  top clamp   a source-row-0 sample whose H - y*H rounds to H (y*H is 0 or
              below half an ulp of H: a jitter draw of 0 or 2^-24) gives
              iy = H, the min brings it back to row H-1, its nominal row: code
              0x5 (Grid: a 0x9 drift into row H-1);
  bottom      a source-row-(H-1) sample with H - fl(y*H) == 1 lands in row 1,
              dy = +1 (Grid: nominal, row 0).

Gui::addRay is pinned by this restatement of its source and by the Grid-row-
plus-one identity against the oracle's GridRenderPlane codes (which are pinned
to compiled reference code), not against compiled gui.cpp: the Gui's
constructor opens X11 displays.

The jitter draws are words 0 and 1 of the KAT-pinned Philox block {0, pass,
pixel, 0} (capi.philox, the library's host build; tests/test_philox_kat.py),
spot-checked against the oracle's randf in test_gui_plane_cpu.py. Radiance
values are the oracle's render_values: the same (x, y) gives the same camera
ray whatever plane receives it."""
import functools

import numpy as np

import drift_cases as dc
from ipt_amd import capi

FLAG = capi.IPT_FLAG_GUI_PLANE
F = np.float32

SQUARE = (640, 640)
# frames of the edge table (passes scanned: SCAN_PASSES below)
TABLE_FRAMES = (dc.WIDE, dc.WIDE_MAX, dc.MAX_HEIGHT, dc.TALL_ODD, dc.TALL, SQUARE)

# Edge samples (pass, source ix) at the default seed. TOP_CLAMP: source row 0,
# raw Gui row H (clamped to H-1, code 0x5, Grid code 0x9). BOTTOM: source row
# H-1, Gui row 1 (code 0x9, Grid code 0x5). Each is confirmed with the
# oracle's randf in test_gui_plane_cpu.py::test_edge_samples.
TOP_CLAMP = {
    dc.WIDE: ((7, 2420), (8, 17598)),
    dc.WIDE_MAX: ((7, 2420), (8, 17598)),
    dc.MAX_HEIGHT: ((127, 1), (143, 1)),
    dc.TALL_ODD: ((127, 1), (143, 1)),
    dc.TALL: ((127, 1), (143, 1)),
    SQUARE: ((25, 210),),
}
BOTTOM = {
    dc.WIDE: (), dc.WIDE_MAX: (), dc.TALL: (),
    dc.MAX_HEIGHT: ((97, 0), (136, 1), (143, 1)),
    dc.TALL_ODD: ((195, 0),),
    SQUARE: ((56, 367),),
}

# renders of the GPU suite that hold edge samples: (W, H, spp, spp_offset)
EDGE_RENDERS = ((60000, 3, 9, 0), (2, 65536, 9, 136), (640, 640, 1, 25), (640, 640, 1, 56))

# {(W, H, spp, spp_offset): {code: samples}} under the Gui map. Passes 0..1 of
# the five drift frames equal drift_cases.HIST (no edge sample there); 60000x3
# at nine passes has lost the Grid map's two 0x9 (top clamps of passes 7, 8).
HIST = {
    (60000, 3, 2, 0): {0x4: 6, 0x6: 461},
    (3, 60000, 2, 0): {0x1: 3, 0x9: 737},
    (65536, 2, 2, 0): {0x6: 344},
    (2, 65536, 2, 0): {0x9: 594},
    (4099, 61, 2, 0): {0x6: 38, 0x9: 2},
    (60000, 3, 9, 0): {0x4: 20, 0x6: 2025},
    # passes 136..144 of the tallest frame: two of the 0x9 are BOTTOM samples
    # (source row H-1 into row 1), and pass 143's top clamp is a 0x5
    (2, 65536, 9, 136): {0x9: 2690},
    (640, 640, 1, 25): {0x6: 6, 0x9: 11},   # holds a top clamp (0x5)
    (640, 640, 1, 56): {0x6: 3, 0x9: 12},   # one 0x9 is the BOTTOM sample
}
# passes scanned for the edge table, by frame
SCAN_PASSES = {dc.WIDE: 16, dc.WIDE_MAX: 16, dc.MAX_HEIGHT: 256, dc.TALL_ODD: 256, dc.TALL: 256, SQUARE: 64}

# A top-clamp sample has y <= 2^-24, the lower edge of the view, and no ray
# there carries radiance in the box scene, whatever its column, seed or tree
# (nor in the floor, corner, fractal and sphere-list scenes: the edge looks
# past the geometry; 640 columns x 8 passes at y < 2^-16, trees 4/3 and 16/8,
# are all zero). Every ray of smallpt's closed room does, so the top clamp's
# non-zero-valued sample is the default seed's pass 7, pixel 2420 (a y draw of
# 2^-24: a top clamp at any height), rendered in that scene on the smallest
# frame that holds it: (scene, W, H, spp, offset).
TOP_CLAMP_NONZERO = ("smallpt", 2421, 3, 1, 7)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def draws(W, H, spp, spp_offset=0, seed=dc.DEFAULT_SEED):
    """The two jitter draws of every sample, [spp][H][W] float32 each."""
    ctr = np.zeros((spp, H * W, 4), np.uint32)
    ctr[:, :, 1] = (spp_offset + np.arange(spp, dtype=np.uint32))[:, None]
    ctr[:, :, 2] = np.arange(H * W, dtype=np.uint32)[None, :]
    w = capi.philox(ctr.reshape(-1, 4), (seed & 0xffffffff, seed >> 32))
    u = (w[:, :2] >> 8).astype(F) * F(2.0 ** -24)
    return _frozen(u[:, 0].reshape(spp, H, W).copy(), u[:, 1].reshape(spp, H, W).copy())


def coords(W, H, spp, spp_offset=0, seed=dc.DEFAULT_SEED):
    """render_sample's jittered (x, y) (main.cpp:192-198), float32."""
    u0, u1 = draws(W, H, spp, spp_offset, seed)
    ix = np.arange(W, dtype=F)[None, None, :]
    iy = np.arange(H, dtype=F)[None, :, None]
    x = (ix + u0) / F(W)
    y = (iy + u1) / F(H)
    below_one = np.nextafter(F(1.0), F(0.0))
    return np.where(x == F(1.0), below_one, x).astype(F), np.where(y == F(1.0), below_one, y).astype(F)


def gui_raw_index(x, y, W, H):
    """size_t(x*W), size_t(H - y*H) before the min (gui.cpp:168-169)."""
    fx = x * F(W)
    fy = F(H) - y * F(H)
    assert fx.dtype == F and fy.dtype == F and (fx >= 0).all() and (fy >= 0).all()
    return fx.astype(np.int64), fy.astype(np.int64)


def grid_index(x, y, W, H):
    """GridRenderPlane.cpp:66-67 (negative -> 0, as the oracle states it)."""
    fx = x * F(W)
    fy = (F(H) - y * F(H)) - F(1.0)
    return np.where(fx < 0, 0, fx.astype(np.int64)), np.where(fy < 0, 0, fy.astype(np.int64))


@functools.lru_cache(maxsize=None)
def raw_rows(W, H, spp, spp_offset=0, seed=dc.DEFAULT_SEED):
    """(clamped column, unclamped row) of every sample under the Gui map."""
    x, y = coords(W, H, spp, spp_offset, seed)
    xi, yr = gui_raw_index(x, y, W, H)
    return _frozen(np.minimum(xi, W - 1), yr)


def nominal_rows(H):
    return (H - 1 - np.arange(H, dtype=np.int64))[None, :, None]


def encode(xi, yi, yn, W, H):
    """Drift codes of destinations (xi, yi) relative to (ix, yn)."""
    dx = xi - np.arange(W, dtype=np.int64)[None, None, :]
    dy = yi - yn
    ok = (np.abs(dx) <= 1) & (np.abs(dy) <= 1) & (xi < W) & (yi < H)
    return np.where(ok, (dx + 1) | ((dy + 1) << 2), 0xff).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def codes(W, H, spp, spp_offset=0, seed=dc.DEFAULT_SEED):
    """ipt_render_values' codes with IPT_FLAG_GUI_PLANE; read-only."""
    xi, yr = raw_rows(W, H, spp, spp_offset, seed)
    return _frozen(encode(xi, np.minimum(yr, H - 1), nominal_rows(H), W, H))[0]


@functools.lru_cache(maxsize=None)
def grid_codes(W, H, spp, spp_offset=0, seed=dc.DEFAULT_SEED):
    """The GridRenderPlane codes by the same restatement of the stream (for
    checking the restatement against the oracle's)."""
    x, y = coords(W, H, spp, spp_offset, seed)
    xi, yi = grid_index(x, y, W, H)
    yn = np.maximum(H - 2 - np.arange(H, dtype=np.int64), 0)[None, :, None]
    return _frozen(encode(xi, yi, yn, W, H))[0]


def destinations(c):
    """(nominal row, destination row, destination column) of Gui codes."""
    _, H, W = c.shape
    yn = np.broadcast_to(nominal_rows(H), c.shape)
    ix = np.arange(W, dtype=np.int64)[None, None, :]
    c = c.astype(np.int64)
    return yn, yn + ((c >> 2) & 3) - 1, ix + (c & 3) - 1


def replay_events(values, yi, xi, img=None, extra_row0_from=None):
    """The plane after Gui::addRay of every sample, passes in order and each
    pass in render_sample's raster order, into `img` (zeros if None; the
    running mean is GridRenderPlane::addRay's, so drift_cases._add_rays serves;
    sums and pixel_max as the library keeps them). Samples with a row outside
    [0, H) are dropped. extra_row0_from: a WRONG replay that also adds that
    source row's samples to row 0 (before the later rows' samples)."""
    spp, H, W = values.shape
    img = dc.plane(W, H) if img is None else img
    for s in range(spp):
        ys, xs, v = yi[s].reshape(-1), xi[s].reshape(-1), values[s].reshape(-1)
        if extra_row0_from is not None:
            r = extra_row0_from
            cut = (r + 1) * W
            ys = np.r_[ys[:cut], np.zeros(W, np.int64), ys[cut:]]
            xs = np.r_[xs[:cut], xi[s, r], xs[cut:]]
            v = np.r_[v[:cut], values[s, r], v[cut:]]
        keep = (ys >= 0) & (ys < H)
        dc._add_rays(img, (ys * W + xs)[keep], v[keep])
    return img


def replay(values, c, img=None):
    _, yi, xi = destinations(c)
    assert (c < 0x10).all()
    return replay_events(values, yi, xi, img)


@functools.lru_cache(maxsize=None)
def gui_plane(W, H, spp, spp_offset=0, n_rays=dc.N_RAYS, depth_max=dc.DEPTH_MAX, seed=dc.DEFAULT_SEED):
    """The Gui plane of the box scene from zeros: the oracle's values, the
    restated codes; read-only."""
    v, _, _ = dc.oracle_samples(W, H, spp, spp_offset, n_rays, depth_max, seed)
    ref = replay(v, codes(W, H, spp, spp_offset, seed))
    _frozen(*ref.values())
    return ref


def wrong_replay(values, W, H, spp, spp_offset=0, how="no_clamp", seed=dc.DEFAULT_SEED):
    """"no_clamp": the min() forgotten -- a sample of raw row H falls off the
    image; "grid_row0": the Gui map with GridRenderPlane's doubled row 0 kept
    (row 0 also fed by source row H-2, as the Grid replay's fast path reads
    it)."""
    xi, yr = raw_rows(W, H, spp, spp_offset, seed)
    if how == "no_clamp":
        return replay_events(values, yr, xi)  # (row H: dropped)
    if how == "grid_row0":
        if H < 2:
            raise ValueError("needs two rows")
        return replay_events(values, np.minimum(yr, H - 1), xi, extra_row0_from=H - 2)
    raise ValueError(how)


def edge_scan(W, H, passes, seed=dc.DEFAULT_SEED):
    """[(pass, ix)] of the top-clamp samples and of the bottom samples in
    passes 0..passes-1: only source rows 0 and H-1 are drawn."""
    out = []
    for row, want in ((0, H), (H - 1, 1)):
        ctr = np.zeros((passes, W, 4), np.uint32)
        ctr[:, :, 1] = np.arange(passes, dtype=np.uint32)[:, None]
        ctr[:, :, 2] = (row * W + np.arange(W, dtype=np.uint32))[None, :]
        w = capi.philox(ctr.reshape(-1, 4), (seed & 0xffffffff, seed >> 32))
        u1 = ((w[:, 1] >> 8).astype(F) * F(2.0 ** -24)).reshape(passes, W)
        y = (F(row) + u1) / F(H)
        y = np.where(y == F(1.0), np.nextafter(F(1.0), F(0.0)), y).astype(F)
        yr = (F(H) - y * F(H)).astype(np.int64)
        out.append(tuple((int(s), int(x)) for s, x in np.argwhere(yr == want)))
    return out


def edge_masks(W, H, spp, spp_offset=0, seed=dc.DEFAULT_SEED):
    """(top clamp, bottom) sample masks [spp][H][W]."""
    _, yr = raw_rows(W, H, spp, spp_offset, seed)
    top = yr == H
    bottom = np.zeros_like(top)
    if H >= 2:
        bottom[:, H - 1] = yr[:, H - 1] == 1
    return top, bottom
