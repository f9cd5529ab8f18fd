"""Adaptive sampling restated in numpy float32: the masked raster replay with
its second-moment plane, ipt_adapt_device's rule and the round loop, for both
row maps, with the wrong variants the CPU tests must tell apart. Shared by
tests/test_adaptive_cpu.py (the conditions alone, oracle only) and
tests/test_gpu_adaptive.py (the same cases through the kernels). Imports from
drift_cases and gui_cases and changes nothing there.

A sample's value depends only on (seed, pass, source pixel), so the oracle's
samples with the inactive ones left out, replayed in raster order, are the
expected plane. The mask is indexed by a sample's NOMINAL destination pixel
(ix, yn): yn = max(H-2-iy, 0) under the Grid map (mask row 0 governs source
rows H-2 and H-1 alike, and row H-1, for H >= 2, governs nothing), H-1-iy
under the Gui's. A traced sample that drifts is added where it lands, whatever
the mask says there."""
import numpy as np

import drift_cases as dc
import gui_cases as gc

F = np.float32
GRID, GUI = "grid", "gui"
PLANES = (GRID, GUI)
FLAG = {GRID: 0, GUI: gc.FLAG}

# the seeded half mask's frames (W, H, spp) and, under the Grid map, per frame:
# masked sources with a non-zero value; active drifted samples landing in a
# masked pixel (of them non-zero); dropped drifted samples whose landing pixel
# is active (non-zero); active drifts into active pixels
HALF_FRAMES = ((60000, 3, 9), (3, 60000, 2), (4099, 61, 2))
HALF_COUNTS = {
    (60000, 3, 9): (342201, (511, 225), (554, 223), 514),
    (3, 60000, 2): (76139, (188, 91), (194, 81), 180),
    (4099, 61, 2): (106164, (10, 3), (8, 4), 9),
}

# the loop case: frames, passes, round, ipt_adapt_params
LOOP_FRAMES = ((37, 23), (13, 11))
LOOP_SPP, LOOP_ROUND = 40, 4
LOOP_ADAPT = dict(min_count=8, rel_tol=0.25, abs_tol=1e-3)


def half_mask(W, H):
    """The seeded half mask [H][W], uint8 (1 = active)."""
    return (np.random.default_rng([W, H, 1]).random(W * H) < 0.5).astype(np.uint8).reshape(H, W)


def nominal_rows(H, plane):
    iy = np.arange(H, dtype=np.int64)
    return np.maximum(H - 2 - iy, 0) if plane == GRID else H - 1 - iy


def codes_of(W, H, spp, plane, spp_offset=0):
    """The drift codes of the box scene's samples under the plane's map."""
    if plane == GRID:
        return dc.oracle_samples(W, H, spp, spp_offset)[1]
    return gc.codes(W, H, spp, spp_offset)


def destinations(codes, plane):
    """(nominal row, destination row, destination column), [spp][H][W]."""
    _, H, W = codes.shape
    yn = np.broadcast_to(nominal_rows(H, plane)[None, :, None], codes.shape)
    ix = np.arange(W, dtype=np.int64)[None, None, :]
    c = codes.astype(np.int64)
    return yn, yn + ((c >> 2) & 3) - 1, ix + (c & 3) - 1


def active_samples(codes, mask, plane, how="nominal"):
    """[spp][H][W] bool: the samples a masked render traces. mask None = all.
    how "source" and "landing" are the wrong indexings."""
    spp, H, W = codes.shape
    ok = codes < 0x10
    if mask is None:
        return ok
    m = np.asarray(mask).reshape(H, W) != 0
    yn, yi, xi = destinations(codes, plane)
    ix = np.broadcast_to(np.arange(W, dtype=np.int64)[None, None, :], codes.shape)
    if how == "nominal":
        return ok & m[yn, ix]
    if how == "source":
        iy = np.broadcast_to(np.arange(H, dtype=np.int64)[None, :, None], codes.shape)
        return ok & m[iy, ix]
    if how == "landing":
        return ok & m[np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)]
    raise ValueError(how)


def _add_rays_m2(img, m2, dest, vals, sumsq=False):
    """dc._add_rays with Welford's second moment: per added sample, in f32,
    m2 += (v - p_old) * (v - p_new). sumsq: the wrong m2 += v * v."""
    if dest.size == 0:
        return
    order = np.argsort(dest, kind="stable")
    ds, vs = dest[order], vals[order]
    first = np.r_[0, np.flatnonzero(ds[1:] != ds[:-1]) + 1]
    rank = np.arange(ds.size) - np.repeat(first, np.diff(np.r_[first, ds.size]))
    with np.errstate(all="ignore"):
        for r in range(int(rank.max()) + 1):
            k = rank == r
            d, v = ds[k], vs[k]
            c = img["counters"][d].astype(np.uint64)
            p_old = img["pixels"][d]
            p = (p_old * c.astype(F) + v) / (c + 1).astype(F)
            img["pixels"][d] = p
            img["counters"][d] = (c + 1).astype(np.uint32)
            img["sums"][d] += v
            img["pixel_max"][d] = np.where(p > img["pixel_max"][d], p, img["pixel_max"][d])
            if m2 is not None:
                m2[d] += (v * v) if sumsq else ((v - p_old).astype(F) * (v - p).astype(F)).astype(F)


def replay(values, codes, mask, plane, img=None, m2=None, how="nominal"):
    """(plane, m2) after the masked samples, passes in order and each pass in
    render_sample's raster order, into img / m2 (zeros if None; both are
    changed in place and returned).
    how: "nominal" is right; "source", "landing": the mask indexed wrongly;
    "zeros": masked samples replayed as zeros; "sumsq": m2 a sum of squares."""
    spp, H, W = values.shape
    img = dc.plane(W, H) if img is None else img
    m2 = np.zeros(W * H, F) if m2 is None else m2
    index = how if how in ("source", "landing") else "nominal"
    act = active_samples(codes, mask, plane, index)
    _, yi, xi = destinations(codes, plane)
    dest = (yi * W + xi).reshape(spp, -1)
    for s in range(spp):
        a = act[s].reshape(-1)
        v = values[s].reshape(-1)
        if how == "zeros":
            ok = (codes[s] < 0x10).reshape(-1)
            _add_rays_m2(img, m2, dest[s][ok], np.where(a, v, F(0))[ok].astype(F))
        else:
            _add_rays_m2(img, m2, dest[s][a], v[a], sumsq=how == "sumsq")
    return img, m2


def counts(codes, mask, plane):
    """(active sources, active drifted): ipt_counters' paths and drifted."""
    act = active_samples(codes, mask, plane)
    return int(act.sum()), int((act & (codes != 0x05)).sum())


def adapt(pixels, counters, m2, W, H, min_count, rel_tol, abs_tol, gui=False):
    """ipt_adapt_device: (mask uint8 [H*W], stats uint32 [4] = {active,
    starved, nan, 0}), in f32, operation for operation."""
    with np.errstate(all="ignore"):
        c = counters.astype(np.uint32)
        starved = c < np.uint32(min_count)
        nf = c.astype(F)
        e2 = (m2.astype(F) / (nf * (nf - F(1.0))).astype(F)).astype(F)
        thr = (F(rel_tol) * np.abs(pixels.astype(F)) + F(abs_tol)).astype(F)
        t2 = (thr * thr).astype(F)
        nan = ~starved & (np.isnan(e2) | np.isnan(t2))
        active = starved | (~starved & (e2 > t2))
    if not gui and H >= 2:  # the Grid map's row H-1 has no nominal source
        live = np.arange(W * H) < (H - 1) * W
        active, starved, nan = active & live, starved & live, nan & live
    stats = np.array([active.sum(), starved.sum(), nan.sum(), 0], np.uint32)
    return active.astype(np.uint8), stats


def loop(values, codes, plane, round_spp, min_count, rel_tol, abs_tol):
    """The round loop from zeros over values' passes: round 0 unmasked, each
    round followed by adapt, stopping when nothing is active. Returns the
    rounds [(plane copy, m2 copy, mask, stats)] and the passes used."""
    spp, H, W = values.shape
    img, m2, mask = dc.plane(W, H), np.zeros(W * H, F), None
    rounds, done = [], 0
    while done < spp:
        n = min(round_spp, spp - done)
        replay(values[done:done + n], codes[done:done + n], mask, plane, img, m2)
        mask, stats = adapt(img["pixels"], img["counters"], m2, W, H, min_count, rel_tol, abs_tol, plane == GUI)
        rounds.append((dc.copy_plane(img), m2.copy(), mask, stats))
        done += n
        if stats[0] == 0:
            break
    return rounds, done
