"""The denoiser restated in numpy float32: ipt_guides_device's scatter (the
preview restatement's kinds and hits, rearranged) and ipt_denoise_device's
filter, operation for operation as include/ipt_capi.h states it, with the
wrong variants the CPU tests must tell apart, an operand census of its
divisions and root, and the planes that leave their in-range windows. Shared by
tests/test_denoise_cpu.py (the restatement alone) and the GPU tests (the same
cases through the kernels). Imports from the other case modules and changes
nothing there."""
import functools

import numpy as np

from ipt_amd import capi, scenes

import adaptive_cases as ac
import drift_cases as dc
import gui_cases as gc

F = np.float32
GRID, GUI = ac.GRID, ac.GUI
DEFAULTS = capi.DENOISE_DEFAULTS
WRONG = ("unsquared_var", "linear_step", "all_taps", "dx_outer", "prefilter_at_s")
WRONG_EDGES = ("daz", "signed_counter")  # (and ("seam", axis, S), below)
HK = (F(0.375), F(0.25), F(0.0625))
EPS = F(2.0 ** -20)
TILE = {"x": 32, "y": 8}  # the tiled form's workgroup, in pixels of one residue's sub-lattice

# The operand census: the filter's five divisions and its root, and per operation
# [evaluations that count, with an operand outside the window in which the
# range-free division / root of ipt_math.h is exact, with a denormal operand
# or result]. A zero dividend is inside the window.
OPS = ("var0", "e/sigma_z", "dc/den", "sc/sw", "sv/sw2", "sqrt")
DIV_WINDOW = (F(2.0 ** -40), F(2.0 ** 41))
SQRT_WINDOW = (F(2.0 ** -96), F(2.0 ** 126))
TINY = np.finfo(F).tiny


def _denormal(a):
    m = np.abs(a)
    return (m > 0) & (m < TINY)


def _daz(a):
    return np.where(_denormal(a), np.copysign(F(0.0), a), a).astype(F)


denormal, daz = _denormal, _daz  # (tests/reproject_cases.py's census and its "daz" variant use them too)


def _inside(a, window):
    m = np.abs(a)
    return (m >= window[0]) & (m < window[1])


def _tally(census, op, counted, outside, denormal):
    c = census.setdefault(op, [0, 0, 0])
    for k, m in enumerate((counted, counted & outside, counted & denormal)):
        c[k] += int(np.count_nonzero(m))


def _div(a, b, op, counted, census=None, daz=False):
    """(a / b) in float32; the census of op over the evaluations `counted`."""
    a, b = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
    if daz:
        a, b = _daz(a), _daz(b)
    q = (a / b).astype(F)
    if census is not None:
        _tally(census, op, counted, ((a != 0) & ~_inside(a, DIV_WINDOW)) | ~_inside(b, DIV_WINDOW),
               _denormal(a) | _denormal(b) | _denormal(q))
    return _daz(q) if daz else q


def _sqrt(a, op, counted, census=None, daz=False):
    a = _daz(a) if daz else np.asarray(a, F)
    r = np.sqrt(a).astype(F)
    if census is not None:
        _tally(census, op, counted, (a != 0) & ~((a >= SQRT_WINDOW[0]) & (a < SQRT_WINDOW[1])),
               _denormal(a) | _denormal(r))
    return _daz(r) if daz else r


# ---------------------------------------------------------------- guides
def guide_rows(H, plane):
    """Source row of each destination row, -1 for none."""
    yd = np.arange(H, dtype=np.int64)
    if plane == GUI:
        return H - 1 - yd
    if H == 1:
        return np.zeros(1, np.int64)
    return np.where(yd <= H - 2, H - 2 - yd, -1)


def scatter_guides(kinds, hits, plane):
    """ipt_guides_device from one pass of ipt_preview_values' kinds [H][W] and
    hits [H][W][6]: GuideRecord [H][W] in destination order."""
    H, W = kinds.shape
    g = np.zeros((H, W), capi.GuideRecord)
    g["kind"] = 0xff
    src = guide_rows(H, plane)
    ok = src >= 0
    g["kind"][ok] = kinds[src[ok]]
    g["pos"][ok] = hits[src[ok]][..., 0:3]
    g["normal"][ok] = hits[src[ok]][..., 3:6]
    return g


def scene_guides(desc, W, H, plane, spp_offset=0, seed=20241223):
    """The guide plane of a scene from the preview restatement."""
    import preview_ref
    p = capi.make_params(W, H, 1, spp_offset=spp_offset, seed=seed, flags=ac.FLAG[plane])
    _, _, kinds, hits, _ = preview_ref.render(desc, p)
    return scatter_guides(kinds[0], hits[0], plane)


# ---------------------------------------------------------------- the filter
def _counts(counters, wrong=None):
    return counters.view(np.int32) if wrong == "signed_counter" else counters


def var0_of(counters, m2, census=None, wrong=None):
    """m2 / (nf * (nf - 1)) where c >= 2, else 0."""
    cn = _counts(np.asarray(counters, np.uint32), wrong)
    with np.errstate(all="ignore"):
        nf = cn.astype(F)
        v = _div(m2, (nf * (nf - F(1.0))).astype(F), "var0", cn >= 2, census, wrong == "daz")
    return np.where(cn >= 2, v, F(0.0)).astype(F)


def participation(pixels, counters, m2, guides, wrong=None):
    v0 = var0_of(counters, m2, wrong=wrong)
    c_ok = _counts(np.asarray(counters, np.uint32), wrong) >= 2
    return ((guides["kind"] & 3) == 1) & c_ok & np.isfinite(pixels) & np.isfinite(v0)


def _pos(a):
    return np.where(a > 0, a, F(0.0)).astype(F)


def denoise(pixels, counters, m2, guides, W, H, iterations=DEFAULTS["iterations"], sigma_l=DEFAULTS["sigma_l"],
            normal_pow=DEFAULTS["normal_pow"], sigma_z=DEFAULTS["sigma_z"], wrong=None, census=None, trace=None,
            resume=None):
    """(out, var_out) float32 [H*W] of ipt_denoise_device. wrong: one of WRONG
    or WRONG_EDGES, or ("seam", axis, S): at step S every 5 x 5 tap whose
    lattice tile along the axis ((x // S) // 32, (y // S) // 8) is not the
    centre's is dropped, as a wrong halo of the tiled form would.
    census: a dict that takes the operand census (OPS); it changes no result.
    trace: a list that takes (col, var) after every iteration; resume: (k, col,
    var) of such a trace, to go on from iteration k (a variant that applies
    from a late step on need not repeat the steps before it)."""
    seam = wrong if isinstance(wrong, tuple) else None
    assert wrong is None or wrong in WRONG or wrong in WRONG_EDGES or (
        len(seam) == 3 and seam[0] == "seam" and seam[1] in TILE)
    daz = wrong == "daz"
    px = np.asarray(pixels, F).reshape(H, W)
    cn = np.asarray(counters, np.uint32).reshape(H, W)
    mm = np.asarray(m2, F).reshape(H, W)
    g = np.asarray(guides).reshape(H, W)
    v0 = var0_of(cn, mm, census, wrong)
    part = participation(px, cn, mm, g, wrong)
    tap_ok = np.ones_like(part) if wrong == "all_taps" else part
    P = [g["pos"][..., k].astype(F) for k in range(3)]
    N = [g["normal"][..., k].astype(F) for k in range(3)]
    sl, sz = F(sigma_l), F(sigma_z)
    col, var = px.copy(), v0.copy()
    first = 0
    if resume is not None:
        first, col, var = resume[0], resume[1].reshape(H, W).copy(), resume[2].reshape(H, W).copy()
    Y, X = np.mgrid[0:H, 0:W]

    def gather(a, yy, xx):
        return a[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]

    with np.errstate(all="ignore"):
        for k in range(first, iterations):
            s = (k + 1) if wrong == "linear_step" else (1 << k)
            gs, gw = np.zeros((H, W), F), np.zeros((H, W), F)
            gd = s if wrong == "prefilter_at_s" else 1
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = Y + gd * dy, X + gd * dx
                    ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W) & gather(tap_ok, yy, xx)
                    wgt = F(0.25) if dx == 0 and dy == 0 else (F(0.125) if dx == 0 or dy == 0 else F(0.0625))
                    gs = np.where(ok, gs + wgt * gather(var, yy, xx), gs).astype(F)
                    gw = np.where(ok, gw + wgt, gw).astype(F)
            gv = (gs / gw).astype(F)
            den = (sl * _sqrt(gv, "sqrt", part, census, daz) + EPS).astype(F)
            sw, sc, sv = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
            taps = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3)]
            if wrong == "dx_outer":
                taps = [(dy, dx) for dx in range(-2, 3) for dy in range(-2, 3)]
            for dy, dx in taps:
                yy, xx = Y + s * dy, X + s * dx
                ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W) & gather(tap_ok, yy, xx)
                if seam and s == seam[2]:
                    tq, tc = (xx, X) if seam[1] == "x" else (yy, Y)
                    ok &= (tq // s) // TILE[seam[1]] == (tc // s) // TILE[seam[1]]
                counted = ok & part
                h = F(HK[abs(dx)] * HK[abs(dy)])
                q = [gather(a, yy, xx) for a in N]
                wn = _pos(((N[0] * q[0] + N[1] * q[1]).astype(F) + N[2] * q[2]).astype(F))
                for _ in range(normal_pow):
                    wn = (wn * wn).astype(F)
                d = [(gather(a, yy, xx) - a).astype(F) for a in P]
                e = np.abs(((N[0] * d[0] + N[1] * d[1]).astype(F) + N[2] * d[2]).astype(F))
                t = _pos((F(1.0) - _div(e, sz, "e/sigma_z", counted, census, daz)).astype(F))
                wz = (t * t).astype(F)
                cq, vq = gather(col, yy, xx), gather(var, yy, xx)
                u = _pos((F(1.0) - _div(np.abs((cq - col).astype(F)), den, "dc/den", counted, census, daz)).astype(F))
                wl = (u * u).astype(F)
                w = (h * ((wn * wz).astype(F) * wl).astype(F)).astype(F)
                wv = w if wrong == "unsquared_var" else (w * w).astype(F)
                sw = np.where(ok, sw + w, sw).astype(F)
                sc = np.where(ok, sc + (w * cq).astype(F), sc).astype(F)
                sv = np.where(ok, sv + (wv * vq).astype(F), sv).astype(F)
            keep = ~part | (sw == 0)
            col = np.where(keep, col, _div(sc, sw, "sc/sw", ~keep, census, daz)).astype(F)
            var = np.where(keep, var, _div(sv, (sw * sw).astype(F), "sv/sw2", ~keep, census, daz)).astype(F)
            if trace is not None:
                trace.append((col.copy(), var.copy()))
    return col.reshape(-1), var.reshape(-1)


def same(a, b):
    """Bit for bit, every NaN equal to every NaN (the payload of a NaN an
    operation makes differs between x86 and gfx950)."""
    a, b = np.asarray(a, F).reshape(-1), np.asarray(b, F).reshape(-1)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------- rendered cases
RENDER = dict(n_rays=4, depth_max=3)
RENDER_SPP = 4
FRAMES = ((37, 23), (64, 48), (131, 67))
TINY_FRAMES = ((1, 1), (2, 3), (1, 7))


@functools.lru_cache(maxsize=None)
def box_plane(W, H, spp=RENDER_SPP, plane=GRID):
    """(img, m2) of the box scene after spp passes, replayed from the oracle's
    samples (adaptive_cases.replay, no mask)."""
    import oracle_binding
    p = capi.make_params(W, H, spp, **RENDER)
    vals, codes = oracle_binding.render_values(scenes.make_scene_box(), p)
    if plane == GUI:  # (a sample's value does not depend on the plane, its code does)
        codes = gc.codes(W, H, spp)
    img, m2 = ac.replay(np.asarray(vals), np.asarray(codes), None, plane)
    for a in list(img.values()) + [m2]:
        a.setflags(write=False)
    return img, m2


@functools.lru_cache(maxsize=None)
def box_guides(W, H, plane=GRID, spp_offset=0):
    g = scene_guides(scenes.make_scene_box(), W, H, plane, spp_offset)
    g.setflags(write=False)
    return g


# ---------------------------------------------------------------- synthetic guides
def crease_guides(W, H):
    """Two half-planes meeting at a crease at x = W/2: the left one z = 0
    (normal +z), the right one rising at 45 degrees."""
    g = np.zeros((H, W), capi.GuideRecord)
    g["kind"] = 1 | 4
    x = (np.arange(W, dtype=F) - F(W // 2)) * F(0.05)
    y = np.arange(H, dtype=F) * F(0.05)
    right = x > 0
    r = F(np.sqrt(0.5))
    g["pos"][..., 0] = np.where(right, x * r, x)[None, :]
    g["pos"][..., 1] = y[:, None]
    g["pos"][..., 2] = np.where(right, x * r, F(0.0))[None, :]
    g["normal"][..., 0] = np.where(right, -r, F(0.0))[None, :]
    g["normal"][..., 2] = np.where(right, r, F(1.0))[None, :]
    return g


def step_guides(W, H):
    """A depth step with equal normals: z drops by 0.5 at x = W/2."""
    g = np.zeros((H, W), capi.GuideRecord)
    g["kind"] = 1 | 4
    g["pos"][..., 0] = (np.arange(W, dtype=F) * F(0.05))[None, :]
    g["pos"][..., 1] = (np.arange(H, dtype=F) * F(0.05))[:, None]
    g["pos"][..., 2] = np.where(np.arange(W) >= W // 2, F(-0.5), F(0.0))[None, :]
    g["normal"][..., 2] = F(1.0)
    return g


def two_level_plane(W, H, seed=9):
    """(pixels, counters, m2): colour 0.25 left of x = W/2 and 0.75 from there
    on (where step_guides drops), random variances, every pixel sampled."""
    _, cn, m2 = random_plane(W, H, seed, holes=False)
    px = np.where(np.arange(W) >= W // 2, F(0.75), F(0.25)).astype(F)
    return np.tile(px, H), cn, m2


def random_plane(W, H, seed, holes=True):
    """(pixels, counters, m2): random colours and variances; with holes, some
    pixels starved (c < 2)."""
    rng = np.random.default_rng([W, H, seed])
    px = rng.random(W * H, dtype=F)
    cn = rng.integers(2, 9, W * H).astype(np.uint32)
    if holes:
        cn[rng.random(W * H) < 0.05] = 1
    m2 = (rng.random(W * H, dtype=F) * F(0.2)).astype(F)
    return px, cn, m2


# ---------------------------------------------------------------- lattice tiles
# Frames on which a 5 x 5 tap leaves its workgroup's 32 x 8 lattice tile: at
# step s along x iff W > 32 s, along y iff H > 8 s.
SEAM_FRAMES = ((300, 75), (1061, 9), (9, 277), (1061, 277))
SEAM_STEPS = (4, 8, 16, 32)


def spans_two_tiles(W, H, axis, S):
    return (W if axis == "x" else H) > TILE[axis] * S


# ---------------------------------------------------------------- edge planes
# Inputs whose divisions and roots leave the windows of DIV_WINDOW and
# SQRT_WINDOW, or are denormal (the census says which, tests/test_denoise_cpu.py
# pins it); random_plane's own never do.
def scaled_plane(W, H, seed, e):
    """random_plane with the colours times 2^e and m2 times 2^(2e)."""
    px, cn, m2 = random_plane(W, H, seed)
    return (px * F(2.0 ** e)).astype(F), cn, (m2 * F(2.0 ** (2 * e))).astype(F)


def scaled_world(g, e):
    """The guides with every position times 2^e (sigma_z is the caller's)."""
    g = g.copy()
    g["pos"] = (g["pos"] * F(2.0 ** e)).astype(F)
    return g


def scaled_normals(g, e):
    """The guides with every normal times 2^e."""
    g = g.copy()
    g["normal"] = (g["normal"] * F(2.0 ** e)).astype(F)
    return g


COUNTER_SETS = {
    "2p24": (2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3),
    "2p31": (2 ** 31 - 1, 2 ** 31, 2 ** 31 + 129, 2 ** 32 - 1),
}
COUNTER_SETS["mix"] = (2, 3, 2 ** 20, 2 ** 21) + COUNTER_SETS["2p24"] + COUNTER_SETS["2p31"]


def counter_plane(W, H, seed, values):
    """random_plane with every sampled pixel's counter drawn from `values` and
    m2 times nf * (nf - 1) in float32, so that var0 stays of random_plane's
    order; the starved pixels stay starved."""
    px, cn, m2 = random_plane(W, H, seed)
    rng = np.random.default_rng([W, H, seed, 77])
    drawn = np.asarray(values, np.uint32)[rng.integers(0, len(values), W * H)]
    cn = np.where(cn >= 2, drawn, cn).astype(np.uint32)
    nf = cn.astype(F)
    return px, cn, (m2 * (nf * (nf - F(1.0))).astype(F)).astype(F)


EDGE_SEED = 3
EDGE_OVERFLOW = "normal_e-32_pow1"  # sw is denormal and sw * sw is 0: the variance is sv / 0 everywhere
# (colour_e-70_it1: after two iterations at 2^-70 every variance has underflowed
# to 0 and the colour ramp is 2^-20 whatever the root, so only one iteration
# shows a filter that flushes denormals there)
EDGE_CASES = tuple(
    ["colour_e%d" % e for e in (-70, -64, -50, 45, 63)] + ["colour_e-70_it1", "colour_e-64_it5", "colour_e63_it5"] +
    ["world_e%d" % e for e in (-140, -120, -45, 45, 60)] +
    ["sigma_l_inf", "sigma_l_3e38", "sigma_l_1e-45", "sigma_z_inf", "sigma_z_3e38", "sigma_z_1e-45"] +
    ["normal_e-30_pow0", "normal_e10_pow0", EDGE_OVERFLOW] +
    ["counters_%s" % k for k in COUNTER_SETS])


def edge_case(name, W=67, H=35):
    """(pixels, counters, m2, guides, denoise()'s keywords) of one of EDGE_CASES:
    crease guides, 3 iterations and sigma_l 6 unless the name says otherwise."""
    plane, g = random_plane(W, H, EDGE_SEED), crease_guides(W, H)
    kw = dict(iterations=3, sigma_l=6.0)
    kind, _, rest = name.partition("_")
    if kind == "colour":
        e, _, it = rest.partition("_it")
        plane = scaled_plane(W, H, EDGE_SEED, int(e[1:]))
        kw["iterations"] = int(it) if it else 3
    elif kind == "world":
        e = int(rest[1:])
        g = scaled_world(g, e)
        kw["sigma_z"] = float(F(DEFAULTS["sigma_z"]) * F(2.0 ** e))
    elif kind == "sigma":
        which, _, val = rest.partition("_")
        kw["sigma_" + which] = float(F(val))
    elif kind == "normal":
        e, _, npow = rest.partition("_pow")
        g = scaled_normals(g, int(e[1:]))
        kw["sigma_z"] = float(F(DEFAULTS["sigma_z"]) * F(2.0 ** int(e[1:])))
        kw["normal_pow"] = int(npow)
    elif kind == "counters":
        plane = counter_plane(W, H, EDGE_SEED, COUNTER_SETS[rest])
    else:
        raise KeyError(name)
    return plane + (g, kw)


# single pixels' guide values that are no numbers, by name: (field, component, bits)
GUIDE_POISON = (
    ("pos_nan", "pos", 0, 0xffffffff), ("pos_snan", "pos", 1, 0x7f800001), ("normal_nan", "normal", 2, 0xffffffff),
    ("pos_inf", "pos", 2, 0x7f800000), ("normal_pinf", "normal", 0, 0x7f800000),
    ("normal_ninf", "normal", 2, 0xff800000))
GUIDE_KINDS = (0, 2, 3, 0x81, 0xfd, 0xfe)  # by kind & 3, 0x81 and 0xfd take part


def poisoned_guides(g, part, infinite_normals=True):
    """(guides, {name: flat index}, {flat index: kind}): g with GUIDE_POISON on
    single pixels and GUIDE_KINDS on others, a dozen pixels spread over the
    participating interior (the recipe of the GPU suite's poisoned-pixel test).
    A NaN or infinite position and a NaN normal give every tap of and on their
    pixel the weight 0; an infinite normal does not (wn = inf meets wz = 0 and
    inf * 0 is NaN), so its pixel and the taps that reach it become NaN:
    without infinite_normals those two pixels keep their guides."""
    H, W = g.shape
    g = g.copy()
    idx = np.flatnonzero(part.reshape(H, W)[2:H - 3, 2:W - 2].reshape(-1))
    sel = [int(i) for i in idx[np.linspace(0, idx.size - 1, len(GUIDE_POISON) + len(GUIDE_KINDS)).astype(int)]]
    at = [(2 + i // (W - 4)) * W + 2 + i % (W - 4) for i in sel]
    where, kinds = {}, {}
    for (name, field, k, bits), i in zip(GUIDE_POISON, at[0::2]):
        if not infinite_normals and name in ("normal_pinf", "normal_ninf"):
            continue
        g[field][i // W, i % W, k] = np.uint32(bits).view(F)
        where[name] = i
    for kind, i in zip(GUIDE_KINDS, at[1::2]):
        g["kind"][i // W, i % W] = kind
        kinds[i] = kind
    return g, where, kinds


def reach(W, H, at, r):
    """The pixels within Chebyshev distance r of one of the flat indices `at`."""
    m = np.zeros((H, W), bool)
    for i in at:
        y, x = divmod(int(i), W)
        m[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = True
    return m.reshape(-1)
