"""Frames for the GridRenderPlane drift-replay tests, each with the CPU-side
conditions that make it discriminating. Shared by tests/test_drift_cpu.py
(the conditions alone, oracle only) and tests/test_gpu_drift.py (the same
frames through the kernels); oracle results are computed once per process and
are read-only.

A sample drifts when (float)(i + u) / N * N truncates to a pixel next to its
source pixel, which happens at a rate of about i * 2^-24 per sample: frames
below a few hundred pixels a side hold no drifted sample at all, a line of
60000 pixels holds a few hundred per pass. The code of a sample is
(dx + 1) | (dy + 1) << 2 relative to its nominal destination (ix,
max(H - 2 - iy, 0)); 0x05 is "no drift". Codes depend on the seed, the pass,
the source pixel, W and H only, so every count below is a constant of the
default seed (capi.make_params) and is pinned: a change of seed or jitter that
removed the drift would fail tests/test_drift_cpu.py instead of silently
hollowing the GPU tests out."""
import functools

import numpy as np

import oracle_binding as ob
from ipt_amd import capi, scenes

N_RAYS, DEPTH_MAX = 4, 3  # the tree of every thin-frame case
SPPS = (2, 9)             # 9: more than eight passes through both branches of the replay

WIDE, TALL = (60000, 3), (3, 60000)   # (W, H)
WIDE_MAX, TALL_ODD = (65536, 2), (2, 65535)
MIXED = (4099, 61)                    # both axes, neither a power of two
MAX_HEIGHT = (2, 65536)               # validate()'s tallest frame: its own test
THIN = (WIDE, TALL, WIDE_MAX, TALL_ODD)
FRAMES = THIN + (MIXED,)

# {(W, H, spp): {code: samples}}, measured with the oracle (passes 0..spp-1)
HIST = {
    (60000, 3, 2): {0x4: 6, 0x6: 461},
    (60000, 3, 4): {0x4: 10, 0x6: 912},
    (60000, 3, 9): {0x4: 20, 0x6: 2025, 0x9: 2},
    (3, 60000, 2): {0x1: 3, 0x9: 737},
    (3, 60000, 4): {0x1: 12, 0x9: 1475},
    (3, 60000, 9): {0x1: 21, 0x9: 3335},
    (65536, 2, 2): {0x6: 344},
    (65536, 2, 9): {0x6: 1532, 0x9: 2},
    (2, 65535, 2): {0x9: 594},
    (2, 65535, 9): {0x9: 2629},
    (2, 65536, 2): {0x9: 594},
    (4099, 61, 2): {0x6: 38, 0x9: 2},
    (4099, 61, 9): {0x6: 180, 0x9: 6},
}
# drifted samples with a non-zero radiance, same keys
NONZERO = {
    (60000, 3, 2): 194, (60000, 3, 4): 387, (60000, 3, 9): 883,
    (3, 60000, 2): 337, (3, 60000, 4): 665, (3, 60000, 9): 1476,
    (65536, 2, 2): 150, (65536, 2, 9): 666,
    (2, 65535, 2): 288, (2, 65535, 9): 1234,
    (2, 65536, 2): 288,
    (4099, 61, 2): 10, (4099, 61, 9): 75,
}

# A drifted sample is added out of its pixel's nominal order only when the
# destination's own nominal source comes later in the raster: the row below
# (dy = -1, source row iy + 1) or the next column (dy = 0, dx = +1). With
# dy = +1, or dy = 0 and dx = -1, the nominal sample has already been added,
# and a replay that defers drifted samples to the end of their pass is right
# by accident.
ORDER_SENSITIVE = (0x0, 0x1, 0x2, 0x6)

# Diagonal codes. The default seed's 2048^2 passes 0..95 hold 0xa (dx = dy =
# +1) twice. 0x8 (dx = -1, dy = +1) turned up once in a codes-only scan of the
# squares of side 2047, 2039, 2001, 1999, 1920 and 1531, passes 0..255, seeds
# 20241223, 1, 2, 3 and 0xC0FFEE (2.9e10 samples: 0xa 93 times); 0x0 and 0x2
# (dy = -1 with dx = -1 or +1) did not: no render in the suite reaches them.
# The replay probe does (ipt_replay_samples on tests/replay_cases.py's chosen
# samples: every code, densely, and one code at a time).
# Each case renders its one pass at the shallowest tree for which the oracle's
# value at the diagonal sample is non-zero:
# (code, side, seed, spp_offset, source ix, source iy, n_rays, depth_max, value)
DEFAULT_SEED = 20241223
DIAGONAL = (
    (0xa, 2048, DEFAULT_SEED, 19, 133, 1241, 2, 2, 0.02293148636817932),
    (0xa, 2048, DEFAULT_SEED, 90, 1596, 1361, 1, 2, 0.010200029239058495),
    (0x8, 1531, 1, 223, 817, 939, 2, 2, 0.3901532292366028),
)
DIAGONAL_UNREACHED = (0x0, 0x2)  # by a render; replay_cases.DIAG_DOWN reaches them

# sharded plans (tile_rows, n_shards) and the passes each is rendered with.
# CROSS pins the drifted samples whose nominal and actual destination rows
# belong to different shards (the 0xfe halo samples of the nominal row's
# owner). The wide frame drifts along x: only its two 0x9 samples (source row
# 0, passes 7 and 8) change rows at all, and passes 0..127 hold no third, so
# it is rendered with nine passes and the floor of 20 such samples is asked
# of the tall frame's one-row plans.
SHARD_PLANS = {
    TALL: ((1, 2), (1, 3), (7, 3), (16, 8)),
    WIDE: ((1, 2), (1, 3), (2, 2)),
}
SHARD_SPP = {TALL: 2, WIDE: 9}
CROSS = {
    (TALL, 1, 2): 740, (TALL, 1, 3): 740, (TALL, 7, 3): 113, (TALL, 16, 8): 50,
    (WIDE, 1, 2): 2, (WIDE, 1, 3): 2, (WIDE, 2, 2): 2,
}
# the (1, 3) tall plan's variants: four passes chunked, four passes in two calls
CROSS_TALL_SPP4 = 1487

PLANE_KEYS = (("pixels", np.float32), ("counters", np.uint32), ("sums", np.float32), ("pixel_max", np.float32))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def plane(W, H):
    return {k: np.zeros(W * H, dt) for k, dt in PLANE_KEYS}


def params(W, H, spp, **kw):
    kw.setdefault("n_rays", N_RAYS)
    kw.setdefault("depth_max", DEPTH_MAX)
    return capi.make_params(W, H, spp, **kw)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def oracle_samples(W, H, spp, spp_offset=0, n_rays=N_RAYS, depth_max=DEPTH_MAX, seed=DEFAULT_SEED):
    """(values, codes, counters) of the box scene by the oracle; read-only."""
    p = capi.make_params(W, H, spp, spp_offset=spp_offset, n_rays=n_rays, depth_max=depth_max, seed=seed)
    v, c, cnt = ob.render_values(scenes.make_scene_box(), p, with_counters=True)
    _frozen(v, c)
    return v, c, cnt


@functools.lru_cache(maxsize=None)
def oracle_plane(W, H, spp, spp_offset=0, n_rays=N_RAYS, depth_max=DEPTH_MAX, seed=DEFAULT_SEED):
    """ob.accumulate of oracle_samples from zeros; read-only."""
    v, c, _ = oracle_samples(W, H, spp, spp_offset, n_rays, depth_max, seed)
    ref = ob.accumulate(v, c)
    _frozen(*ref.values())
    return ref


def histogram(codes):
    u, n = np.unique(codes, return_counts=True)
    return {int(a): int(b) for a, b in zip(u, n) if a != 0x05}


def destinations(codes):
    """(nominal row, destination row, destination column) of every sample of
    codes [spp][H][W]."""
    _, H, W = codes.shape
    iy = np.arange(H, dtype=np.int64)[None, :, None]
    ix = np.arange(W, dtype=np.int64)[None, None, :]
    yn = np.broadcast_to(np.maximum(H - 2 - iy, 0), codes.shape)
    c = codes.astype(np.int64)
    return yn, yn + ((c >> 2) & 3) - 1, ix + (c & 3) - 1


def shard_of(rows, tile_rows, n_shards):
    return (rows // tile_rows) % n_shards


def cross_shard(codes, tile_rows, n_shards):
    """Drifted samples whose nominal and actual destination rows have
    different owners."""
    yn, yi, _ = destinations(codes)
    d = codes != 0x05
    return int((shard_of(yn[d], tile_rows, n_shards) != shard_of(yi[d], tile_rows, n_shards)).sum())


# ---- a numpy restatement of the replay, and two wrong ones -----------------
def _add_rays(img, dest, vals):
    """GridRenderPlane::addRay of the events (dest[k], vals[k]) in order.
    Events of different pixels commute, so the k-th event of every pixel is
    applied as one vector step."""
    if dest.size == 0:
        return
    order = np.argsort(dest, kind="stable")
    ds, vs = dest[order], vals[order]
    first = np.r_[0, np.flatnonzero(ds[1:] != ds[:-1]) + 1]
    rank = np.arange(ds.size) - np.repeat(first, np.diff(np.r_[first, ds.size]))
    with np.errstate(all="ignore"):
        for r in range(int(rank.max()) + 1):
            m = rank == r
            d, v = ds[m], vs[m]
            c = img["counters"][d].astype(np.uint64)
            p = (img["pixels"][d] * c.astype(np.float32) + v) / (c + 1).astype(np.float32)
            img["pixels"][d] = p
            img["counters"][d] = (c + 1).astype(np.uint32)
            img["sums"][d] += v
            img["pixel_max"][d] = np.where(p > img["pixel_max"][d], p, img["pixel_max"][d])


def replay(values, codes, how="raster"):
    """The plane after the samples, from zeros.
    "raster":       passes, rows, columns -- render_sample's order; must equal
                    ob.accumulate (test_drift_cpu.py checks that it does);
    "drift_last":   wrong: a pass's drifted samples after its nominal ones;
    "nominal_only": wrong: samples with a code other than 0x05 are dropped."""
    spp, H, W = values.shape
    img = plane(W, H)
    _, yi, xi = destinations(codes)
    dest = (yi * W + xi).reshape(spp, -1)
    vals = values.reshape(spp, -1)
    drift = (codes != 0x05).reshape(spp, -1)
    for s in range(spp):
        if how == "raster":
            _add_rays(img, dest[s], vals[s])
        elif how == "drift_last":
            k = np.r_[np.flatnonzero(~drift[s]), np.flatnonzero(drift[s])]
            _add_rays(img, dest[s][k], vals[s][k])
        elif how == "nominal_only":
            _add_rays(img, dest[s][~drift[s]], vals[s][~drift[s]])
        else:
            raise ValueError(how)
    return img


# ---- preloaded planes --------------------------------------------------------
SMALL = (13, 11)
SMALL_SPPS = (7, 8, 9, 16, 17)
BIG_MAX = np.float32(1e30)  # above every running mean of the box scene


def preload_kinds(spp, per_pass=3):
    """The preloaded values by array. The last counter leaves room for three
    samples per pass (a pixel's nominal one, row 0's second one, a drifted
    one; test_drift_cpu.py checks the frames' own maxima) below the uint32
    wrap (ipt_capi.h, ipt_image); per_pass: for more than three
    (replay_cases.py's injected samples)."""
    return {
        "counters": (0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31, 0xfffffffe - spp * per_pass),
        "pixels": ("random", "negative", "-0", "subnormal", "+inf", "nan"),
        "pixel_max": ("zero", "big", "-1", "nan"),
        "sums": ("random", "+inf"),
    }


def preload(W, H, spp, hot=None, seed=7, per_pass=3):
    """(plane, kind index per pixel and array): a seeded mix of
    preload_kinds(spp). `hot` (pixel indices, e.g. the destinations of the
    drifted samples) count through the kinds of the four arrays as the digits
    of a mixed-radix number, so that each kind -- and each combination, given
    336 of them -- sits on some.

    One pairing is excluded: +inf pixels never get counter 0. inf * 0 makes a
    NaN out of no NaN, and the sign bit of such a generated NaN is the
    processor's choice (x86 sets it, the GPU does not); every other pairing
    only propagates its operands."""
    rng = np.random.default_rng(seed)
    n = W * H
    kinds = preload_kinds(spp, per_pass)
    pick = {k: rng.integers(0, len(v), n) for k, v in kinds.items()}
    if hot is not None:
        hot = np.unique(hot)
        j = np.arange(hot.size)
        for k, v in kinds.items():  # mixed radix: 7 * 6 * 4 * 2 = 336 pixels see every combination
            pick[k][hot] = j % len(v)
            j = j // len(v)
    clash = (pick["pixels"] == kinds["pixels"].index("+inf")) & (pick["counters"] == 0)
    pick["counters"][clash] = 1 + (np.flatnonzero(clash) % (len(kinds["counters"]) - 1))
    rnd = (rng.random(n, dtype=np.float32) * np.float32(0.25)).astype(np.float32)
    img = plane(W, H)
    img["counters"][:] = np.array(kinds["counters"], np.uint32)[pick["counters"]]
    px = np.stack([rnd, -rnd, np.full(n, -0.0, np.float32), np.full(n, 2.0 ** -140, np.float32),
                   np.full(n, np.inf, np.float32), np.full(n, np.nan, np.float32)])
    img["pixels"][:] = px[pick["pixels"], np.arange(n)]
    mx = np.array([0.0, BIG_MAX, -1.0, np.nan], np.float32)
    img["pixel_max"][:] = mx[pick["pixel_max"]]
    sm = np.stack([rnd * np.float32(3.0), np.full(n, np.inf, np.float32)])
    img["sums"][:] = sm[pick["sums"], np.arange(n)]
    return img, pick


def copy_plane(img):
    return {k: v.copy() for k, v in img.items()}
