"""Inputs of the display-statistics GPU tests (tests/test_gpu_display_stats.py),
built on the CPU, and the conditions under which they discriminate
(asserted on the reference alone in tests/test_display_stats_cpu.py)."""
import functools

import numpy as np

import stats_ref as sr

CUTOFF = 1.01  # the Gui's glare cutoff
SHAPES = ((1, 1), (1, 7), (5, 17), (37, 23), (640, 640), (257, 1024), (4096, 512), (1024, 1024))
OFFSET_SHAPES = ((37, 23), (257, 1024))
SEL_BITS = (11, 11, 10)  # the library's radix split, most significant digit first


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def shape_image(W, H):
    """A dim render-like plane (u^3 / 2) with a dozen pixels above the cutoff:
    the glare stage has work, the oracle's O(n * bright) stays cheap."""
    rng = np.random.default_rng(1000 * W + H)
    n = W * H
    u = rng.random(n, dtype=np.float32)
    img = (u * u * u * np.float32(0.49)).astype(np.float32)
    k = min(12, max(n // 8, 1))
    img[rng.choice(n, k, replace=False)] = (rng.random(k, dtype=np.float32) * 40 + np.float32(1.5)).astype(np.float32)
    return img


@functools.lru_cache(maxsize=None)
def shape_ref(W, H, glare):
    """(image, rank, reference), computed once per shape and glare mode."""
    img = shape_image(W, H)
    img.setflags(write=False)
    k = sr.white_rank_for(W, H, 0.95)
    return img, k, sr.stats_ref(img, W, H, CUTOFF if glare else 0.0, 400, k)


# ---- histogram edges ---------------------------------------------------------
def inner_edge_image(nb=400, mx=3.0):
    """The image's maximum and, for each of the nb - 1 inner bucket edges
    vmin + j (vmax - vmin) / nb (double), the three floats around its f32
    rounding."""
    mx = np.float32(mx)
    vmin, vmax = np.float64(mx / np.float32(100000.0)), np.float64(mx)
    e = (vmin + np.arange(1, nb, dtype=np.float64) * (vmax - vmin) / nb).astype(np.float32)
    around = np.stack([np.nextafter(e, np.float32(-np.inf)), e, np.nextafter(e, np.float32(np.inf))], 1).reshape(-1)
    return np.concatenate([[mx], around]).astype(np.float32)


def spread_image():
    rng = np.random.default_rng(51)
    return (rng.random(97 * 33, dtype=np.float32) * np.float32(3.0)).astype(np.float32)


def hist_edge_cases():
    """[(name, W, H, image, buckets)]"""
    rng = np.random.default_rng(53)
    n = 64 * 48
    rnd = (rng.random(n, dtype=np.float32) * np.float32(3.0)).astype(np.float32)
    nan0, nan100, inf1 = rnd.copy(), rnd.copy(), rnd.copy()
    nan0[0] = np.nan
    nan100[100] = np.nan
    inf1[[5, 1234]] = np.inf
    sub = f32(rng.integers(1, 0x2000, n).astype(np.uint32))  # subnormals: max / 100000.0f underflows to 0
    edges = inner_edge_image()
    out = [("constant", 512, 512, np.full(512 * 512, 0.3, np.float32), 400),
           ("zeros", 64, 48, np.zeros(n, np.float32), 400),
           ("negative_max", 64, 48, (-rnd - np.float32(0.5)).astype(np.float32), 400),
           ("inf_max", 64, 48, inf1, 400),
           ("nan_first", 64, 48, nan0, 400),
           ("nan_elsewhere", 64, 48, nan100, 400),
           ("subnormal_max", 64, 48, sub, 400),
           ("inner_edges", edges.size // 2, 2, edges, 400)]
    out += [(f"buckets_{nb}", 97, 33, spread_image(), nb) for nb in (1, 2, 400, 4095, 4096)]
    return out


# ---- selection edges ---------------------------------------------------------
def select_trace(img, k, bits=SEL_BITS):
    """Per radix pass (remaining rank, size of the chosen digit's bin) of the
    selection of rank k < n, most significant digit first."""
    keys = np.sort(sr.keys(img))
    out, shift = [], 32
    for b in bits:
        shift -= b
        chosen = keys[k] >> shift
        lo = int(np.searchsorted(keys >> shift, chosen, "left"))
        hi = int(np.searchsorted(keys >> shift, chosen, "right"))
        out.append((k - lo, hi - lo))
        keys, k = keys[lo:hi], k - lo
    return out


def bin_edge_image():
    """Three top-digit bins (keys of 1.x, 2.x and 4.x), each with several
    middle and low digits and with duplicates of its smallest and largest
    element; BIN_EDGE_RANKS are the first and the last element of the middle
    bin: the remaining rank is 0, respectively count - 1, in every pass."""
    rng = np.random.default_rng(59)
    parts = []
    for base in (0x3f800000, 0x40000000, 0x40800000):  # top 11 bits differ; bits 20..0 free
        body = base + rng.integers(0x100, 0x1fff00, 300).astype(np.uint32)
        parts.append(np.concatenate([[base + 7] * 3, body, [base + 0x1fffff] * 3]).astype(np.uint32))
    img = f32(np.concatenate(parts))
    return f32(rng.permutation(img.view(np.uint32)))


BIN_EDGE_RANKS = (306, 611)


def select_edge_cases():
    """[(name, W, H, image, ranks)]; a rank >= n selects the maximum."""
    rng = np.random.default_rng(61)
    n = 37 * 23
    rnd = (rng.random(n, dtype=np.float32) * np.float32(3.0)).astype(np.float32)
    two = np.where(rng.random(n) < 0.4, np.float32(1.0), np.float32(4.0)).astype(np.float32)
    ones = int((two == 1.0).sum())
    low = f32(0x3f800000 + rng.integers(0, 1024, n).astype(np.uint32))           # only the last digit differs
    high = f32((rng.integers(1, 0x3fc, n).astype(np.uint32) << 21))             # only the first digit differs
    signs = np.concatenate([-rnd[:300], rnd[300:600], np.zeros(100, np.float32), -np.zeros(100, np.float32),
                            [np.inf, -np.inf, np.inf]]).astype(np.float32)
    signs = signs[rng.permutation(signs.size)]
    nans = rnd.copy()
    nans[rng.choice(np.arange(1, n), 40, replace=False)] =f32(np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff8fffff] * 10))
    nans[0] = 1.0
    m = signs.size
    return [("ranks", 37, 23, rnd, (0, 1, n // 2, n - 2, n - 1, n, 2 * n)),
            ("constant", 37, 23, np.full(n, 0.3, np.float32), (0, n // 2, n - 1)),
            ("two_valued", 37, 23, two, (ones - 1, ones)),
            ("low_digit", 37, 23, low, (0, 17, n // 2, n - 1)),
            ("high_digit", 37, 23, high, (0, 17, n // 2, n - 1)),
            ("signs_zeros_infs", m, 1, signs, (0, 1, 300, 301, 400, 401, 500, 501, m - 3, m - 2, m - 1)),
            ("nans", 37, 23, nans, (n - 42, n - 41, n - 40, n - 20, n - 1)),
            ("bin_edges", 306, 3, bin_edge_image(), BIN_EDGE_RANKS)]


def percentile_image():
    """A dim plane with the emitter in view: 1 % of the pixels 1000 times
    brighter than the rest, so the max-normalised picture is nearly black."""
    rng = np.random.default_rng(67)
    n = 96 * 64
    u = rng.random(n, dtype=np.float32)
    img = (u * u * np.float32(0.8) + np.float32(0.01)).astype(np.float32)
    img[rng.choice(n, n // 100, replace=False)] = np.float32(900.0)
    return 96, 64, img
