"""CPU reference of the display statistics (ipt_display_stats /
ipt_display_stats_device), restated in numpy:

  histogram  CImg get_histogram(nb, mx / 100000.0f, mx) (gui.cpp:83-88), in
             float64 with CImg's expression order
  selection  CImg kth_smallest(k) by sorting the order-preserving integer keys
             (-0 before +0, NaNs of either sign after +inf -> 0x7fc00000)
  tone       display_ref's arithmetic with the white point in place of the max

and the reader of tests/golden/ref_display_stats.bin, what the reference's own
CImg returns for the cases of tests/native/ref_cimg_stats.cpp."""
import struct
from pathlib import Path

import numpy as np

import display_ref as dr

HERE = Path(__file__).resolve().parent
GOLDEN = HERE / "golden" / "ref_display_stats.bin"
QNAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]
CASE_NAMES = ("spread", "percentile", "mixed_sign", "1x1", "constant", "zeros", "negative_max", "inf_max",
              "subnormal_max", "buckets_4096", "two_valued")


def cimg_cases(path=GOLDEN):
    """[{name, W, H, nb, k, px, hist, mx, kth}] of the fixture."""
    data = Path(path).read_bytes()
    count, = struct.unpack_from("<I", data, 0)
    assert count == len(CASE_NAMES)
    pos, out = 4, []
    for name in CASE_NAMES:
        W, H, nb, _, k = struct.unpack_from("<iiiiq", data, pos)
        pos += 24
        px = np.frombuffer(data, np.float32, W * H, pos)
        pos += 4 * W * H
        hist = np.frombuffer(data, np.uint32, nb, pos)
        pos += 4 * nb
        mx, kth = np.frombuffer(data, np.float32, 2, pos)
        pos += 8
        out.append(dict(name=name, W=W, H=H, nb=nb, k=k, px=px, hist=hist, mx=mx, kth=kth))
    assert pos == len(data)
    return out


def white_rank_for(width, height, fraction):
    """arg.width()*arg.height()*0.95 (gui.cpp:13): int product, double multiply, cast."""
    return int(np.float64(int(width) * int(height)) * np.float64(fraction))


def hist_bounds(a):
    """(mx, lo = mx / 100000.0f, vmin, vmax): Gui's arguments and CImg's swap."""
    mx = dr.fold_max(np.ascontiguousarray(a, np.float32).reshape(-1))
    with np.errstate(all="ignore"):
        lo = np.float32(mx) / np.float32(100000.0)
    lt = bool(lo < mx)
    return mx, lo, np.float64(lo if lt else mx), np.float64(mx if lt else lo)


def histogram(a, nb):
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    _, _, vmin, vmax = hist_bounds(a)
    val = a.astype(np.float64)
    with np.errstate(all="ignore"):
        inside = (val >= vmin) & (val <= vmax)
        v = val[inside]
        top = v == vmax
        q = (v[~top] - vmin) * np.float64(nb) / (vmax - vmin)
    idx = np.full(v.size, nb - 1, np.int64)
    idx[~top] = q.astype(np.int64)  # (unsigned) of a value in [0, nb)
    return np.bincount(idx, minlength=nb).astype(np.uint32)


def keys(a):
    u = np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)
    k = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[(u & 0x7fffffff) > 0x7f800000] = 0xffffffff
    return k


def unkey(k):
    k = np.uint32(k)
    if k == 0xffffffff:
        return QNAN
    u = np.uint32(k & np.uint32(0x7fffffff)) if k & 0x80000000 else np.uint32(~k)
    return np.array([u], np.uint32).view(np.float32)[0]


def kth_smallest(a, k):
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    if k >= a.size:
        return dr.fold_max(a)
    return unkey(np.sort(keys(a))[k])


def tone_map(processed, white):
    p = np.ascontiguousarray(processed, np.float32)
    with np.errstate(all="ignore"):
        v = (p / np.float32(white)).astype(np.float32)
    return dr.cut01(dr.libm_powf(v, dr.GAMMA))


def stats_ref(pixels, W, H, glare_cutoff=0.0, nb=400, white_rank=-1):
    """{processed, tone, gray8, hist, stats} of a W x H float32 image. A
    glare_cutoff > 0 needs the built oracle (the `oracle` fixture)."""
    px = np.ascontiguousarray(pixels, np.float32).reshape(-1)
    assert px.size == W * H
    processed = dr.oracle_glare(px, W, H, glare_cutoff) if glare_cutoff > 0 else px.copy()
    mx, lo, _, _ = hist_bounds(processed)
    white = mx if white_rank < 0 else kth_smallest(processed, white_rank)
    tone = tone_map(processed, white)
    return {"processed": processed, "tone": tone, "gray8": dr.to_gray8(tone),
            "hist": histogram(processed, nb) if nb > 0 else np.zeros(0, np.uint32),
            "stats": pack(mx, lo, white, np.float32(0.0))}


def bits1(v):
    """The bit pattern of one float32, as an int."""
    return int(np.array(v, np.float32).reshape(1).view(np.uint32)[0])


def pack(*vals):
    """float32 array of the scalars, bit patterns kept (NaN payloads included)."""
    return np.array([np.array(v, np.float32).reshape(1).view(np.uint32)[0] for v in vals], np.uint32).view(np.float32)
