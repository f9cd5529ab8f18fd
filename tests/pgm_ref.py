"""CPU reference of the PGM path (ipt_smooth_device / ipt_pgm_device):
main.cpp:291-309, GridRenderPlane::smooth -> computeSmoothedMax -> n_val,
restated in numpy float32 from independent parts:

  smooth     the window sum in the reference's order (yy outer, xx inner, float
             adds), accum / (float)(side*side); pinned to the compiled
             reference by tests/golden/ref_smooth.bin (tests/test_pgm_cpu.py)
  folds      from 0 with `>`: the largest positive element, +0 without one
  logf/powf  the host libm's, through tests/native/logf_ref.c / powf_ref.c
  n_val      pinned to the host layer's compiled ipt::n_val (tests/native/
             pgm_dump.cpp, tests/test_pgm_cpu.py)
"""
import ctypes as C
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np

import display_ref as dr

HERE = Path(__file__).resolve().parent
GOLD_SMOOTH = HERE / "golden" / "ref_smooth.bin"
ONE, B500, FLT_MAX = 0x3f800000, 0x43fa0000, 0x7f7fffff
NEXT1 = np.uint32(ONE + 1).view(np.float32)  # nextafter(1)
# (contrast, gamma): main.cpp's, a second pair, log(contrast) at its smallest and near its largest
PAIRS = ((500.0, 0.6), (2.0, 0.5), (float(NEXT1), 0.6), (3e38, 0.6))

_logf_lib = None


def logf_lib():
    global _logf_lib
    if _logf_lib is None:
        so = Path(tempfile.mkdtemp(prefix="logf_ref")) / "logf_ref.so"
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-builtin", "-o", str(so),
                        str(HERE / "native" / "logf_ref.c"), "-lm", "-lpthread"], check=True)
        lib = C.CDLL(str(so))
        lib.logf_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int]
        lib.logf_eval.restype = None
        _logf_lib = lib
    return _logf_lib


def libm_logf(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    logf_lib().logf_eval(x.ctypes.data, out.ctypes.data, x.size, min(16, os.cpu_count() or 1))
    return out


def floats(lo_bits, hi_bits, stride=1):
    """The floats of the bit patterns lo_bits, lo_bits + stride, ... <= hi_bits."""
    return np.arange(lo_bits, hi_bits + 1, stride, dtype=np.uint64).astype(np.uint32).view(np.float32)


def logf_edges():
    """1 and its neighbour, 500 and both neighbours, the first and last pattern
    of each of logf's 16 table intervals across two binades, FLT_MAX."""
    pats = [ONE, ONE + 1, B500 - 1, B500, B500 + 1, FLT_MAX]
    # interval i of binade k starts where (ix - 0x3f330000) has bits 19..22 == i
    for start in range(0x3f330000 + (1 << 23), 0x3f330000 + 3 * (1 << 23), 1 << 19):
        pats += [start, start + (1 << 19) - 1]
    return np.array(sorted(set(pats)), np.uint32).view(np.float32)


def fold_max0(a):
    """`if (v > max) max = v` from 0: the largest positive element, else +0."""
    a = np.asarray(a, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        pos = a[a > 0]
    return pos.max() if pos.size else np.float32(0.0)


def smooth(px, W, H, side):
    """(pixels after GridRenderPlane::smooth(side), its max_value). The in-place
    filter reads only pixels it has not written yet, so it equals this
    out-of-place one (ipt_post.hip's header)."""
    src = np.ascontiguousarray(px, np.float32).reshape(H, W)
    out = src.copy()
    if side < 2 or side > W or side > H:
        return out.reshape(-1), np.float32(0.0)
    acc = np.zeros((H - side + 1, W - side + 1), np.float32)
    with np.errstate(all="ignore"):
        for yy in range(side):
            for xx in range(side):
                acc = (acc + src[side - 1 - yy:H - yy, side - 1 - xx:W - xx]).astype(np.float32)
        acc = (acc / np.float32(side * side)).astype(np.float32)
    out[side - 1:, side - 1:] = acc
    return out.reshape(-1), fold_max0(acc)


def smooth_golden_cases():
    """[(W, H, side, input, smooth(input), smooth's max, computeSmoothedMax's)]
    of tests/golden/ref_smooth.bin, the compiled reference's outputs."""
    d = np.fromfile(GOLD_SMOOTH, np.float32)
    n, pos, out = int(d[0]), 1, []
    for _ in range(n):
        W, H, side = (int(v) for v in d[pos:pos + 3])
        pos += 3
        inp = d[pos:pos + W * H]
        pos += W * H
        sm = d[pos:pos + W * H]
        pos += W * H
        out.append((W, H, side, inp, sm, d[pos], d[pos + 1]))
        pos += 2
    return out


def n_val(v, mx, contrast=500.0, gamma=0.6):
    """ipt::n_val (main.cpp:225-235) of every element, as uint8."""
    v = np.ascontiguousarray(v, np.float32).reshape(-1)
    c, mx = np.float32(contrast), np.float32(mx)
    with np.errstate(all="ignore"):
        adj = ((v * c).astype(np.float32) / mx).astype(np.float32)
        adj = np.where(c < adj, c, adj).astype(np.float32)                # std::min(adj, contrast)
        adj = np.where(adj < np.float32(1), np.float32(1), adj).astype(np.float32)  # std::max(adj, 1.0f)
        fn = (libm_logf(adj) / libm_logf(np.array([c]))[0]).astype(np.float32)
        fn = dr.libm_powf(fn, float(np.float32(gamma)))
        t = (np.float32(256.0) * fn).astype(np.float32)
        bad = np.isnan(t) | (t >= np.float32(2147483648.0)) | (t < np.float32(-2147483648.0))
        n = np.where(bad, np.int64(-2147483648), np.trunc(np.where(bad, 0, t)).astype(np.int64))  # cvttss2si
    return np.clip(n, 0, 255).astype(np.uint8)


def pgm_ref(px, W, H, smooth_side=0, max_side=0, contrast=500.0, gamma=0.6, max_value=0.0, pixel_max=None):
    """{smoothed, gray8, stats} of ipt_pgm_device, the max_value rules of
    include/ipt_capi.h included."""
    px = np.ascontiguousarray(px, np.float32).reshape(-1)
    assert px.size == W * H
    mx = np.float32(max_value)
    if pixel_max is not None:
        mx = fold_max0(pixel_max)
    plane = px.copy()
    if smooth_side >= 2:
        plane, mx = smooth(px, W, H, smooth_side)
    if max_side >= 2:
        mx = smooth(plane, W, H, max_side)[1]
    stats = np.array([mx, libm_logf(np.array([contrast], np.float32))[0], 0, 0], np.float32)
    return {"smoothed": plane, "gray8": n_val(plane, mx, contrast, gamma), "stats": stats}


# ---- inputs shared by the CPU and the GPU tests ------------------------------
TABLE_MAX = (0.0, 1.0, 1e-40, np.inf, np.nan, -1.0)
TABLE_VAL = (0.0, -0.0, -1.0, 1e-3, 0.5, 1.0, 2.0, 3e38, np.inf, np.nan)
# the issue's table (contrast 500, gamma 0.6), a g++ -O2 build of ipt::n_val
TABLE_WANT = {
    0.0: (0, 0, 0, 255, 255, 255, 255, 255, 255, 0),
    1.0: (0, 0, 0, 0, 238, 255, 255, 255, 255, 0),
    1e-40: (0, 0, 0, 255, 255, 255, 255, 255, 255, 0),
    np.inf: (0,) * 10,
    "nan": (0,) * 10,
    -1.0: (0, 0, 255, 0, 0, 0, 0, 0, 0, 0),
}


def table_want(mx):
    return TABLE_WANT["nan" if np.isnan(mx) else mx]


def random_plane(W, H, seed):
    """A render-like plane: mostly dim, a few bright pixels, some exact zeros."""
    rng = np.random.default_rng(seed)
    img = (rng.random(W * H, dtype=np.float32) ** 3 * np.float32(0.8)).astype(np.float32)
    img[rng.choice(W * H, max(W * H // 50, 1), replace=False)] = np.float32(0.0)
    hot = rng.choice(W * H, max(W * H // 100, 1), replace=False)
    img[hot] = (rng.random(hot.size, dtype=np.float32) * 30 + np.float32(1.0)).astype(np.float32)
    return img
