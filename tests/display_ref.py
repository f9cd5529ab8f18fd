"""CPU reference of the display pipeline (ipt_display / ipt_display_device):
Gui::updateDisplay's glare -> normalize -> Gui::save's normalize(0,255) and
8-bit cast, restated from independent parts:

  glare      the oracle's ipt_oracle_glare (pinned to the reference's compiled
             gui.cpp glare() by tests/golden/ref_glare.bin, tests/test_post.py)
  folds      numpy float32; `mx = max(mx, v)` from element 0 keeps the first
             maximum and skips NaN unless element 0 is one
  powf       the host libm's, through tests/native/powf_ref.c
"""
import ctypes as C
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
GAMMA = np.float32(np.float32(1.0) / np.float32(2.2))  # (float)(double)(1.0f / 2.2f)

_powf_lib = None


def powf_lib():
    global _powf_lib
    if _powf_lib is None:
        so = Path(tempfile.mkdtemp(prefix="powf_ref")) / "powf_ref.so"
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-builtin", "-o", str(so),
                        str(HERE / "native" / "powf_ref.c"), "-lm", "-lpthread"], check=True)
        lib = C.CDLL(str(so))
        lib.powf_eval.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_long, C.c_int]
        lib.powf_eval.restype = None
        _powf_lib = lib
    return _powf_lib


def libm_powf(x, y):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    powf_lib().powf_eval(x.ctypes.data, C.c_float(y), out.ctypes.data, x.size, min(16, os.cpu_count() or 1))
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cut01(v):
    """cimg::cut(v, 0, 1): v < 0 ? 0 : (v > 1 ? 1 : v); NaN passes."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(v < 0, np.float32(0), np.where(v > 1, np.float32(1), v)).astype(np.float32)


def fold_max(a):
    """std::max fold from element 0: (mx < v) ? v : mx."""
    return a[0] if np.isnan(a[0]) else a[np.nanargmax(a)]


def fold_min(a):
    return a[0] if np.isnan(a[0]) else a[np.nanargmin(a)]


def oracle_glare(img, W, H, cutoff):
    import oracle_binding as ob

    lib = ob.load()
    lib.ipt_oracle_glare.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float]
    src = np.ascontiguousarray(img, np.float32)
    out = np.empty_like(src)
    lib.ipt_oracle_glare(src.ctypes.data, out.ctypes.data, W, H, C.c_float(cutoff))
    return out


def glare_golden_cases():
    """[(W, H, cutoff, input, glare(input, cutoff))] of tests/golden/ref_glare.bin,
    the outputs of the reference's own compiled gui.cpp glare()."""
    d = np.fromfile(HERE / "golden" / "ref_glare.bin", np.float32)
    n, pos, out = int(d[0]), 1, []
    for _ in range(n):
        W, H, cutoff = int(d[pos]), int(d[pos + 1]), d[pos + 2]
        pos += 3
        inp = d[pos:pos + W * H]
        pos += W * H
        ref = d[pos:pos + W * H]
        pos += W * H
        out.append((W, H, cutoff, inp, ref))
    return out


def tone_map(processed):
    p = np.ascontiguousarray(processed, np.float32)
    with np.errstate(all="ignore"):
        v = (p / fold_max(p)).astype(np.float32)
    return cut01(libm_powf(v, GAMMA))


def to_gray8(tone):
    t = np.ascontiguousarray(tone, np.float32)
    m, M = fold_min(t), fold_max(t)
    if m == M:
        return np.zeros(t.size, np.uint8)
    with np.errstate(all="ignore"):
        v = ((t - m) / (M - m) * np.float32(255.0) + np.float32(0.0)).astype(np.float32)
    return np.where(np.isnan(v), np.float32(0), v).astype(np.uint8)  # NaN -> 0, stated


def display_ref(pixels, W, H, glare_cutoff=0.0):
    """{processed, tone, gray8} of a W x H float32 image (flat arrays). A
    glare_cutoff > 0 needs the built oracle (the `oracle` fixture)."""
    px = np.ascontiguousarray(pixels, np.float32).reshape(-1)
    assert px.size == W * H
    processed = oracle_glare(px, W, H, glare_cutoff) if glare_cutoff > 0 else px.copy()
    tone = tone_map(processed)
    return {"processed": processed, "tone": tone, "gray8": to_gray8(tone)}
