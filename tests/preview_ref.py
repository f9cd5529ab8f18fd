"""Builds and binds tests/native/preview_ref.cpp, the reference restatement of
the preview estimator (render_sample's loop with ray_power_preview, from the
oracle's own leaves). Test infrastructure only. The shared object goes into a
temporary directory of the test process (nothing is written under oracle/),
compiled with the oracle Makefile's CXXFLAGS."""
from __future__ import annotations

import atexit
import ctypes as C
import functools
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from ipt_amd import capi

ROOT = Path(__file__).resolve().parents[1]
SRC = Path(__file__).resolve().parent / "native" / "preview_ref.cpp"

OUTCOME_MISS, OUTCOME_SURFACE, OUTCOME_LIGHT = 0, 1, 2
KIND_SI, KIND_LI = 4, 8
# the counters the preview's events define; the others stay 0 (the
# acceleration-structure counters hold what the kernel ran)
EVENT_COUNTERS = ("paths", "traced_rays", "surface_hits", "light_hits", "light_traces", "drifted")
ZERO_COUNTERS = ("expanded_nodes", "iterations", "light_samples", "skipped", "sphere_frames")


def oracle_cxxflags():
    txt = (ROOT / "oracle" / "Makefile").read_text()
    return re.search(r"^CXXFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


@functools.lru_cache(maxsize=None)
def load():
    d = Path(tempfile.mkdtemp(prefix="ipt_preview_ref_"))
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = d / "libpreview_ref.so"
    subprocess.run(["g++", *oracle_cxxflags(), "-Wno-unused-function", "-I", str(ROOT / "include"), "-shared",
                    "-o", str(so), str(SRC), "-lpthread"], check=True)
    lib = C.CDLL(str(so))
    lib.ipt_preview_ref.argtypes = [C.POINTER(capi.Scene), C.POINTER(capi.Params)] + [C.c_void_p] * 4 + [
        C.POINTER(capi.Counters)]
    return lib


def render(scene_desc: dict, p):
    """(values, codes, kinds [spp][H][W], hits [spp][H][W][6], counters dict)
    of the reference restatement; p.flags' IPT_FLAG_GUI_PLANE selects the
    Gui's codes, n_rays and depth_max are not read."""
    lib = load()
    s, keep = capi.make_scene(scene_desc)
    n = p.spp * p.width * p.height
    vals, codes, kinds = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    hits = np.zeros(6 * n, np.float32)
    cnt = capi.Counters()
    rc = lib.ipt_preview_ref(C.byref(s), C.byref(p), vals.ctypes.data, codes.ctypes.data, kinds.ctypes.data,
                             hits.ctypes.data, C.byref(cnt))
    assert rc == 0, rc
    shape = (p.spp, p.height, p.width)
    out = (vals.reshape(shape), codes.reshape(shape), kinds.reshape(shape), hits.reshape(shape + (6,)))
    for a in out:
        a.setflags(write=False)
    return out + (cnt.as_dict(),)


def classes(kinds: np.ndarray) -> dict:
    """The outcome histogram and both-hit classes of a kinds array."""
    o = kinds & 3
    both = (kinds & (KIND_SI | KIND_LI)) == (KIND_SI | KIND_LI)
    return {"outcomes": [int((o == k).sum()) for k in range(3)],
            "surface_wins": int((both & (o == OUTCOME_SURFACE)).sum()),
            "light_wins": int((both & (o == OUTCOME_LIGHT)).sum()),
            "light_alone": int(((o == OUTCOME_LIGHT) & ((kinds & KIND_SI) == 0)).sum())}
