#!/usr/bin/env python3
"""Measures the preview estimator against the cheapest full-estimator call.

Not a test and not the benchmark (bench.py): one MI355X, 1 spp, on the C2
frame (box, 1024^2), the C3 frame (10 000 spheres, 1024^2) and the C5 frame
(256 lights, 2048^2), each with

  preview   flags = IPT_FLAG_PREVIEW (preview_kernel)
  full0     flags = 0, n_rays = 0, depth_max = 1: the cheapest call the
            library had before (raygen_kernel + the persistent path kernel,
            its sampling tables built by the context's first render)

through ipt_render_device into device planes. Per frame and mode: the wall
time of the first call on a fresh context (where the tables' 1.2 GiB shows),
the device memory that call took, and the medians of five alternating runs
(preview, full0, preview, ...) of the wall time and of ipt_last_kernel_ms.
One JSON line per frame and mode, appended to --out (default
profiles/preview_bench.jsonl).

    python3 scripts/preview_bench.py [--frames c2,c3,c5] [--runs 5] [--out FILE]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402  (torch's HIP runtime first, as bench.py)

from ipt_amd import capi, scenes  # noqa: E402

FRAMES = {
    "c2": ("box 1024^2", scenes.make_scene_box, 1024, 1024),
    "c3": ("10 000 spheres 1024^2", lambda: scenes.make_scene_spheres(10000), 1024, 1024),
    "c5": ("256 lights 2048^2", lambda: scenes.make_scene_box_lights(16), 2048, 2048),
}
MODES = {
    "preview": dict(flags=capi.IPT_FLAG_PREVIEW),
    "full0": dict(flags=0, n_rays=0, depth_max=1),
}


class Run:
    def __init__(self, desc, W, H, mode):
        self.W, self.H, self.mode = W, H, mode
        self.ctx = capi.Context(0)
        self.ctx.upload_scene(desc)
        self.pixels = torch.zeros(W * H, dtype=torch.float32, device="cuda")
        self.counters = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        self.pass_ = 0

    def call(self):
        """One synchronous 1-spp call into a zeroed plane: (wall ms, path ms, accumulate ms)."""
        self.pixels.zero_()
        self.counters.zero_()
        torch.cuda.synchronize()
        p = capi.make_params(self.W, self.H, 1, spp_offset=self.pass_, **MODES[self.mode])
        self.pass_ += 1
        t0 = time.perf_counter()
        self.ctx.render_device(p, self.pixels.data_ptr(), self.counters.data_ptr())
        wall = (time.perf_counter() - t0) * 1e3
        k, a = self.ctx.last_kernel_ms()
        return wall, k, a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="c2,c3,c5")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "preview_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("preview_bench.py needs a gfx950 device")
    torch.cuda.init()
    # the process's first launches load the code objects: a throwaway context
    # runs both modes once, so a "first call" below is a fresh context's, not
    # a fresh process's
    for mode in MODES:
        w = Run(scenes.make_scene_box(), 64, 64, mode)
        w.call()
        w.ctx.close()
    lines = []
    for f in a.frames.split(","):
        label, build, W, H = FRAMES[f]
        desc = build()
        runs, first = {}, {}
        for mode in MODES:
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            r = Run(desc, W, H, mode)
            wall, k, acc = r.call()
            first[mode] = {"wall_ms": wall, "kernel_ms": k, "accumulate_ms": acc,
                           "device_bytes": free0 - torch.cuda.mem_get_info()[0]}
            runs[mode] = r
        samples = {m: [] for m in MODES}
        for _ in range(a.runs):  # alternating
            for m in MODES:
                samples[m].append(runs[m].call())
        for m in MODES:
            w, k, acc = zip(*samples[m])
            line = {"frame": f, "label": label, "width": W, "height": H, "spp": 1, "mode": m, "runs": a.runs,
                    "wall_ms": statistics.median(w), "kernel_ms": statistics.median(k),
                    "accumulate_ms": statistics.median(acc), "wall_ms_runs": list(w), "kernel_ms_runs": list(k),
                    "first_call": first[m], "pixel_mean": float(runs[m].pixels.mean().item())}
            lines.append(line)
            print(json.dumps(line), flush=True)
        for r in runs.values():
            r.ctx.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
