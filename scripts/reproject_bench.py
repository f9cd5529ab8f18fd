#!/usr/bin/env python3
"""Measures temporal reprojection: ipt_reproject_device's kernel time against
its traffic floor and against one full-estimator render pass of the same
frame, and what the adaptive loop gains from it after a camera move.

Not a test and not the benchmark (bench.py): one MI355X, the box scene,
n_rays 16, depth_max 8.

Kernel time (--sizes, 1024 and 2048): the history is 4 passes through
ipt_render_masked_device with m2 at the previous camera, then both guide
planes. Two moves: "small" (the previous camera 0.02, 0, 0.01 away: the four
taps of neighbouring pixels are neighbours) and "large" (1.2, 0, 0 away: the
gathers are scattered and much of the frame finds no history). A run is
--calls (20) back-to-back calls between two events on a stream of the
script's own, whose handle the calls get; the time is per call and holds the
call's 16-byte stats memset. Five runs after a warm-up one, alternating the
moves; a line holds the median, every run and the spread (max - min) /
median. A render pass is ipt_last_kernel_ms of a 16-pass ipt_render_device
launch / 16, timed in the same round.

Floor: the bytes a call must move once -- 32 B of the pixel's own guide, one
32 B guide and 12 B of planes of history, 12 B written: 88 B per pixel -- at the
6.29 TB/s a streaming copy reaches from HBM (MI355X_MICROARCH.md; the figure
DESIGN.md 4.17 uses). Pixels that are no surface or find no history move less,
so the floor is an upper bound of the compulsory traffic.

Loop gain (--loop-size, 1024, C2's frame): 16 passes at the previous camera
(the CPU test's move, 0.15, 0, 0.05), then the adaptive loop at the new one
with the adaptive defaults (min_count 8, rel_tol 0.05, abs_tol 1e-3) in rounds
of 4 passes until ipt_adapt_device reports no active pixel or --loop-cap
passes are used: once from the reprojected planes (the first round is masked
already) and once from zero (the first round traces every pixel). A line holds
the passes, the traced samples (the masks' active pixels times the passes)
and the time of each loop, --loop-runs (3) runs alternating.

One JSON line per measurement, appended to --out (default
profiles/reproject_bench.jsonl).

    python3 scripts/reproject_bench.py [--runs 5] [--sizes 1024,2048] [--loop-size 1024] [--out FILE]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime first, as bench.py)

from ipt_amd import capi, scenes  # noqa: E402

HBM_BPS = 6.29e12
BYTES_PER_PIXEL = 88
MOVES = {"small": (0.02, 0.0, 0.01), "large": (1.2, 0.0, 0.0)}
LOOP_MOVE = (0.15, 0.0, 0.05)
RENDER = dict(n_rays=16, depth_max=8)
F = np.float32


def moved(desc, shift):
    """The scene seen from its camera displaced by `shift` (right and up depend
    on the direction and the up hint alone)."""
    cam = dict(desc["camera"])
    cam["position"] = (np.array(cam["position"], F) + np.array(shift, F)).astype(F).tolist()
    return dict(desc, camera=cam)


class Planes:
    def __init__(self, n, dev):
        self.px = torch.zeros(n, dtype=torch.float32, device=dev)
        self.cn = torch.zeros(n, dtype=torch.int32, device=dev)
        self.m2 = torch.zeros(n, dtype=torch.float32, device=dev)

    def zero(self):
        self.px.zero_(), self.cn.zero_(), self.m2.zero_()


def history(ctx, box, shift, W, H, spp, prev, pg, cg):
    """spp passes with m2 and the guides at the previous camera, then the new
    camera and its guides."""
    prev.zero()
    torch.cuda.synchronize()
    ctx.upload_scene(moved(box, shift))
    ctx.render_masked_device(capi.make_params(W, H, spp, **RENDER), prev.px.data_ptr(), prev.cn.data_ptr(),
                             m2_ptr=prev.m2.data_ptr())
    gp = capi.make_params(W, H, 1)
    ctx.guides_device(gp, pg.data_ptr())
    ctx.upload_scene(box)
    ctx.guides_device(gp, cg.data_ptr())
    ctx.wait()
    torch.cuda.synchronize()


def kernel_times(ctx, a, dev, size, lines):
    W = H = size
    n = W * H
    box = scenes.make_scene_box()
    stream = torch.cuda.Stream()  # (a real handle: 0 would select the context's own stream)
    assert stream.cuda_stream != 0
    cur, stats = Planes(n, dev), torch.zeros(4, dtype=torch.int32, device=dev)
    sets = {}
    for name, shift in MOVES.items():
        prev = Planes(n, dev)
        pg, cg = (torch.zeros(n * 32, dtype=torch.uint8, device=dev) for _ in range(2))
        history(ctx, box, shift, W, H, 4, prev, pg, cg)
        sets[name] = (prev, pg, cg, capi.make_reproject_params(W, H, moved(box, shift)["camera"]))
    scratch = Planes(n, dev)

    def reproject_ms(name):
        prev, pg, cg, rp = sets[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.calls):
            ctx.reproject_device(rp, prev.px.data_ptr(), prev.cn.data_ptr(), prev.m2.data_ptr(), pg.data_ptr(),
                                 cg.data_ptr(), cur.px.data_ptr(), cur.cn.data_ptr(), cur.m2.data_ptr(),
                                 stats.data_ptr(), stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        ctx.wait()
        return e0.elapsed_time(e1) / a.calls

    def render_pass_ms():
        scratch.zero()
        torch.cuda.synchronize()
        ctx.render_device(capi.make_params(W, H, 16, **RENDER), scratch.px.data_ptr(), scratch.cn.data_ptr())
        return ctx.last_kernel_ms()[0] / 16.0

    names = list(MOVES)
    for name in names:  # warm-up
        reproject_ms(name)
    render_pass_ms()
    runs, r_runs, st = {k: [] for k in names}, [], {}
    for r in range(a.runs):
        r_runs.append(render_pass_ms())
        for k in range(len(names)):
            name = names[(r + k) % len(names)]
            runs[name].append(reproject_ms(name))
            st[name] = stats.cpu().numpy().view(np.uint32)[:3].tolist()
    floor = n * BYTES_PER_PIXEL / HBM_BPS * 1e3
    render_ms = statistics.median(r_runs)
    for name in names:
        med = statistics.median(runs[name])
        line = {"measure": "kernel", "frame": size, "move": name, "shift": MOVES[name], "runs": a.runs,
                "calls_per_run": a.calls, "reused": st[name][0], "disoccluded": st[name][1],
                "not_surface": st[name][2], "reproject_ms": med, "reproject_ms_runs": runs[name],
                "spread": (max(runs[name]) - min(runs[name])) / med, "floor_compulsory_ms": floor,
                "fraction_of_floor": floor / med, "render_pass_ms": render_ms, "render_pass_ms_runs": r_runs,
                "reproject_in_render_passes": med / render_ms}
        lines.append(line)
        print(json.dumps(line), flush=True)


def loop_gain(ctx, a, dev, lines):
    W = H = a.loop_size
    n = W * H
    box = scenes.make_scene_box()
    prev, cur = Planes(n, dev), Planes(n, dev)
    pg, cg = (torch.zeros(n * 32, dtype=torch.uint8, device=dev) for _ in range(2))
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    stats, rstats = (torch.zeros(4, dtype=torch.int32, device=dev) for _ in range(2))
    history(ctx, box, LOOP_MOVE, W, H, 16, prev, pg, cg)
    rp = capi.make_reproject_params(W, H, moved(box, LOOP_MOVE)["camera"])
    ap = capi.make_adapt_params(W, H)  # the adaptive defaults

    def adapt():
        ctx.adapt_device(ap, cur.px.data_ptr(), cur.cn.data_ptr(), cur.m2.data_ptr(), mask.data_ptr(), stats.data_ptr())
        ctx.wait()
        torch.cuda.synchronize()
        return int(stats.cpu().numpy().view(np.uint32)[0])

    def loop(reproject):
        cur.zero()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        passes, samples, offset, rs = 0, 0, 0, None
        if reproject:
            ctx.reproject_device(rp, prev.px.data_ptr(), prev.cn.data_ptr(), prev.m2.data_ptr(), pg.data_ptr(),
                                 cg.data_ptr(), cur.px.data_ptr(), cur.cn.data_ptr(), cur.m2.data_ptr(),
                                 rstats.data_ptr())
            offset = 16
            active = adapt()
            rs = rstats.cpu().numpy().view(np.uint32)[:3].tolist()
        else:
            active = n  # round 0 traces every pixel
        first_active = active
        while active and passes < a.loop_cap:
            masked = reproject or passes > 0
            ctx.render_masked_device(capi.make_params(W, H, 4, spp_offset=offset + passes, **RENDER), cur.px.data_ptr(),
                                     cur.cn.data_ptr(), mask_ptr=mask.data_ptr() if masked else None,
                                     m2_ptr=cur.m2.data_ptr())
            passes += 4
            samples += 4 * active
            active = adapt()
        return dict(passes=passes, traced_samples=samples, first_round_active=first_active, left_active=active,
                    seconds=time.perf_counter() - t0, reproject_stats=rs)

    loop(True)  # warm-up
    res = {True: [], False: []}
    for r in range(a.loop_runs):
        for k in ((True, False) if r % 2 == 0 else (False, True)):
            res[k].append(loop(k))
    for k, name in ((True, "reprojected"), (False, "from_zero")):
        secs = [x["seconds"] for x in res[k]]
        med = statistics.median(secs)
        line = dict(res[k][0], measure="loop", frame=a.loop_size, start=name, shift=LOOP_MOVE, history_passes=16,
                    adapt=dict(min_count=ap.min_count, rel_tol=ap.rel_tol, abs_tol=ap.abs_tol), round_spp=4,
                    cap=a.loop_cap, runs=a.loop_runs, seconds=med, seconds_runs=secs,
                    spread=(max(secs) - min(secs)) / med, passes_runs=[x["passes"] for x in res[k]])
        lines.append(line)
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sizes", default="1024,2048")
    ap.add_argument("--loop-size", type=int, default=1024)
    ap.add_argument("--loop-cap", type=int, default=512)
    ap.add_argument("--loop-runs", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "reproject_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("reproject_bench.py needs a gfx950 device")
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    lines = []
    for size in (int(s) for s in a.sizes.split(",") if s):
        kernel_times(ctx, a, dev, size, lines)
    if a.loop_size > 0:
        loop_gain(ctx, a, dev, lines)
    ctx.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
