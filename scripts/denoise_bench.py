#!/usr/bin/env python3
"""Measures the denoiser: the guide pass, the prepare pass and every iteration
of ipt_denoise_device in both tap-loop forms, against their traffic floors and
against one full-estimator render pass of the same frame.

Not a test and not the benchmark (bench.py): one MI355X, the box scene at C2's
frame (1024^2) and C5's (2048^2), n_rays 16, depth_max 8. The plane is 4
passes through ipt_render_masked_device with m2; the filter runs its 5
default iterations. Kernel times are HIP events around each pass inside the
call (ipt_denoise_pass_ms, IPT_DENOISE_PROFILE=1). The guide pass is timed by
events recorded on a stream of the script's own, whose handle the call gets
(handle 0, torch's default stream, would mean the context's own stream, which
events on the default stream do not bracket): from before ipt_guides_device
to behind its scatter, so the span holds the work-slot stream's two memsets,
the preview kernel, the cross-stream wait and the scatter ("guides_ms");
"guides_preview_ms" is the library's own event time of the preview launch
alone (ipt_last_kernel_ms). A render pass is ipt_last_kernel_ms of a 16-pass
ipt_render_device launch / 16.

The forms (IPT_DENOISE_FORM = direct, tiled, and unset: the library's choice)
run alternating, --runs rounds (5) after one warm-up round, their order
rotated from round to round (the pass that follows the render launch runs a
few microseconds slower, whichever form it is); a line holds the medians,
every run and the spread (max - min) / median of the call's total.

Floors, per pass, from the bytes the pass must move (MI355X_MICROARCH.md):
  compulsory  every byte once, at the 6.29 TB/s a streaming copy reaches from
              HBM (the planes of a 1024^2 frame also fit the 256 MiB Infinity
              Cache; the HBM figure is the conservative one):
              prepare 44 B read + 32 B written per pixel; an iteration 32 B
              read + 32 B written, the last one 32 B read + 8 B written
              (colour and variance)
  gather      an iteration's 25 taps x 32 B + 9 x 4 B of the prefilter per
              pixel at the 34.5 TB/s aggregate L2 rate (the direct form's
              reads; the tiled form reads (36 x 12) / (32 x 8) records per
              pixel from global memory and its taps from LDS)
One JSON line per frame and form, appended to --out (default
profiles/denoise_bench.jsonl).

    python3 scripts/denoise_bench.py [--runs 5] [--sizes 1024,2048] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402  (torch's HIP runtime first, as bench.py)

from ipt_amd import capi, scenes  # noqa: E402

HBM_BPS, L2_BPS = 6.29e12, 34.5e12
FORMS = ("auto", "direct", "tiled")
ITER = capi.DENOISE_DEFAULTS["iterations"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sizes", default="1024,2048")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "denoise_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("denoise_bench.py needs a gfx950 device")
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    os.environ["IPT_DENOISE_PROFILE"] = "1"
    ctx = capi.Context(0)
    ctx.upload_scene(scenes.make_scene_box())
    lines = []
    for size in (int(s) for s in a.sizes.split(",")):
        W = H = size
        n = W * H
        pixels = torch.zeros(n, dtype=torch.float32, device=dev)
        counters = torch.zeros(n, dtype=torch.int32, device=dev)
        m2 = torch.zeros(n, dtype=torch.float32, device=dev)
        guides = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        out = torch.zeros(n, dtype=torch.float32, device=dev)
        var = torch.zeros(n, dtype=torch.float32, device=dev)
        scratch_px = torch.zeros(n, dtype=torch.float32, device=dev)
        scratch_cn = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.render_masked_device(capi.make_params(W, H, 4, n_rays=16, depth_max=8), pixels.data_ptr(),
                                 counters.data_ptr(), m2_ptr=m2.data_ptr())
        gp = capi.make_params(W, H, 1)
        dp = capi.make_denoise_params(W, H)
        stream = torch.cuda.Stream()  # (a real handle: 0 would select the context's own stream)
        assert stream.cuda_stream != 0
        torch.cuda.synchronize()

        def guides_ms():
            """(events on `stream` around the whole call, the preview launch's own time)"""
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx.guides_device(gp, guides.data_ptr(), stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            ctx.wait()
            return e0.elapsed_time(e1), ctx.last_kernel_ms()[0]

        def denoise_ms(form):
            if form == "auto":
                os.environ.pop("IPT_DENOISE_FORM", None)
            else:
                os.environ["IPT_DENOISE_FORM"] = form
            ctx.denoise_device(dp, pixels.data_ptr(), counters.data_ptr(), m2.data_ptr(), guides.data_ptr(),
                               out.data_ptr(), var.data_ptr(), stream.cuda_stream)
            ms = ctx.denoise_pass_ms()[:1 + ITER]  # (waits for the call)
            stream.synchronize()
            return ms

        def render_pass_ms():
            scratch_px.zero_()
            scratch_cn.zero_()
            torch.cuda.synchronize()
            ctx.render_device(capi.make_params(W, H, 16, n_rays=16, depth_max=8), scratch_px.data_ptr(),
                              scratch_cn.data_ptr())
            return ctx.last_kernel_ms()[0] / 16.0

        guides_ms()
        render_pass_ms()
        ref = None
        for f in FORMS:  # warm-up, and the forms' outputs are the same bits
            denoise_ms(f)
            torch.cuda.synchronize()
            bits = out.view(torch.int32).clone()
            assert ref is None or torch.equal(bits, ref), f
            ref = bits
        g_runs, r_runs, d_runs = [], [], {f: [] for f in FORMS}
        for r in range(a.runs):  # alternating, the forms' order rotated
            g_runs.append(guides_ms())
            r_runs.append(render_pass_ms())
            for k in range(len(FORMS)):
                f = FORMS[(r + k) % len(FORMS)]
                d_runs[f].append(denoise_ms(f))
        g_med = statistics.median(g[0] for g in g_runs)
        part = int(((guides.view(torch.int32).view(-1, 8)[:, 3] & 3) == 1).sum().item())
        render_ms = statistics.median(r_runs)
        floor_prepare = n * 76 / HBM_BPS * 1e3
        floor_iter = [n * (64 if k < ITER - 1 else 40) / HBM_BPS * 1e3 for k in range(ITER)]
        floor_gather = n * (25 * 32 + 9 * 4) / L2_BPS * 1e3
        for f in FORMS:
            runs = d_runs[f]
            med = [statistics.median(r[k] for r in runs) for k in range(1 + ITER)]
            totals = [sum(r) for r in runs]
            total = statistics.median(totals)
            line = {"frame": size, "form": f, "iterations": ITER, "runs": a.runs, "surface_pixels": part,
                    "guides_ms": g_med, "guides_ms_runs": [g[0] for g in g_runs],
                    "guides_preview_ms": statistics.median(g[1] for g in g_runs),
                    "guides_floor_scatter_ms": n * 57 / HBM_BPS * 1e3,
                    "prepare_ms": med[0], "iteration_ms": med[1:], "denoise_total_ms": total,
                    "denoise_total_ms_runs": totals, "total_spread": (max(totals) - min(totals)) / total,
                    "pass_ms_runs": runs,
                    "floor_compulsory_prepare_ms": floor_prepare, "floor_compulsory_iteration_ms": floor_iter,
                    "floor_gather_iteration_ms": floor_gather,
                    "prepare_fraction_of_floor": floor_prepare / med[0] if med[0] > 0 else 0.0,
                    "iteration_fraction_of_compulsory": [fl / m if m > 0 else 0.0 for fl, m in zip(floor_iter, med[1:])],
                    "iteration_fraction_of_gather": [floor_gather / m if m > 0 else 0.0 for m in med[1:]],
                    "render_pass_ms": render_ms, "render_pass_ms_runs": r_runs,
                    "denoise_plus_guides_in_render_passes": (total + g_med) / render_ms}
            lines.append(line)
            print(json.dumps(line), flush=True)
    ctx.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
