#!/usr/bin/env python3
"""Measures what a masked launch costs: path and accumulate kernel time against
the share of active pixels.

Not a test and not the benchmark (bench.py): one MI355X, the C2 frame (box,
1024^2, n_rays 16, depth_max 8), 16 passes per launch through
ipt_render_masked_device into zeroed device planes, kernel times from
ipt_last_kernel_ms. Configurations:

  unmasked        ipt_render_device (no mask, no m2): this build's unmasked launch
  parent          the same call through the parent commit's library (--parent-lib,
                  a libipt_hip.so built from the parent's sources), if given
  m2              no mask, with the m2 plane (the ADAPT replay alone)
  share X         a seeded random mask with a fraction X of the pixels active
                  (1.0, 0.5, 0.25, 0.1, 0.01), with m2
  loop R          the mask the adaptive loop itself produces on this frame after
                  16 unmasked passes with rel_tol R (0.25, 0.05 and 0.02; abs_tol
                  1e-3, min_count 8: the dark lower half and the misses go
                  inactive first), with m2
  NAME compact    the compacted twin of every masked configuration above (share
                  X, loop R): the same call with IPT_FLAG_COMPACT
  shard           one shard (shard 1) of a 3-shard plan of 16-row tiles, no mask,
                  no m2; "shard compact" with IPT_FLAG_COMPACT (the halo rows of
                  the other shards leave the pool)

A line also holds ipt_last_units of the call: the launch's dense units, the
units its pool handed out and the units traced.

All configurations run alternating, --runs rounds (5) after one warm-up round;
a line holds the medians, every run, and the spread (max - min) / median of
the path time, so that a difference can be set against the run-to-run noise.
One JSON line per configuration, appended to --out (default
profiles/adaptive_bench.jsonl).

    python3 scripts/adaptive_bench.py [--parent-lib FILE] [--runs 5] [--spp 16] [--size 1024] [--out FILE]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime first, as bench.py)

from ipt_amd import capi, scenes  # noqa: E402

SHARES = (1.0, 0.5, 0.25, 0.1, 0.01)
LOOP_RULE = dict(min_count=8, abs_tol=1e-3)
LOOP_REL = (0.25, 0.05, 0.02)


def context_of(lib):
    """A capi.Context on a library other than the tree's own."""
    ctx = capi.Context.__new__(capi.Context)
    ctx.lib = lib
    h = C.c_void_p()
    rc = lib.ipt_create(0, C.byref(h))
    if rc != capi.IPT_OK:
        raise capi.IptError(rc, lib.ipt_last_error(None).decode(errors="replace"))
    ctx.h, ctx._keep = h, None
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "adaptive_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adaptive_bench.py needs a gfx950 device")
    torch.cuda.init()
    W = H = a.size
    n = W * H
    desc = scenes.make_scene_box()
    ctx = capi.Context(0)
    ctx.upload_scene(desc)
    parent = None
    if a.parent_lib:
        parent = context_of(capi.load(a.parent_lib))
        parent.upload_scene(desc)
    dev = torch.device("cuda", 0)
    pixels = torch.zeros(n, dtype=torch.float32, device=dev)
    counters = torch.zeros(n, dtype=torch.int32, device=dev)
    m2 = torch.zeros(n, dtype=torch.float32, device=dev)
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    p = capi.make_params(W, H, a.spp, n_rays=16, depth_max=8)
    pc = capi.make_params(W, H, a.spp, n_rays=16, depth_max=8, flags=capi.IPT_FLAG_COMPACT)
    shard = dict(tile_rows=16, n_shards=3, shard_id=1)
    ps = capi.make_params(W, H, a.spp, n_rays=16, depth_max=8, **shard)
    psc = capi.make_params(W, H, a.spp, n_rays=16, depth_max=8, flags=capi.IPT_FLAG_COMPACT, **shard)

    masks = {}
    rng = np.random.default_rng([W, H, 2])
    u = rng.random(n)
    for s in SHARES:
        masks["share %g" % s] = torch.from_numpy((u < s).astype(np.uint8)).to(dev)
    # the loop's own masks: 16 unmasked passes, then the rule
    ctx.render_masked_device(capi.make_params(W, H, 16, n_rays=16, depth_max=8), pixels.data_ptr(), counters.data_ptr(),
                             m2_ptr=m2.data_ptr())
    for rel in LOOP_REL:
        loop_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
        ctx.adapt_device(capi.make_adapt_params(W, H, rel_tol=rel, **LOOP_RULE), pixels.data_ptr(), counters.data_ptr(),
                         m2.data_ptr(), loop_mask.data_ptr(), stats.data_ptr())
        masks["loop %g" % rel] = loop_mask
    ctx.wait()
    torch.cuda.synchronize()

    def call(name):
        pixels.zero_()
        counters.zero_()
        m2.zero_()
        torch.cuda.synchronize()
        if name == "parent":
            parent.render_device(p, pixels.data_ptr(), counters.data_ptr())
            return parent.last_kernel_ms()
        if name == "unmasked":
            ctx.render_device(p, pixels.data_ptr(), counters.data_ptr())
        elif name in ("shard", "shard compact"):
            ctx.render_device(psc if name.endswith(" compact") else ps, pixels.data_ptr(), counters.data_ptr())
        elif name == "m2":
            ctx.render_masked_device(p, pixels.data_ptr(), counters.data_ptr(), m2_ptr=m2.data_ptr())
        else:
            compact = name.endswith(" compact")
            mask = masks[name[:-len(" compact")] if compact else name]
            ctx.render_masked_device(pc if compact else p, pixels.data_ptr(), counters.data_ptr(),
                                     mask_ptr=mask.data_ptr(), m2_ptr=m2.data_ptr())
        units[name] = ctx.last_units()
        return ctx.last_kernel_ms()

    units = {}
    names = ["unmasked"] + (["parent"] if parent else []) + ["m2"]
    for k in masks:
        names += [k, k + " compact"]
    names += ["shard", "shard compact"]
    for name in names:  # warm-up: every configuration once
        call(name)
    samples = {k: [] for k in names}
    for _ in range(a.runs):  # alternating
        for name in names:
            samples[name].append(call(name))
    base = statistics.median(x[0] for x in samples["parent" if parent else "unmasked"])
    lines = []
    for name in names:
        path, acc = zip(*samples[name])
        mp = statistics.median(path)
        mask_name = name[:-len(" compact")] if name.endswith(" compact") else name
        share = float(masks[mask_name].float().mean().item()) if mask_name in masks else 1.0
        line = {"config": name, "width": W, "height": H, "spp": a.spp, "n_rays": 16, "depth_max": 8, "runs": a.runs,
                "active_share": share, "path_ms": mp, "accumulate_ms": statistics.median(acc),
                "path_ms_runs": list(path), "accumulate_ms_runs": list(acc),
                "path_spread": (max(path) - min(path)) / mp if mp > 0 else 0.0,
                "path_vs_baseline": mp / base if base > 0 else 0.0,
                "baseline": "parent" if parent else "unmasked"}
        if name in units:
            line["units"] = list(units[name])
        lines.append(line)
        print(json.dumps(line), flush=True)
    ctx.close()
    if parent:
        parent.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
