#!/usr/bin/env python3
"""What ``WanPipeline.__call__(edit_region=True, edit_region_follow=0)`` saves and what it adds, the moving-box arm of
tools/bench_edit_region.py, at 81f@1080x1920: a mask of 81 x 1080 x 1920 pixels, the loop state 16 x 43 x 135 x 240 in bf16 ([source 21
| grounding 1 | target 21] latent frames), Wan2.1-14B random-init weights, no guidance, ``spatial_window=(480, 832)``.  The mask is a
rectangle of 200 x 200 pixels that crosses the frame, 64 pixels per latent frame: its union box is wider than one tile of 60 x 104 cells
and runs as tiles inside the region, its own box fits one tile.

    python tools/bench_edit_region_follow.py [--rounds 2] [--layers 40] [--kernels-only] [--steps 1] [--log PATH]

The protocol of tools/bench_edit_region.py: one process, warm, alternating, HIP-event time.  The two kernels are timed alone, each
beside ``Tensor.copy_`` over as many bytes as the kernel moves (read + written), beside itself with constant origins (the box of latent
frame 10 for every frame) and beside the frames form on those same bytes, in rotating order, minimum of 8 (each sample is one call of
the ``ops`` function between two HIP events, so it holds that call's host work as well as the launch); then the per-call overhead as the pipeline
runs it -- bounds, their copy to the host (the one synchronisation), the rule, the two crops, the restore -- in wall time, minimum of 5.
Then ``--steps`` denoise steps of the same ``WanPipeline`` call with ``edit_region_follow=0`` against ``edit_region=True`` alone,
``output_type='latent'``, alternating (follow, union, follow, union, ...), minimum of ``--rounds``.  The expectations -- not asserted --
are parity of the two kernels with the frames forms, and a call ratio of about the tile ratio.  Prints one JSON line and appends it to
``--log`` (default profiles/r17/edit_region_follow_ab.log).  A protocol for a measurement, not a pass criterion."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--kernels-only", action="store_true", help="time the two kernels and the per-call overhead only (no model)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r17", "edit_region_follow_ab.log"))
    args = ap.parse_args()
    from videocof_amd import (FlowUniPCMultistepScheduler, WanPipeline, WanTransformer3DModel, ops, region_plan, region_track_plan)
    from videocof_amd.weights import random_dit_state_dict

    dev = torch.device("cuda", 0)
    dim, ffn, heads = 5120, 13824, 40
    T, H, W, C, Fs, G, h, w = 81, 1080, 1920, 16, 21, 1, 135, 240
    margin, tile, windows = (64, 64), (60, 104), dict(spatial_window=(480, 832))
    g = torch.Generator(device=dev).manual_seed(0)
    alpha = torch.zeros(T, H, W, device=dev, dtype=torch.uint8)
    for f in range(Fs):                                          # 200 x 200 pixels, 64 pixels to the right per latent frame
        frames = slice(0, 1) if f == 0 else slice(4 * f - 3, 4 * f + 1)
        alpha[frames, 400:600, 80 + 64 * f:280 + 64 * f] = 255
    weights = ops.latent_mask(alpha[None], 1, 0, 1)
    lat = torch.randn(1, C, 2 * Fs + G, h, w, device=dev, generator=g).bfloat16()
    rule = (h, w), (margin[0] // 8, margin[1] // 8), tile, 2

    def plans():
        bounds = ops.mask_bounds(weights).cpu()
        return region_track_plan(bounds, *rule, span=0), bounds
    track, bounds = plans()
    union = region_plan(bounds, *rule)
    assert (track.h, track.w) == tile and union.w > tile[1], (track, union)
    table = np.concatenate([track.origins, track.origins[:G], track.origins])
    runs = [(0, 2 * Fs + G)]
    es = lat.element_size()
    result = {"what": "edit_region_follow=0 at 81 x 1080 x 1920 / state 16 x 43 x 135 x 240 bf16, spatial_window (480, 832): the two kernels "
                      "beside a plain copy of the bytes they move, with constant origins and beside the frames forms on those bytes (us, min of 8), the "
                      f"per-call overhead (us, wall, min of 5), and {args.steps} step(s) of a Wan2.1-14B call ({args.layers} layers, no "
                      "guidance) with the following box and with the union box (ms, HIP events)",
              "box_cells": [track.h, track.w], "corner_columns": track.origins[:, 1].tolist(), "corner_rows": track.origins[:, 0].tolist(),
              "union_cells": list(union)}
    mid = tuple(int(v) for v in track.origins[Fs // 2])
    fixed = (mid[0], mid[1], track.h, track.w)
    state_r = ops.region_crop_track(lat, runs, table, tile)
    source = lat[:, :, :Fs].contiguous()
    full = torch.empty_like(lat)
    still, still_s = np.array([mid] * (2 * Fs + G), np.int32), np.array([mid] * Fs, np.int32)     # the track forms on the frames forms' bytes
    kern = {}
    for key, fn, const, same, nbytes in (
            ("region_crop_track_state", lambda: ops.region_crop_track(lat, runs, table, tile, out=state_r),
             lambda: ops.region_crop_track(lat, runs, still, tile, out=state_r),
             lambda: ops.region_crop_frames(lat, runs, fixed, out=state_r), 2 * state_r.numel() * es),
            ("region_restore_track", lambda: ops.region_restore_track(source, state_r, track.origins, (0, Fs), out=full),
             lambda: ops.region_restore_track(source, state_r, still_s, (0, Fs), out=full),
             lambda: ops.region_restore_frames(source, state_r, mid, (0, Fs), out=full), 2 * full.numel() * es)):
        src = torch.empty(max(nbytes // 4, 1), device=dev, dtype=torch.bfloat16)
        dst = torch.empty_like(src)
        forms = [("kernel", fn), ("constant_origins", const), ("frames_form", same), ("copy", lambda: dst.copy_(src))]
        for _, f in forms:
            f()
        us = {name: [] for name, _ in forms}
        for r in range(8):                                       # every form after every other one: the order rotates
            for name, f in forms[r % 4:] + forms[:r % 4]:
                us[name].append(timed(f)[0] * 1e3)
        kern[key] = {"bytes": nbytes, **{f"{name}_us_min": round(min(v), 1) for name, v in us.items()},
                     **{f"{name}_tbps": round(nbytes / min(v) / 1e6, 3) for name, v in us.items()}}
        del src, dst
    result["kernels"] = kern

    def per_call():                                              # what the two stages of the pipeline run, in its order
        p, _ = plans()
        tb = np.concatenate([p.origins, p.origins[:G], p.origins])
        s, _ = ops.region_crop_track(lat, runs, tb, (p.h, p.w)), ops.region_crop_track(weights, [(0, Fs)], p.origins, (p.h, p.w))
        return ops.region_restore_track(lat[:, :, :Fs], s, p.origins, (0, Fs))
    walls = []
    for _ in range(6):
        torch.cuda.synchronize()
        t_wall = time.perf_counter()
        per_call()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t_wall) * 1e6)
    result["per_call_overhead_us"] = {"wall_us_min": round(min(walls[1:]), 1), "wall_us": [round(v, 1) for v in walls[1:]]}
    if not args.kernels_only:
        model = WanTransformer3DModel(dim=dim, ffn_dim=ffn, num_heads=heads, num_layers=args.layers)
        model.load_state_dict(random_dit_state_dict(dev, seed=0, dim=dim, ffn_dim=ffn, num_layers=args.layers), device=dev)
        pipe = WanPipeline(transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))
        ctx = torch.randn(37, 4096, device=dev, generator=g).bfloat16()

        def call(**kw):
            return pipe(latents=lat, prompt_embeds=[ctx], source_frames=T, reasoning_frames=4, height=H, width=W,
                        num_inference_steps=args.steps, guidance_scale=1.0, cot=True, output_type="latent", return_dict=True,
                        edit_mask=alpha, edit_region=True, edit_region_margin=margin, **windows, **kw)
        forms = (("follow", lambda: call(edit_region_follow=0)), ("union", lambda: call()))
        times = {"follow": [], "union": []}
        for key, fn in forms:                                    # warm-up: workspaces, text K/V, kernel attributes
            ms, out = timed(fn)
            print(f"[warm] {key}: {ms:.0f} ms, edit_region={out.edit_region}", flush=True)
        for r in range(args.rounds):
            for key, fn in forms:
                ms, out = timed(fn)
                times[key].append(ms)
                print(f"[round {r}] {key}: {ms:.0f} ms", flush=True)
                assert bool(torch.isfinite(out.latents).all()) and tuple(out.latents.shape) == tuple(lat.shape)
        fo, un = min(times["follow"]), min(times["union"])
        result["call"] = {"steps": args.steps, "follow_ms": [round(v, 1) for v in times["follow"]],
                          "union_ms": [round(v, 1) for v in times["union"]], "follow_ms_min": round(fo, 1),
                          "union_ms_min": round(un, 1), "union_over_follow": round(un / fo, 3)}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
